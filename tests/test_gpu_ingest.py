"""Frame ingest on the GPU (csrc/ingest.hip, sdflabel_amd/frame.py, pipelines/refinement.py, pipelines/frame.py refine_sample) against golden
G19 -- recorded from the reference's own functions and from PIL by tools/make_golden_ingest.py -- and against the numpy restatements of
tests/_ingest_ref.py, which tests/test_ingest_cpu.py pins to the same golden and to PIL.  Everything is exact: integers, bytes and float
bits are compared for equality, so there is no tolerance to choose.  Figures are printed before they are asserted."""
import warnings

import numpy as np
import pytest
import torch

import sdflabel_amd
from sdflabel_amd import frame as FR
from sdflabel_amd.pipelines import refinement as rtools
from tests import _ingest_ref as R
from tests._util import ASSET, gold

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def z():
    return gold("g19_frame_ingest.npz")


@pytest.fixture(scope="module")
def dec32():
    return sdflabel_amd.setup_dsdf(ASSET + ".pt", precision=torch.float32)[0].to(DEV)


@pytest.fixture(scope="module")
def dec16():
    return sdflabel_amd.setup_dsdf(ASSET + ".pt", precision=torch.float16)[0].to(DEV)


def count_syncs(fn):
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            out = fn()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    return sum("synchroniz" in str(x.message).lower() for x in w), out


def cloud(z, i):
    if "dm%d_lidar" % i in z.files:
        return z["dm%d_lidar" % i]
    return np.ascontiguousarray(z["dm0_lidar"][z["dm%d_perm_of_dm0" % i]])


def same_bits(t, ref):
    a = t.detach().cpu().numpy()
    return a.dtype == ref.dtype and a.shape == ref.shape and a.tobytes() == ref.tobytes()


# ---- depth map ---------------------------------------------------------------------------------------------------------------------------

def test_depth_map_is_bit_equal_to_the_reference(z):
    for i in range(int(z["dm_n"])):
        lidar, K = cloud(z, i), z["dm%d_K" % i]
        w, h = z["dm%d_wh" % i].tolist()
        syncs, (depth, info) = count_syncs(lambda: FR.depth_map(lidar, K, w, h, return_info=True))
        counts = info["counts"].tolist()
        d = depth.cpu().numpy()
        print("cloud %d (%s points, %s K): %d of %d points on a pixel, %d dropped, %d depth values differ, %d winners differ, %d synchronisations" %
              (i, lidar.dtype, K.dtype, counts[0], len(lidar), counts[1], int((d != z["dm%d_depth" % i]).sum()),
               int((info["winner"].cpu().numpy() != z["dm%d_winner" % i]).sum()), syncs))
        assert depth.is_cuda and same_bits(depth, z["dm%d_depth" % i])
        assert same_bits(info["winner"], z["dm%d_winner" % i])
        assert counts == [int(z["dm%d_kept" % i]), 0]
        assert syncs == 0
        again, info2 = FR.depth_map(torch.from_numpy(lidar).to(DEV), torch.from_numpy(K), w, h, return_info=True)      # device input, second run
        assert torch.equal(again, depth) and torch.equal(info2["winner"], info["winner"]) and torch.equal(info2["counts"], info["counts"])
        assert np.array_equal(rtools.compute_depth_map(lidar, K, w, h), z["dm%d_depth" % i])
    d0, d2 = FR.depth_map(cloud(z, 0), z["dm0_K"], 96, 32), FR.depth_map(cloud(z, 2), z["dm2_K"], 96, 32)
    assert not torch.equal(d0, d2) and torch.equal(d0 != 0, d2 != 0)              # the shuffled cloud: other winners on the same pixels


def test_depth_map_at_kitti_scale_equals_the_restatement():
    rng = np.random.default_rng(77)
    K = np.array([[721.5377, 0, 609.5593], [0, 721.5377, 172.854], [0, 0, 1]], np.float64)
    w, h, n = 1242, 375, 26000
    zc = rng.uniform(3.0, 70.0, n)
    u, v = rng.uniform(-150, w + 150, n), rng.uniform(-60, h + 60, n)
    v[::3] = rng.uniform(150, 260, len(v[::3]))                                   # the lidar's dense band: several points per pixel
    u[::3] = np.round(rng.uniform(300, 700, len(u[::3]))) + 0.5
    v[::3] = np.round(v[::3] / 8) * 8 + 0.5
    lidar = np.stack([(u - K[0, 2]) / K[0, 0] * zc, (v - K[1, 2]) / K[1, 1] * zc, zc], 1)
    depth, winner, kept, dropped = R.depth_map(lidar, K, w, h)
    got, info = FR.depth_map(lidar, K, w, h, return_info=True)
    counts = info["counts"].tolist()
    print("KITTI scale: %d points, %d on a pixel (restatement %d), %d pixels set, %d dropped; %d depth values and %d winners differ" %
          (n, counts[0], kept, int((winner >= 0).sum()), counts[1], int((got.cpu().numpy() != depth).sum()),
           int((info["winner"].cpu().numpy() != winner).sum())))
    assert 18000 <= kept <= 24000 and kept > 1.05 * (winner >= 0).sum()
    assert same_bits(got, depth) and same_bits(info["winner"], winner) and counts == [kept, dropped] and dropped == 0
    got32 = FR.depth_map(lidar.astype(np.float32), K, w, h)                        # a float32 cloud is widened, not recomputed in float32
    assert same_bits(got32, R.depth_map(lidar.astype(np.float32), K, w, h)[0])
    empty, info = FR.depth_map(np.zeros((0, 3)), K, 64, 48, return_info=True)
    assert not empty.any() and (info["winner"] == -1).all() and info["counts"].tolist() == [0, 0]


# ---- box matching ------------------------------------------------------------------------------------------------------------------------

def test_match_boxes_equals_the_reference(z):
    for i in range(int(z["mb_n"])):
        p = "mb%d_" % i
        syncs, (best, iou, keep) = count_syncs(lambda: FR.match_boxes(z[p + "anno"], z[p + "det"]))
        print("match case %d: best %s keep %s, %d iou values differ in bits, %d synchronisations" %
              (i, best.tolist(), keep.tolist(), int((iou.cpu().numpy() != z[p + "iou"]).sum()), syncs))
        assert best.dtype == torch.int32 and best.tolist() == z[p + "best"].tolist()
        assert keep.dtype == torch.bool and keep.tolist() == z[p + "keep"].tolist()
        assert same_bits(iou, z[p + "iou"]) and syncs == 0
        b2, i2, k2 = FR.match_boxes(torch.from_numpy(z[p + "anno"]).to(DEV), torch.from_numpy(z[p + "det"]).to(DEV))
        assert torch.equal(b2, best) and torch.equal(i2, iou) and torch.equal(k2, keep)
    best, _, _ = FR.match_boxes(z["mb2_anno"], z["mb2_det"])
    assert best[0].item() == 1 and np.array_equal(z["mb2_det"][1], z["mb2_det"][3])       # the tie returns the first
    best, iou, keep = FR.match_boxes(z["mb0_anno"], np.zeros((0, 4)))
    assert best.tolist() == [-1] * len(z["mb0_anno"]) and not keep.any() and not iou.any()


# ---- CSS input ---------------------------------------------------------------------------------------------------------------------------

def _css_case(z, i):
    mask = z["css%d_mask" % i] if "css%d_mask" % i in z.files else None
    ref = z["css%d_u8" % i]
    return z["css%d_box" % i].tolist(), mask, ref, z["css_orig_lut"][ref.transpose(2, 0, 1)], np.stack([z["css_norm_lut"][c][ref[:, :, c]] for c in range(3)])


def test_css_inputs_are_byte_equal_to_pil_and_bit_equal_to_torch(z):
    n = int(z["css_n"])
    image = z["css_image"]
    boxes, masks = [], []
    for i in range(n):
        box, mask, u8_ref, orig_ref, im_ref = _css_case(z, i)
        boxes.append(box), masks.append(mask)
        syncs, (im, orig, u8) = count_syncs(lambda: FR.css_inputs_many(image, [box], masks=None if mask is None else [mask], orig=True, return_u8=True))
        print("css case %d box %s%s: %d bytes differ after the resample, %d / %d floats differ in im_orig / im, %d synchronisations" %
              (i, box, " masked" if mask is not None else "", int((u8[0].cpu().numpy() != u8_ref).sum()),
               int((orig[0].cpu().numpy() != orig_ref).sum()), int((im[0].cpu().numpy() != im_ref).sum()), syncs))
        assert same_bits(u8[0], u8_ref)
        assert np.array_equal(np.round(orig[0].cpu().numpy() * 255).astype(np.uint8).transpose(1, 2, 0), u8_ref)
        assert same_bits(orig[0], orig_ref) and same_bits(im[0], im_ref) and syncs == 0
    # all of them in one call, masks mixed with None, the image already on the device
    im, orig = FR.css_inputs_many(torch.from_numpy(image).to(DEV), boxes, masks=masks, orig=True)
    assert im.shape == orig.shape == (n, 3, 128, 128)
    for i in range(n):
        _, _, _, orig_ref, im_ref = _css_case(z, i)
        assert same_bits(orig[i], orig_ref) and same_bits(im[i], im_ref), i
    only = FR.css_inputs_many(image, boxes, masks=masks)
    assert torch.equal(only, im)


def test_css_inputs_of_a_frame_equal_single_calls_and_the_drop_in(z):
    rng = np.random.default_rng(8)
    image = torch.from_numpy(z["css_image"]).to(DEV)
    H, W = image.shape[:2]
    boxes, masks = [], []
    for i in range(16):
        l, t = int(rng.integers(0, W - 2)), int(rng.integers(0, H - 2))
        r, b = int(rng.integers(l + 1, W + 1)), int(rng.integers(t + 1, H + 1))
        boxes.append([l, t, r, b])
        masks.append(torch.from_numpy(rng.random((b - t, r - l)) < 0.6) if i % 3 == 0 else None)
    syncs, (im, orig) = count_syncs(lambda: FR.css_inputs_many(image, boxes, masks=masks, orig=True))
    print("16 boxes in one call: %d synchronisations" % syncs)
    assert syncs == 0
    for i in range(16):
        a, o = FR.css_inputs_many(image, [boxes[i]], masks=[masks[i]], orig=True)
        assert torch.equal(a[0], im[i]) and torch.equal(o[0], orig[i]), i
        l, t, r, b = boxes[i]
        crop = z["css_image"][t:b, l:r].copy()
        if masks[i] is not None:
            crop *= masks[i].numpy()[:, :, None].astype(np.float32)
        keep = crop.copy()
        one, one_orig = rtools.transform_bgr_crop(crop, orig=True)               # the drop-in: CPU tensors, (3, 128, 128)
        assert not one.is_cuda and one.shape == (3, 128, 128) and torch.equal(one, im[i].cpu()) and torch.equal(one_orig, orig[i].cpu())
        assert torch.equal(rtools.transform_bgr_crop(crop), one) and np.array_equal(crop, keep)
        ref_im, ref_orig, _ = R.css_input(z["css_image"][t:b, l:r], None if masks[i] is None else masks[i].numpy())
        assert same_bits(im[i], ref_im) and same_bits(orig[i], ref_orig), i
    with pytest.raises(ValueError):
        FR.css_inputs_many(image, [[0, 0, W + 1, 10]])
    with pytest.raises(ValueError):
        FR.css_inputs_many(image, [[5, 5, 5, 10]])


def test_css_input_of_a_kitti_sized_crop_equals_pil():
    from PIL import Image
    rng = np.random.default_rng(9)
    u = rng.integers(0, 256, (375, 1242, 3), dtype=np.uint8)
    image = (u.astype(np.float32) / np.float32(255.0)).astype(np.float32)
    for box in ([0, 0, 1242, 375], [3, 1, 1000, 129], [600, 100, 601, 101]):
        l, t, r, b = box
        rgb = np.ascontiguousarray((image[t:b, l:r] * 255).astype(np.uint8)[:, :, ::-1])
        ref = np.asarray(Image.fromarray(rgb).resize((128, 128), Image.BILINEAR))
        _, u8 = FR.css_inputs_many(image, [box], return_u8=True)
        print("box %s: %d bytes differ from PIL" % (box, int((u8[0].cpu().numpy() != ref).sum())))
        assert same_bits(u8[0], ref)


# ---- the sample --------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def sample(dec32):
    from sdflabel_amd.fixtures import synthetic_sample
    return synthetic_sample(dec32, 40, 32, DEV)


def _by_hand(sample, lidar, net, dec, grid, iters, weights, boxes, masks=None, css_batch=None, seed=7):
    """the parent's path: crops sliced in numpy on the host, css_net on css_inputs_many's output, then refine_frame"""
    from sdflabel_amd.pipelines.frame import refine_frame
    image = sample["image"]
    H, W = image.shape[:2]
    depth = FR.depth_map(lidar, sample["orig_cam"], W, H).cpu().numpy()
    css_in = FR.css_inputs_many(image, boxes, masks=masks)
    uvw, lat = [], []
    step = len(boxes) if not css_batch else css_batch
    with torch.no_grad():
        for c0 in range(0, len(boxes), step):
            pred = net(css_in[c0:c0 + step])
            uvw.extend(pred["uvw_sm_masked"])
            lat.extend(pred["latent"])
    annotations = [{"bbox": [l, t, r, b], "color": image[t:b, l:r].copy(), "depth": depth[t:b, l:r].copy(), "nocs_pred": uvw[j] / 255.}
                   for j, (l, t, r, b) in enumerate(boxes)]
    latents = [x.to(grid.points.dtype) for x in lat]
    return refine_frame(annotations, dec, grid, latents, sample["orig_cam"], sample["world_to_cam"], iters, weights, seed=seed, return_stages=True)


def _same_frame(est, hand):
    assert est["name"] == hand["name"]
    for k in FR.NECESSARY_KEYS:
        assert est[k].dtype == hand[k].dtype and est[k].shape == hand[k].shape and est[k].tobytes() == hand[k].tobytes(), k


@pytest.mark.parametrize("css_batch", [None, 1])
def test_refine_sample_equals_the_host_sliced_composition_and_feeds_the_evaluator(sample, dec16, css_batch):
    from sdflabel_amd.fixtures import stand_in_css
    from sdflabel_amd.pipelines import detection_3d as D3
    from sdflabel_amd.pipelines import optimizer as OP
    from sdflabel_amd.pipelines.frame import refine_sample
    smp, lidar = sample
    net = stand_in_css().to(DEV)
    grid = sdflabel_amd.Grid3D(40, DEV)
    W8, iters = {"2d": 0.3, "3d": 0.5}, 10
    annos = rtools.get_annos("", smp)
    n = len(annos)
    boxes = [[int(v) for v in a["bbox"]] for a in annos]
    before = [a["bbox"].copy() for a in annos]
    OP.clear_refiner_cache()
    est, kept, frame_annos, st = refine_sample(smp, net, dec16, grid, iters, W8, lidar=lidar, css_batch=css_batch, seed=7, return_stages=True)
    print("refine_sample: image %s, %d lidar points, %d annotations, %d kept; lidar points per crop %s; NOCS points per crop %s" %
          (smp["image"].shape, len(lidar), n, len(kept), [int(x[0].shape[0]) for x in st["lidar"]], [int(x[0].shape[0]) for x in st["nocs_3d"]]))
    assert n >= 2 and len(kept) >= 1, "the synthetic sample should give some annotation a RANSAC pose"
    hand, hkept, hst = _by_hand(smp, lidar, net, dec16, grid, iters, W8, boxes, css_batch=css_batch)
    assert kept == hkept
    for i in range(n):
        assert torch.equal(st["lidar"][i][0], hst["lidar"][i][0]) and torch.equal(st["lidar"][i][1], hst["lidar"][i][1])
        assert torch.equal(st["nocs_3d"][i][0], hst["nocs_3d"][i][0])
    for a, b in zip(st["params"], hst["params"]):
        for k in ("yaw", "trans", "scale", "latent"):
            assert torch.equal(a[k], b[k]), k
    _same_frame(est, hand)
    assert all(np.array_equal(a["bbox"], b) for a, b in zip(annos, before))       # the caller's annotations are not modified
    # sample['depth'] in the lidar's place gives the same frame
    smp2 = dict(smp, depth=FR.depth_map(lidar, smp["orig_cam"], smp["image"].shape[1], smp["image"].shape[0]).cpu().numpy())
    est2, kept2, _ = refine_sample(smp2, net, dec16, grid, iters, W8, css_batch=css_batch, seed=7)
    assert kept2 == kept
    _same_frame(est2, est)
    # the evaluator takes both dicts as they are
    assert frame_annos["name"] == ["Car"] * n and frame_annos["bbox"].shape == (n, 4) and frame_annos["location"].shape == (n, 3)
    assert frame_annos["dimensions"].shape == (n, 3) and frame_annos["rotation_y"].shape == frame_annos["alpha"].shape == (n,)
    assert est["location"].shape == (len(kept), 3) and est["bbox"].shape == (len(kept), 4) and np.isfinite(est["location"]).all()
    from tests import _eval_golden as GD
    g17 = GD.load()
    ev = D3.Detection3DEvaluator(D3.clean_kitti_data, GD.id_to_name(g17), g17["overlap_thresholds"], g17["dist_thresholds"], compute_nuscenes=False,
                                 coordinate_frame=D3.CoordinateFrame.CAMERA)
    text, result = ev.evaluate_detection_3d([frame_annos], [est], ["Car"], difficulties=[0])
    print(text)
    assert isinstance(text, str) and isinstance(result, dict) and len(result) > 0


def test_refine_sample_with_detector_boxes_and_masks(sample, dec16):
    from sdflabel_amd.fixtures import stand_in_css
    from sdflabel_amd.pipelines import optimizer as OP
    from sdflabel_amd.pipelines.frame import refine_sample
    smp, lidar = sample
    net = stand_in_css().to(DEV)
    grid = sdflabel_amd.Grid3D(40, DEV)
    W8, iters = {"2d": 0.3, "3d": 0.5}, 10
    annos = rtools.get_annos("", smp)
    n = len(annos)
    H, W = smp["image"].shape[:2]
    rng = np.random.default_rng(3)
    det = np.stack([a["bbox"] + rng.uniform(0.0, 2.9, 4) * [1, 1, -1, -1] for a in annos]).astype(np.float32)
    lost = 1
    w_lost = det[lost, 2] - det[lost, 0]
    det[lost, [0, 2]] = det[lost, [0, 2]] + np.float32(0.45 * w_lost) * (1 if det[lost, 2] + 0.45 * w_lost < W else -1)    # IoU about 0.38
    det = np.concatenate([[[1.0, 1.0, 6.0, 5.0]], det]).astype(np.float32)                                              # detector box 0 matches nothing
    tb = det.astype(np.int64)
    masks = []
    for l, t, r, b in tb:
        m = torch.ones((b - t, r - l), dtype=torch.bool)
        m[: (b - t) // 6] = False
        masks.append(m)
    labels = {"bboxes": torch.from_numpy(det), "masks": masks}
    ref_best, ref_iou, ref_keep = R.match_boxes(np.stack([a["bbox"] for a in annos]), det)
    assert not ref_keep[lost] and ref_keep.sum() == n - 1 and (np.abs(ref_iou - 0.5) > 1e-3).all()
    OP.clear_refiner_cache()
    est, kept, frame_annos, st = refine_sample(smp, net, dec16, grid, iters, W8, label_type="maskrcnn", maskrcnn_labels=labels, lidar=lidar, seed=7,
                                               return_stages=True)
    print("maskrcnn: iou %s, best %s, kept %s of %d" % (np.round(ref_iou, 3).tolist(), ref_best.tolist(), kept, n))
    assert st["match"]["best"].tolist() == ref_best.tolist() and st["match"]["keep"].tolist() == ref_keep.tolist()
    assert lost not in kept and len(kept) >= 1 and all(0 <= i < n for i in kept)
    assert frame_annos["bbox"].shape == (n, 4) and np.array_equal(frame_annos["bbox"], np.stack([a["bbox"] for a in annos]))    # all of them, original boxes
    live = [i for i in range(n) if ref_keep[i]]
    boxes = [tb[ref_best[i]].tolist() for i in live]
    assert [st["boxes"][i] for i in live] == boxes and st["boxes"][lost] is None
    assert np.array_equal(est["bbox"], np.asarray([boxes[live.index(i)] for i in kept]))                                # the label carries the matched box
    hand, hkept, hst = _by_hand(smp, lidar, net, dec16, grid, iters, W8, boxes, masks=[masks[ref_best[i]] for i in live])
    assert [live[j] for j in hkept] == kept
    _same_frame(est, hand)
    # the mask goes into the CSS input only: the lidar crop's colours are those of the unmasked image
    masked = FR.css_inputs_many(smp["image"], boxes, masks=[masks[ref_best[i]] for i in live])
    plain = FR.css_inputs_many(smp["image"], boxes)
    assert torch.equal(st["css_input"], masked) and not torch.equal(masked, plain)
    for j in range(len(live)):
        assert torch.equal(st["lidar"][j][1], hst["lidar"][j][1])
    # 'rcnn' uses the boxes without the masks
    est_r, kept_r, _, st_r = refine_sample(smp, net, dec16, grid, iters, W8, label_type="rcnn", maskrcnn_labels=labels, lidar=lidar, seed=7,
                                           return_stages=True)
    assert torch.equal(st_r["css_input"], plain) and lost not in kept_r


def test_refine_sample_adds_at_most_the_read_of_the_match(sample, dec16):
    from sdflabel_amd.fixtures import stand_in_css
    from sdflabel_amd.pipelines.frame import refine_frame, refine_sample
    smp, lidar = sample
    net = stand_in_css().to(DEV)
    grid = sdflabel_amd.Grid3D(40, DEV)
    W8, iters = {"2d": 0.3, "3d": 0.5}, 10
    annos = rtools.get_annos("", smp)
    det = np.stack([a["bbox"] for a in annos]).astype(np.float32)
    labels = {"bboxes": torch.from_numpy(det), "masks": [torch.ones((int(b - t), int(r - l))) for l, t, r, b in det]}
    run_gt = lambda: refine_sample(smp, net, dec16, grid, iters, W8, lidar=lidar, seed=7, return_stages=True)                # noqa: E731
    run_mr = lambda: refine_sample(smp, net, dec16, grid, iters, W8, label_type="maskrcnn", maskrcnn_labels=labels, lidar=lidar, seed=7)   # noqa: E731
    _, _, _, st = run_gt()                                                        # warm: refiners built, graphs captured
    run_mr()
    image, depth = torch.from_numpy(smp["image"]).to(DEV), st["depth"]
    annotations = [{"bbox": [l, t, r, b], "color": image[t:b, l:r], "depth": depth[t:b, l:r], "nocs_pred": st["nocs_pred"][i]}
                   for i, (l, t, r, b) in enumerate(st["boxes"])]
    run_rf = lambda: refine_frame(annotations, dec16, grid, st["latents"], smp["orig_cam"], smp["world_to_cam"], iters, W8, seed=7)    # noqa: E731
    run_rf()
    s_rf, s_gt, s_mr = count_syncs(run_rf)[0], count_syncs(run_gt)[0], count_syncs(run_mr)[0]
    print("host synchronisations per call: refine_frame %d, refine_sample 'gt' %d, refine_sample 'maskrcnn' %d" % (s_rf, s_gt, s_mr))
    assert s_gt == s_rf and s_mr <= s_rf + 1
