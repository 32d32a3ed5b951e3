"""Golden G19 (tests/golden/g19_frame_ingest.npz): frame ingest -- the lidar depth map, the box matching, the CSS network's input.

Runs the reference's own utils.refinement functions (tools/_ref_import.py: read-only, cv2 / open3d / pyquaternion stubbed) on the CPU:
compute_depth_map, build_view_frustum, get_iou, get_annos and is_anno_easy / _moderate / _hard.  Only DATA is committed: clouds, boxes, one
small image and the recorded results.

cv2 is not installed here.  `project` (utils/refinement.py:470-472) calls cv2.projectPoints with zero rotation, zero translation and no
distortion, `unproject` (:475-477) cv2.undistortPoints without distortion and cv2.convertPointsToHomogeneous; this generator supplies the
three as float64 pinholes (fx x / z + cx; (u - cx) / fx; a column of ones).  The file records the fact (`_cv2_is_float64_pinhole`).

torchvision is not installed either, so the CSS-input cases RESTATE transform_bgr_crop (utils/refinement.py:60-84) and do not call it: the
crop is turned into uint8 and RGB with numpy as :72 does, resized with PIL itself -- Image.fromarray(...).resize((128, 128), Image.BILINEAR),
which is what transforms.Resize((128, 128)) calls for a PIL image --, and ToTensor / Normalize are torch float32 operations (x / 255, then
(x - mean) / std).  Because the float32 results depend only on the byte (and the channel), the file stores the resampled uint8 images and
the two torch-made tables orig_lut[256] and norm_lut[3][256]; the expected float images are the tables indexed by the bytes.

Contents
  dm*      lidar clouds of 2 000 points in a KITTI-like camera at a small w x h (several points per pixel, points outside each of the four
           planes, a float32 cloud, a float32 camera matrix) through compute_depth_map; per cloud also the frustum of build_view_frustum and
           the winner image -- the loop of :103-104 run again with the reference's project, recording the point's index instead of its z.
           dm2 is dm0 shuffled (stored as the permutation): its depth image must differ from dm0's.
  mb*      annotation and detector boxes through the loop of refine_css.py:101-114 around the reference's get_iou: the whole IoU matrix,
           np.argmax, the 0.5 test; disjoint and touching boxes; mb2 holds a detector box twice on purpose, to pin "the first maximum".
  an_*     a synthetic sample's annotations through get_annos for 'hard', 'medium', '' and the three difficulty predicates.
  css*     crops of one 140 x 310 frame (smaller than, equal to and larger than 128 in each direction, one 1 pixel wide), with and without
           a mask.

Conditions enforced by REFUSING (they are not measurements): a cloud's points are drawn until none of them violates the first two, then the
case is checked as a whole, the reference alone deciding what it keeps:
  - no kept point's float64 pixel coordinate lies within 1e-3 of an integer;
  - no |plane . p| is below 1e-6 |p|;
  - no IoU lies within 1e-6 of 0.5;
  - no two detector boxes tie for an annotation's maximum, except in mb2.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _ref_import  # noqa: E402

_ref_import.setup()
sys.modules["pyquaternion"].Quaternion = object  # `from pyquaternion import Quaternion` (utils/refinement.py:6)

import numpy as np  # noqa: E402
import torch  # noqa: E402
from PIL import Image  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "..", "tests", "golden", "g19_frame_ingest.npz")


def project64(p3d, rvec, tvec, K, dist):
    p = np.asarray(p3d, np.float64).reshape(-1, 3)
    K = np.asarray(K, np.float64)
    uv = np.stack([K[0, 0] * (p[:, 0] / p[:, 2]) + K[0, 2], K[1, 1] * (p[:, 1] / p[:, 2]) + K[1, 2]], 1)
    return uv[:, None, :], None


def undistort64(p2d, K, dist):
    p = np.asarray(p2d, np.float64).reshape(-1, 2)
    K = np.asarray(K, np.float64)
    return np.stack([(p[:, 0] - K[0, 2]) / K[0, 0], (p[:, 1] - K[1, 2]) / K[1, 1]], 1)[:, None, :]


def homogeneous(p):
    p = np.asarray(p)
    return np.concatenate([p, np.ones(p.shape[:-1] + (1,), p.dtype)], -1)


cv2 = sys.modules["cv2"]
cv2.projectPoints, cv2.undistortPoints, cv2.convertPointsToHomogeneous = project64, undistort64, homogeneous

import utils.refinement as rtools  # noqa: E402

NEAR_PIXEL, NEAR_PLANE, NEAR_IOU = 1e-3, 1e-6, 1e-6


def cloud_conditions(lidar, K, w, h):
    """(per point: violates a condition, inside the frustum) judged from the reference's frustum and the float64 pinhole"""
    fr = rtools.build_view_frustum(K, 0, 0, w, h).astype(np.float64)
    p = lidar.astype(np.float64)
    dots = fr @ p.T
    near_plane = (np.abs(dots) < NEAR_PLANE * np.linalg.norm(p, axis=1)[None]).any(0)
    inside = np.logical_and.reduce(dots > 0, axis=0)
    uv = project64(p, None, None, K, None)[0][:, 0]
    near_pix = (np.abs(uv - np.round(uv)) < NEAR_PIXEL).any(1) & inside
    return near_plane | near_pix, inside, dots


def draw_cloud(rng, n, K, w, h, dtype):
    out = np.zeros((0, 3), dtype)
    while out.shape[0] < n:
        z = rng.uniform(4.0, 40.0, n)
        # pixel targets a little beyond the image on every side, so that points fall outside each plane; a third of the points crowd a corner
        u = rng.uniform(-0.12 * w, 1.12 * w, n)
        v = rng.uniform(-0.2 * h, 1.2 * h, n)
        crowd = rng.random(n) < 0.33
        u[crowd], v[crowd] = rng.uniform(0.1 * w, 0.3 * w, int(crowd.sum())), rng.uniform(0.2 * h, 0.6 * h, int(crowd.sum()))
        Kd = np.asarray(K, np.float64)
        pts = np.stack([(u - Kd[0, 2]) / Kd[0, 0] * z, (v - Kd[1, 2]) / Kd[1, 1] * z, z], 1).astype(dtype)
        bad, _, _ = cloud_conditions(pts, K, w, h)
        out = np.concatenate([out, pts[~bad]])
    return np.ascontiguousarray(out[:n])


def depth_case(arrs, tag, lidar, K, w, h):
    bad, inside, dots = cloud_conditions(lidar, K, w, h)
    assert not bad.any(), "refused: %s violates a condition" % tag
    outside = (dots <= 0)
    assert outside.any(1).all(), "refused: %s has no point outside some plane" % tag
    depth = rtools.compute_depth_map(lidar, K, w, h)                                   # the reference keeps the case on its own (no IndexError)
    frustum = rtools.build_view_frustum(K, 0, 0, w, h)
    winner = np.full((h, w), -1, np.int32)
    idx = np.nonzero(np.logical_and.reduce(frustum @ lidar.T > 0, axis=0))[0]
    for (x, y), i in zip(rtools.project(K, lidar[idx]).astype(np.int32), idx):        # the loop of :103-104 with the index in z's place
        winner[y, x] = i
    assert np.array_equal(idx, np.nonzero(inside)[0])
    assert np.array_equal(depth, np.where(winner >= 0, lidar[np.maximum(winner, 0), 2], 0).astype(np.float32))
    per_pixel = len(idx) / max(int((winner >= 0).sum()), 1)
    assert per_pixel > 1.3, "refused: %s has too few pixels with several points" % tag
    arrs[tag + "_lidar"], arrs[tag + "_K"], arrs[tag + "_wh"] = lidar, K, np.array([w, h])
    arrs[tag + "_depth"], arrs[tag + "_winner"], arrs[tag + "_frustum"], arrs[tag + "_kept"] = depth, winner, frustum, len(idx)
    print(tag, lidar.dtype, K.dtype, "%dx%d" % (w, h), "inside", len(idx), "of", len(lidar), "pixels set", int((winner >= 0).sum()),
          "points per set pixel %.2f" % per_pixel, "outside per plane", outside.sum(1).tolist())
    return depth


def depth_cases(arrs):
    rng = np.random.default_rng(19)
    K0 = np.array([[70.0, 0, 47.3], [0, 70.0, 15.7], [0, 0, 1]], np.float64)
    l0 = draw_cloud(rng, 2000, K0, 96, 32, np.float64)
    d0 = depth_case(arrs, "dm0", l0, K0, 96, 32)
    K1 = np.array([[58.5, 0, 41.2], [0, 59.25, 11.4], [0, 0, 1]], np.float64)
    depth_case(arrs, "dm1", draw_cloud(rng, 2000, K1, 80, 24, np.float32), K1, 80, 24)
    perm = rng.permutation(len(l0))
    d2 = depth_case(arrs, "dm2", np.ascontiguousarray(l0[perm]), K0, 96, 32)
    del arrs["dm2_lidar"]
    arrs["dm2_perm_of_dm0"] = perm.astype(np.int32)
    assert not np.array_equal(d0, d2), "the shuffled cloud must give another depth image"
    assert np.array_equal(d0 != 0, d2 != 0)
    print("dm2: %d pixels differ from dm0" % int((d0 != d2).sum()))
    K3 = np.array([[72.15377, 0, 60.95593], [0, 72.15377, 17.2854], [0, 0, 1]], np.float32)     # a float32 camera matrix, as a loader may give
    depth_case(arrs, "dm3", draw_cloud(rng, 2000, K3, 124, 37, np.float64), K3, 124, 37)
    arrs["dm_n"] = 4


def match_case(arrs, tag, anno, det, tie_ok):
    A, M = len(anno), len(det)
    mat = np.zeros((A, M))
    best, top = np.zeros(A, np.int32), np.zeros(A)
    for i in range(A):
        iou = []
        for bbox in det:                                                                # refine_css.py:102-106
            iou.append(rtools.get_iou(bbox, anno[i]))
        best[i] = np.argmax(iou)
        top[i] = iou[best[i]]
        mat[i] = iou
        ties = int((np.asarray(iou) == top[i]).sum())
        assert tie_ok or ties == 1 or top[i] == 0.0, "refused: %s annotation %d has tied maxima" % (tag, i)
    assert (np.abs(mat - 0.5) >= NEAR_IOU).all(), "refused: %s has an IoU near 0.5" % tag
    arrs[tag + "_anno"], arrs[tag + "_det"] = np.asarray(anno, np.float64), np.asarray(det, np.float64)
    arrs[tag + "_matrix"], arrs[tag + "_best"], arrs[tag + "_iou"], arrs[tag + "_keep"] = mat, best, top, ~(top < 0.5)
    print(tag, "best", best.tolist(), "iou", np.round(top, 4).tolist(), "keep", (~(top < 0.5)).tolist())
    return best, top


def match_cases(arrs):
    rng = np.random.default_rng(191)
    # mb0: integer annotation boxes, float detector boxes near some of them, far from others
    xy = rng.integers(0, 900, (7, 2))
    anno = np.concatenate([xy, xy + rng.integers(30, 300, (7, 2))], 1).astype(np.float64)
    det = []
    for i, a in enumerate(anno):
        jit = rng.uniform(-1, 1, 4) * np.tile(a[2:] - a[:2], 2) * (0.04 if i % 2 == 0 else 0.3)
        det.append(a + jit)
    det += [np.array([2000.0, 2000.0, 2100.0, 2050.0]), anno[1] + np.array([5.0, 3.0, -8.0, -2.0])]
    det = np.stack(det)[rng.permutation(len(det))]
    anno = np.concatenate([anno, [[3000.0, 10.0, 3100.0, 90.0]]])                        # overlaps nothing: every IoU is 0.0, argmax is 0
    best, top = match_case(arrs, "mb0", anno, det, False)
    assert (top >= 0.5).any() and (top < 0.5).any() and (top == 0.0).any()
    # mb1: touching boxes (width == 0 is not "< 0": an IoU of 0 through the division) and contained boxes
    anno = np.array([[100.0, 100, 200, 200], [0, 0, 50, 50], [300, 300, 420, 380]])
    det = np.array([[200.0, 100, 300, 200], [110, 110, 190, 190], [0, 50, 50, 100], [10, 10, 40, 45], [290, 310, 430, 370], [1000, 1000, 1001, 1001]])
    match_case(arrs, "mb1", anno, det, False)
    # mb2: the tie on purpose -- detector boxes 1 and 3 are the same box
    anno = np.array([[50.0, 60, 250, 180], [400, 100, 640, 260]])
    det = np.array([[300.0, 300, 350, 350], [55, 62, 245, 185], [410, 90, 650, 255], [55, 62, 245, 185], [60, 70, 150, 120]])
    best, top = match_case(arrs, "mb2", anno, det, True)
    assert best[0] == 1 and arrs["mb2_matrix"][0, 1] == arrs["mb2_matrix"][0, 3] == top[0]
    arrs["mb_n"] = 3


def anno_cases(arrs):
    rng = np.random.default_rng(192)
    # (occluded, truncated, box height): each predicate's three limits from both sides, the limits themselves included
    rows = [(0, 0.0, 60.0), (0, 0.15, 40.0), (0, 0.16, 60.0), (1, 0.0, 60.0), (0, 0.0, 39.5), (1, 0.30, 25.0), (2, 0.1, 50.0), (1, 0.31, 50.0),
            (1, 0.2, 24.5), (2, 0.5, 25.0), (3, 0.0, 70.0), (2, 0.51, 70.0), (0, 0.1, 45.0), (2, 0.4, 30.0)]
    n = len(rows)
    tab = np.zeros((n, 8))                                                            # bbox[4], occluded, truncated, depth z, difficulty list
    sample = {"annos": {"easy": [], "medium": [], "hard": []}}
    for i, (occ, trunc, hgt) in enumerate(rows):
        t = rng.uniform(100, 200)
        anno = {"bbox": np.array([rng.uniform(0, 900), t, rng.uniform(950, 1200), t + hgt]), "occluded": occ, "truncated": trunc,
                "location": np.array([rng.uniform(-8, 8), 1.5, [12.0, 30.0, 7.5, 12.0][i % 4] + (i // 8)]), "id": i}
        lst = int(rng.integers(0, 3))
        sample["annos"][("easy", "medium", "hard")[lst]].append(anno)
        tab[i] = list(anno["bbox"]) + [anno["occluded"], anno["truncated"], anno["location"][2], lst]
        arrs.setdefault("an_easy", []).append(rtools.is_anno_easy(anno))
        arrs.setdefault("an_moderate", []).append(rtools.is_anno_moderate(anno))
        arrs.setdefault("an_hard", []).append(rtools.is_anno_hard(anno))
    arrs["an_table"] = tab
    for diff in ("hard", "medium", ""):
        arrs["an_order_" + (diff or "default")] = np.array([a["id"] for a in rtools.get_annos(diff, sample)], np.int32)
    for k in ("an_easy", "an_moderate", "an_hard"):
        assert 0 < sum(arrs[k]) < n
    print("annos", {k: arrs[k].tolist() for k in arrs if k.startswith("an_order")})


def css_cases(arrs):
    rng = np.random.default_rng(193)
    H, W = 140, 310
    image = (rng.integers(0, 256, (H, W, 3)).astype(np.float32) / np.float32(255.0)).astype(np.float32)     # what a loader's uint8 / 255 gives
    image[60:100, 200:260] = rng.random((40, 60, 3)).astype(np.float32)                                      # and arbitrary values
    image[0, 0], image[1, 1] = 1.0, 0.0
    arrs["css_image"] = image
    boxes = [(10, 5, 101, 42), (0, 0, 128, 128), (5, 0, 305, 140), (7, 3, 8, 139), (100, 20, 300, 60), (30, 5, 158, 135), (50, 50, 57, 55),
             (190, 50, 270, 110)]
    masked = [False, True, False, True, False, False, True, True]
    mean = torch.as_tensor([0.485, 0.456, 0.406], dtype=torch.float32)
    std = torch.as_tensor([0.229, 0.224, 0.225], dtype=torch.float32)
    byte = torch.arange(256, dtype=torch.uint8)
    orig_lut = byte.to(torch.float32).div(255)                                             # ToTensor
    norm_lut = (orig_lut[None, :].expand(3, 256).clone().sub_(mean[:, None]).div_(std[:, None]))          # Normalize
    arrs["css_orig_lut"], arrs["css_norm_lut"] = orig_lut.numpy(), norm_lut.numpy()
    sizes = set()
    for i, ((l, t, r, b), m) in enumerate(zip(boxes, masked)):
        crop = image[t:b, l:r].copy()
        mask = None
        if m:
            mask = rng.random((b - t, r - l)) < 0.7
            crop *= torch.from_numpy(mask).unsqueeze(-1).float().expand_as(torch.tensor(crop)).numpy()       # refine_css.py:135
        rgb = np.ascontiguousarray((crop * 255).astype(np.uint8)[:, :, ::-1])                                  # :72 (cv2.cvtColor BGR2RGB)
        u8 = np.asarray(Image.fromarray(rgb).resize((128, 128), Image.BILINEAR))
        # the tables are exactly the torch pipeline on this image
        ten = torch.from_numpy(u8.copy()).permute(2, 0, 1).contiguous().to(torch.float32).div(255)
        assert np.array_equal(ten.numpy(), arrs["css_orig_lut"][u8.transpose(2, 0, 1)])
        nrm = ten.clone().sub_(mean[:, None, None]).div_(std[:, None, None])
        assert np.array_equal(nrm.numpy(), np.stack([arrs["css_norm_lut"][c][u8[:, :, c]] for c in range(3)]))
        p = "css%d_" % i
        arrs[p + "box"], arrs[p + "u8"] = np.array([l, t, r, b]), u8
        if m:
            arrs[p + "mask"] = mask
        for s in (b - t, r - l):
            sizes.add(-1 if s < 128 else (0 if s == 128 else 1))
        print("css", i, (b - t, r - l), "masked" if m else "")
    assert sizes == {-1, 0, 1} and any(r - l == 1 for l, t, r, b in boxes)
    arrs["css_n"] = len(boxes)
    arrs["_pil_version"] = str(Image.__version__)


def main():
    arrs = {"_cv2_is_float64_pinhole": True, "_torch_version": str(torch.__version__), "_numpy_version": str(np.__version__)}
    depth_cases(arrs)
    match_cases(arrs)
    anno_cases(arrs)
    css_cases(arrs)
    np.savez_compressed(OUT, **{k: np.asarray(v) for k, v in arrs.items()})
    print("wrote", OUT, "%.1f KB" % (os.path.getsize(OUT) / 1024))


if __name__ == "__main__":
    main()
