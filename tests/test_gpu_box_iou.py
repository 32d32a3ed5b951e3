"""Box overlaps of the evaluator on the device (csrc/box_iou.hip): parity with golden G16 (recorded from the reference's rotate_iou.py),
analytic cases, the 16-point polygon, the fused 3-D launch, grouped (per-frame) mode, empty inputs, and the evaluator's sharded BEV / 3-D
flow run on the compat module."""
import math
import sys

import numpy as np
import pytest
import torch

from sdflabel_amd import box_iou as B
from tests.test_box_iou_cpu import G16, COMPAT, d3_np, rotate_iou_np

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g16():
    return np.load(G16)


@pytest.fixture(scope="module")
def R():
    """the compat module pipelines.rotate_iou (imported from the compat directory, as INTEGRATION.md sets the path up)"""
    sys.path.insert(0, COMPAT)
    try:
        import pipelines.rotate_iou as mod
    finally:
        sys.path.remove(COMPAT)
        sys.modules.pop("pipelines.rotate_iou", None)
        sys.modules.pop("pipelines", None)
    return mod


def _np(t):
    return t.cpu().numpy()


def test_rotate_iou_matches_g16(g16):
    crit = [int(c) for c in g16["criteria"]]
    diff_bits, total = 0, 0
    for name in g16["bev_cases"]:
        p = "bev_%s_" % name
        d = g16[p + "defined"].astype(bool)
        for ci, c in enumerate(crit):
            got = _np(B.rotate_iou(g16[p + "boxes"], g16[p + "qboxes"], c))
            ref = g16[p + "iou"][ci]
            assert got.dtype == np.float32 and got.shape == ref.shape
            g, r = got[d], ref[d]
            assert np.array_equal(np.isnan(g), np.isnan(r)), (name, c)
            ok = ~np.isnan(r)
            if c == 2:
                assert np.all(np.abs(g[ok] - r[ok]) <= 1e-6 * np.maximum(np.abs(r[ok]), 1.0)), (name, c)
            else:
                assert np.abs(g[ok] - r[ok]).max(initial=0) <= 1e-6, (name, c)
            diff_bits += int((g[ok].view(np.uint32) != r[ok].view(np.uint32)).sum())
            total += int(ok.sum())
    print("rotate_iou vs G16: %d of %d defined entries not bit-identical" % (diff_bits, total))


def test_box3d_and_image_iou_match_g16(g16):
    crit = [int(c) for c in g16["criteria"]]
    for name in g16["d3_cases"]:
        p = "d3_%s_" % name
        d = g16[p + "defined"].astype(bool)
        cam = bool(g16[p + "camera"])
        for ci, c in enumerate(crit):
            got = _np(B.box3d_iou(g16[p + "boxes"], g16[p + "qboxes"], c, camera_frame=cam))
            assert got.dtype == np.float32
            assert np.array_equal(got[d], g16[p + "iou"][ci][d]), (name, c)
    for ci, c in enumerate(crit):
        got = _np(B.image_box_iou(g16["img_boxes"], g16["img_qboxes"], c))
        assert got.dtype == np.float64 and np.array_equal(got, g16["img_iou"][ci]), c


def test_compat_functions_reproduce_g16(g16, R):
    crit = [int(c) for c in g16["criteria"]]
    for name in g16["bev_cases"]:
        p = "bev_%s_" % name
        d = g16[p + "defined"].astype(bool)
        for ci, c in enumerate(crit):
            got = R.rotate_iou_gpu_eval(g16[p + "boxes"].astype(np.float64), g16[p + "qboxes"], c)
            assert got.dtype == np.float32          # always float32, whatever went in (the reference's re-bound `boxes`)
            assert np.array_equal(got[d], g16[p + "iou"][ci][d], equal_nan=True), (name, c)
    for name in g16["d3_cases"]:
        p = "d3_%s_" % name
        d = g16[p + "defined"].astype(bool)
        rinc = np.nan_to_num(g16[p + "rinc"])
        for ci, c in enumerate(crit):
            r = rinc.copy()
            R.d3_box_overlap_kernel(g16[p + "boxes"], g16[p + "qboxes"], r, c, bool(g16[p + "camera"]))
            assert np.array_equal(r[d], g16[p + "iou"][ci][d]), (name, c)
    for ci, c in enumerate(crit):
        got = R.image_box_overlap(g16["img_boxes"], g16["img_qboxes"], c)
        assert got.dtype == np.float64 and np.array_equal(got, g16["img_iou"][ci])
    assert R.image_box_overlap(g16["img_boxes"].astype(np.float32), g16["img_qboxes"]).dtype == np.float32
    assert R.div_up(128, 64) == 2 and R.div_up(129, 64) == 3


def test_analytic_cases():
    sq = np.array([[0.0, 0.0, 1.0, 1.0, 0.0]], np.float32)
    turned = np.array([[0.0, 0.0, 1.0, 1.0, math.pi / 4]], np.float32)
    far = np.array([[10.0, 0.0, 1.0, 1.0, 0.3]], np.float32)
    big = np.array([[0.1, -0.2, 4.0, 2.0, 0.0]], np.float32)
    small = np.array([[0.1, -0.2, 1.0, 0.5, 0.0]], np.float32)
    box = np.array([[1.0, 2.0, 4.0, 1.5, 0.7]], np.float32)
    assert _np(B.rotate_iou(box, box))[0, 0] == pytest.approx(1.0, abs=1e-6)
    assert _np(B.rotate_iou(sq, far))[0, 0] == 0.0
    # the octagon of a unit square and itself turned by 45 degrees: area 2 (sqrt 2 - 1), IoU 1 / sqrt 2
    assert _np(B.rotate_iou(sq, turned, 2))[0, 0] == pytest.approx(2 * (math.sqrt(2) - 1), abs=1e-6)
    assert _np(B.rotate_iou(sq, turned))[0, 0] == pytest.approx(1 / math.sqrt(2), abs=1e-6)
    # a box inside a larger one: IoU = the area ratio
    assert _np(B.rotate_iou(big, small))[0, 0] == pytest.approx(0.5 / 8.0, abs=1e-6)
    # criterion 0 divides by the QUERY box's area, criterion 1 by the box's
    assert _np(B.rotate_iou(big, small, 0))[0, 0] == pytest.approx(1.0, abs=1e-6)
    assert _np(B.rotate_iou(big, small, 1))[0, 0] == pytest.approx(0.5 / 8.0, abs=1e-6)
    assert _np(B.rotate_iou(small, big, 0))[0, 0] == pytest.approx(0.5 / 8.0, abs=1e-6)
    ib = np.array([[0.0, 0.0, 10.0, 10.0]])
    iq = np.array([[5.0, 5.0, 15.0, 20.0]])
    assert _np(B.image_box_iou(ib, iq))[0, 0] == 25.0 / (100.0 + 150.0 - 25.0)
    assert _np(B.image_box_iou(ib, iq, 0))[0, 0] == 0.25 and _np(B.image_box_iou(ib, iq, 1))[0, 0] == 25.0 / 150.0
    assert _np(B.image_box_iou(ib, iq, 5))[0, 0] == 25.0


def test_sixteen_point_polygon_matches_the_restatement(g16):
    """pairs the reference leaves undefined (more than 8 candidate points) equal the in-file restatement with the same 16-point capacity"""
    seen = 0
    for name in g16["bev_cases"]:
        p = "bev_%s_" % name
        und = g16[p + "defined"] == 0
        if not und.any():
            continue
        ref, _ = rotate_iou_np(g16[p + "boxes"], g16[p + "qboxes"])
        for ci, c in enumerate((-1, 0, 1, 2)):
            got = _np(B.rotate_iou(g16[p + "boxes"], g16[p + "qboxes"], c))
            assert np.array_equal(got[und], ref[ci][und], equal_nan=True), (name, c)
        seen += int(und.sum())
    assert seen > 0


@pytest.mark.parametrize("camera", [True, False])
def test_fused_box3d_equals_bev_then_compat_d3(g16, R, camera):
    fr = "cam" if camera else "lidar"
    cols = [0, 2, 3, 5, 6] if camera else [0, 1, 3, 4, 6]
    for case in ("random", "cluster"):
        p = "d3_%s_%s_" % (fr, case)
        b, q = g16[p + "boxes"], g16[p + "qboxes"]
        for c in (-1, 0, 1, 2):
            fused = _np(B.box3d_iou(b, q, c, camera_frame=camera))
            rinc = _np(B.rotate_iou(b[:, cols], q[:, cols], 2))
            R.d3_box_overlap_kernel(b, q, rinc, c, camera)
            assert np.array_equal(fused.view(np.uint32), rinc.view(np.uint32)), (p, c)
            assert np.array_equal(rinc, d3_np(b, q, _np(B.rotate_iou(b[:, cols], q[:, cols], 2)), c, camera)), (p, c)


def _frames_of(boxes, qboxes, sizes):
    bl, ql, bo, qo = [], [], 0, 0
    for nb, nq in sizes:
        bl.append(boxes[bo:bo + nb])
        ql.append(qboxes[qo:qo + nq])
        bo, qo = bo + nb, qo + nq
    return bl, ql


def test_frames_equal_slices_of_the_dense_matrix(g16):
    sizes = [(3, 4), (0, 5), (6, 0), (0, 0), (15, 12), (1, 1), (70, 66)]
    nb, nq = sum(s[0] for s in sizes), sum(s[1] for s in sizes)
    b = np.concatenate([g16["bev_cluster_boxes"], g16["bev_random_boxes"]])[:nb]
    q = np.concatenate([g16["bev_cluster_qboxes"], g16["bev_random_qboxes"]])[:nq]
    b3 = np.concatenate([g16["d3_cam_cluster_boxes"], g16["d3_cam_random_boxes"]])[:nb]
    q3 = np.concatenate([g16["d3_cam_cluster_qboxes"], g16["d3_cam_random_qboxes"], g16["d3_lidar_cluster_qboxes"]])[:nq]
    ib = np.concatenate([g16["img_boxes"]] * 3)[:nb]
    iq = np.concatenate([g16["img_qboxes"]] * 3)[:nq]
    for fn, fr, x, y, kw in ((B.rotate_iou, B.rotate_iou_frames, b, q, {}), (B.box3d_iou, B.box3d_iou_frames, b3, q3, {"camera_frame": True}),
                             (B.box3d_iou, B.box3d_iou_frames, b3, q3, {"camera_frame": False}),
                             (B.image_box_iou, B.image_box_iou_frames, ib, iq, {})):
        for c in (-1, 0, 2):
            dense = _np(fn(x, y, c, **kw))
            blocks = fr(*_frames_of(x, y, sizes), criterion=c, **kw)
            assert len(blocks) == len(sizes)
            bo = qo = 0
            for (n, k), blk in zip(sizes, blocks):
                assert tuple(blk.shape) == (n, k) and blk.dtype == (torch.float64 if fn is B.image_box_iou else torch.float32)
                ref = dense[bo:bo + n, qo:qo + k]
                assert np.array_equal(_np(blk).view(np.uint8), np.ascontiguousarray(ref).view(np.uint8)), (fn.__name__, c, n, k)
                bo, qo = bo + n, qo + k
    assert B.rotate_iou_frames([], []) == []


def test_empty_inputs_and_dtypes(g16, R):
    b = g16["bev_random_boxes"][:5]
    for n, k in ((0, 5), (5, 0), (0, 0)):
        out = B.rotate_iou(b[:n], b[:k])
        assert tuple(out.shape) == (n, k) and out.dtype == torch.float32
        r = R.rotate_iou_gpu_eval(b[:n].astype(np.float64), b[:k])
        assert r.shape == (n, k) and r.dtype == np.float32 and not r.any()
    assert tuple(B.box3d_iou(np.zeros((0, 7)), g16["d3_cam_random_qboxes"]).shape) == (0, 45)
    assert tuple(B.image_box_iou(g16["img_boxes"], np.zeros((0, 4))).shape) == (60, 0)
    # float64 inputs are cast to float32 as the reference casts them
    b64 = g16["bev_cluster_boxes"].astype(np.float64) + 1e-9
    assert np.array_equal(_np(B.rotate_iou(b64, b64)), _np(B.rotate_iou(b64.astype(np.float32), b64.astype(np.float32))))
    # device tensors in, device tensor out on the same device, no host round trip needed
    t = torch.from_numpy(g16["bev_cluster_boxes"]).cuda()
    out = B.rotate_iou(t, t)
    assert out.is_cuda and np.array_equal(_np(out), _np(B.rotate_iou(g16["bev_cluster_boxes"], g16["bev_cluster_boxes"])))


def _shards(num, num_shards):
    """Detection3DEvaluator.get_shards (detection_3d.py:634-657)"""
    per, rem = num // num_shards, num % num_shards
    full = num_shards * (per > 0)
    return [per] * full + ([rem] if rem else [])


def test_evaluator_sharded_bev_and_3d_on_the_compat_module(g16, R):
    """the BEV and 3-D branches of Detection3DEvaluator.calculate_match_degree_sharded (detection_3d.py:550-632), copied, on the compat
    functions: shard matrices and per-frame slices"""
    for camera in (True, False):
        fr = "cam" if camera else "lidar"
        gt_all, dt_all = g16["d3_%s_cluster_qboxes" % fr], g16["d3_%s_cluster_boxes" % fr]
        gt_n = [4, 0, 7, 5, 3, 9, 2, 7]
        dt_n = [5, 3, 0, 6, 4, 8, 6, 8]
        gt_annos, dt_annos, go, do = [], [], 0, 0
        for ng, nd in zip(gt_n, dt_n):
            for lst, src, o, n in ((gt_annos, gt_all, go, ng), (dt_annos, dt_all, do, nd)):
                rows = src[o:o + n]
                lst.append({"name": np.array(["Car"] * n), "location": rows[:, 0:3], "dimensions": rows[:, 3:6], "rotation_y": rows[:, 6]})
            go, do = go + ng, do + nd
        total_gt = np.stack([len(a["name"]) for a in gt_annos], 0)
        total_dt = np.stack([len(a["name"]) for a in dt_annos], 0)
        cols2 = [0, 2] if camera else [0, 1]
        for metric in ("bev", "3d"):
            shards = _shards(len(gt_annos), 3)
            by_shard, idx = [], 0
            for nps in shards:
                gp, dp = gt_annos[idx:idx + nps], dt_annos[idx:idx + nps]
                if metric == "bev":
                    gt_boxes = np.concatenate([np.concatenate([a["location"][:, cols2] for a in gp], 0),
                                               np.concatenate([a["dimensions"][:, cols2] for a in gp], 0),
                                               np.concatenate([a["rotation_y"] for a in gp], 0)[..., np.newaxis]], axis=1)
                    dt_boxes = np.concatenate([np.concatenate([a["location"][:, cols2] for a in dp], 0),
                                               np.concatenate([a["dimensions"][:, cols2] for a in dp], 0),
                                               np.concatenate([a["rotation_y"] for a in dp], 0)[..., np.newaxis]], axis=1)
                    m = R.rotate_iou_gpu_eval(dt_boxes, gt_boxes, -1).astype(np.float64)
                    ref = np.squeeze(rotate_iou_np(dt_boxes, gt_boxes, (-1,))[0], 0).astype(np.float64)
                else:
                    gt_boxes = np.concatenate([np.concatenate([a["location"] for a in gp], 0), np.concatenate([a["dimensions"] for a in gp], 0),
                                               np.concatenate([a["rotation_y"] for a in gp], 0)[..., np.newaxis]], axis=1)
                    dt_boxes = np.concatenate([np.concatenate([a["location"] for a in dp], 0), np.concatenate([a["dimensions"] for a in dp], 0),
                                               np.concatenate([a["rotation_y"] for a in dp], 0)[..., np.newaxis]], axis=1)
                    cols = [0, 2, 3, 5, 6] if camera else [0, 1, 3, 4, 6]
                    rinc = R.rotate_iou_gpu_eval(dt_boxes[:, cols], gt_boxes[:, cols], 2)
                    R.d3_box_overlap_kernel(dt_boxes, gt_boxes, rinc, -1, camera)
                    m = rinc.astype(np.float64)
                    ref = d3_np(dt_boxes, gt_boxes, rotate_iou_np(dt_boxes[:, cols], gt_boxes[:, cols], (2,))[0][0], -1, camera).astype(np.float64)
                    frames = B.box3d_iou_frames([a for a in _stack7(dp)], [a for a in _stack7(gp)], -1, camera_frame=camera)
                    fo_d = fo_g = 0
                    for f, blk in enumerate(frames):
                        nd, ng = len(dp[f]["name"]), len(gp[f]["name"])
                        assert np.array_equal(_np(blk).astype(np.float64), m[fo_d:fo_d + nd, fo_g:fo_g + ng])
                        fo_d, fo_g = fo_d + nd, fo_g + ng
                assert np.array_equal(m, ref), (fr, metric)
                by_shard.append(m)
                idx += nps
            overlaps, idx = [], 0
            for j, nps in enumerate(shards):
                gi = di = 0
                for i in range(nps):
                    overlaps.append(by_shard[j][di:di + total_dt[idx + i], gi:gi + total_gt[idx + i]])
                    gi += total_gt[idx + i]
                    di += total_dt[idx + i]
                idx += nps
            assert [o.shape for o in overlaps] == list(zip(dt_n, gt_n))
            if metric == "3d":
                # every frame's slice equals the frame's own block of G16's matrix (the same boxes, evaluated in one piece there)
                full = g16["d3_%s_cluster_iou" % fr][0]
                d = g16["d3_%s_cluster_defined" % fr].astype(bool)
                go = do = 0
                for o, ng, nd in zip(overlaps, gt_n, dt_n):
                    blk, dd = full[do:do + nd, go:go + ng], d[do:do + nd, go:go + ng]
                    assert np.array_equal(o[dd], blk[dd].astype(np.float64))
                    go, do = go + ng, do + nd


def _stack7(annos):
    return [np.concatenate([a["location"], a["dimensions"], a["rotation_y"][:, None]], axis=1) for a in annos]
