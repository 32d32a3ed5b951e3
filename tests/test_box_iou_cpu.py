"""Box overlaps of the evaluator, host side (no GPU): a numpy float32 restatement of the reference's rotate_iou.py arithmetic pinned to
golden G16, the compat module's precedence over the reference's own pipelines/rotate_iou.py, and the refusal to compute on the host.

The restatement mirrors csrc/box_iou.hip, including its 16-point polygon: on the pairs the reference defines (at most 8 candidate points)
it equals G16; on the others it is what the kernel computes (tests/test_gpu_box_iou.py)."""
import math
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G16 = os.path.join(ROOT, "tests", "golden", "g16_box_iou.npz")
COMPAT = os.path.join(ROOT, "sdflabel_amd", "compat")
CAP = 16
f32 = np.float32


def corners(box):
    """rbbox_to_corners: cos / sin of the float32 angle in double, rounded to float32; float32 products and sums"""
    x, y, dx, dy, a = (f32(v) for v in box)
    c, s = f32(math.cos(float(a))), f32(math.sin(float(a)))
    cx = (-dx / f32(2), -dx / f32(2), dx / f32(2), dx / f32(2))
    cy = (-dy / f32(2), dy / f32(2), dy / f32(2), -dy / f32(2))
    out = []
    for i in range(4):
        out += [c * cx[i] + s * cy[i] + x, (-s) * cx[i] + c * cy[i] + y]
    return out


def _inside(px, py, q):
    ab0, ab1, ad0, ad1 = q[2] - q[0], q[3] - q[1], q[6] - q[0], q[7] - q[1]
    ap0, ap1 = px - q[0], py - q[1]
    abab, abap = ab0 * ab0 + ab1 * ab1, ab0 * ap0 + ab1 * ap1
    adad, adap = ad0 * ad0 + ad1 * ad1, ad0 * ap0 + ad1 * ap1
    eps = f32(1e-4)
    return abab >= abap - eps and abap >= f32(0) - eps and adad >= adap - eps and adap >= f32(0) - eps


def _cross(p1, p2, i, j):
    i1, j1 = (i + 1) % 4, (j + 1) % 4
    A0, A1, B0, B1 = p1[2 * i], p1[2 * i + 1], p1[2 * i1], p1[2 * i1 + 1]
    C0, C1, D0, D1 = p2[2 * j], p2[2 * j + 1], p2[2 * j1], p2[2 * j1 + 1]
    BA0, BA1, DA0, CA0, DA1, CA1 = B0 - A0, B1 - A1, D0 - A0, C0 - A0, D1 - A1, C1 - A1
    if (DA1 * CA0 > CA1 * DA0) == ((D1 - B1) * (C0 - B0) > (C1 - B1) * (D0 - B0)):
        return None
    if (CA1 * BA0 > BA1 * CA0) == (DA1 * BA0 > BA1 * DA0):
        return None
    DC0, DC1 = D0 - C0, D1 - C1
    ABBA, CDDC = A0 * B1 - B0 * A1, C0 * D1 - D0 * C1
    DH, Dx, Dy = BA1 * DC0 - BA0 * DC1, ABBA * DC0 - BA0 * CDDC, ABBA * DC1 - BA1 * CDDC
    return Dx / DH, Dy / DH


def inter_area(p1, p2, cap=CAP):
    """intersection area of two corner lists (float32) and the number of candidate points before the capacity"""
    pts = []
    for i in range(4):
        if _inside(p1[2 * i], p1[2 * i + 1], p2):
            pts.append((p1[2 * i], p1[2 * i + 1]))
        if _inside(p2[2 * i], p2[2 * i + 1], p1):
            pts.append((p2[2 * i], p2[2 * i + 1]))
    for i in range(4):
        for j in range(4):
            r = _cross(p1, p2, i, j)
            if r is not None:
                pts.append(r)
    count = len(pts)
    pts = pts[:cap]
    n = len(pts)
    if n < 3:
        return f32(0), count
    c0, c1 = f32(0), f32(0)
    for x, y in pts:
        c0, c1 = c0 + x, c1 + y
    c0, c1 = c0 / f32(n), c1 / f32(n)
    keys = []
    for x, y in pts:
        v0, v1 = x - c0, y - c1
        d = f32(math.sqrt(float(v0 * v0 + v1 * v1)))
        v0, v1 = v0 / d, v1 / d
        keys.append(f32(-2) - v0 if v1 < 0 else v0)
    for i in range(1, n):          # the reference's insertion sort
        if keys[i - 1] > keys[i]:
            t, tp, j = keys[i], pts[i], i
            while j > 0 and keys[j - 1] > t:
                keys[j], pts[j] = keys[j - 1], pts[j - 1]
                j -= 1
            keys[j], pts[j] = t, tp
    a = f32(0)
    for i in range(n - 2):
        (a0, a1), (b0, b1), (e0, e1) = pts[0], pts[i + 1], pts[i + 2]
        a = a + abs(((a0 - e0) * (b1 - e1) - (a1 - e1) * (b0 - e0)) / f32(2))
    return a, count


def with_criterion(ai, qarea, barea, c):
    if c == -1:
        return ai / (qarea + barea - ai)
    if c == 0:
        return ai / qarea
    if c == 1:
        return ai / barea
    return ai


def rotate_iou_np(boxes, qboxes, criteria=(-1, 0, 1, 2)):
    """[len(criteria)][N][K] float32 and the candidate counts [N][K]: pair (n, k) = devRotateIoUEval(qboxes[k], boxes[n])"""
    boxes, qboxes = np.asarray(boxes, np.float32), np.asarray(qboxes, np.float32)
    bc, qc = [corners(b) for b in boxes], [corners(q) for q in qboxes]
    out = np.zeros((len(criteria), len(boxes), len(qboxes)), np.float32)
    cnt = np.zeros((len(boxes), len(qboxes)), np.int32)
    with np.errstate(all="ignore"):
        for n, b in enumerate(boxes):
            for k, q in enumerate(qboxes):
                ai, cnt[n, k] = inter_area(qc[k], bc[n])
                for ci, c in enumerate(criteria):
                    out[ci, n, k] = with_criterion(ai, q[2] * q[3], b[2] * b[3], c)
    return out, cnt


def d3_np(boxes, qboxes, rinc, criterion, camera):
    """d3_box_overlap_kernel in float64 on a float32 rinc (a new array)"""
    r = rinc.copy()
    for i in range(boxes.shape[0]):
        for j in range(qboxes.shape[0]):
            if r[i, j] > 0:
                b, q = boxes[i], qboxes[j]
                iw = (min(b[1], q[1]) - max(b[1] - b[4], q[1] - q[4])) if camera else (min(b[2] + b[5], q[2] + q[5]) - max(b[2], q[2]))
                if iw > 0:
                    a1, a2 = b[3] * b[4] * b[5], q[3] * q[4] * q[5]
                    inc = iw * np.float64(r[i, j])
                    ua = {-1: a1 + a2 - inc, 0: a1, 1: a2}.get(criterion, inc)
                    r[i, j] = inc / ua
                else:
                    r[i, j] = 0.0
    return r


def image_np(boxes, qboxes, criterion):
    out = np.zeros((boxes.shape[0], qboxes.shape[0]), boxes.dtype)
    for k, q in enumerate(qboxes):
        qa = (q[2] - q[0]) * (q[3] - q[1])
        for n, b in enumerate(boxes):
            iw = min(b[2], q[2]) - max(b[0], q[0])
            if iw > 0:
                ih = min(b[3], q[3]) - max(b[1], q[1])
                if ih > 0:
                    ua = {-1: (b[2] - b[0]) * (b[3] - b[1]) + qa - iw * ih, 0: (b[2] - b[0]) * (b[3] - b[1]), 1: qa}.get(criterion, 1.0)
                    out[n, k] = iw * ih / ua
    return out


@pytest.fixture(scope="module")
def g16():
    return np.load(G16)


def test_restatement_reproduces_g16_bev(g16):
    crit = tuple(int(c) for c in g16["criteria"])
    for name in g16["bev_cases"]:
        p = "bev_%s_" % name
        got, cnt = rotate_iou_np(g16[p + "boxes"], g16[p + "qboxes"], crit)
        d = g16[p + "defined"].astype(bool)
        assert np.array_equal(cnt, g16[p + "npts"]), name
        assert np.array_equal(d, cnt <= 8), name                   # the reference is defined exactly up to its 8-point array
        for ci in range(len(crit)):
            assert np.array_equal(got[ci][d], g16[p + "iou"][ci][d], equal_nan=True), (name, crit[ci])


def test_restatement_reproduces_g16_3d_and_image(g16):
    crit = tuple(int(c) for c in g16["criteria"])
    for name in g16["d3_cases"]:
        p = "d3_%s_" % name
        b, q, camera = g16[p + "boxes"], g16[p + "qboxes"], bool(g16[p + "camera"])
        cols = [0, 2, 3, 5, 6] if camera else [0, 1, 3, 4, 6]
        rinc = rotate_iou_np(b[:, cols], q[:, cols], (2,))[0][0]
        d = g16[p + "defined"].astype(bool)
        assert np.array_equal(rinc[d], g16[p + "rinc"][d]), name
        for ci, c in enumerate(crit):
            assert np.array_equal(d3_np(b, q, rinc, c, camera)[d], g16[p + "iou"][ci][d]), (name, c)
    for ci, c in enumerate(crit):
        assert np.array_equal(image_np(g16["img_boxes"], g16["img_qboxes"], c), g16["img_iou"][ci]), c


def test_g16_covers_the_issue_cases(g16):
    """overlapping pairs in every BEV case, undefined pairs where the reference overruns, and both frames for 3-D"""
    for name in g16["bev_cases"]:
        assert (g16["bev_%s_iou" % name][3] > 0).any(), name
    assert sum(int((g16["bev_%s_defined" % n] == 0).sum()) for n in g16["bev_cases"]) > 0
    assert {bool(g16["d3_%s_camera" % n]) for n in g16["d3_cases"]} == {True, False}


def _reference_like_tree(root):
    """a stand-in of the reference's layout: root/main.py and root/pipelines/ (no __init__.py) holding its own rotate_iou.py -- which
    must never be imported -- and an evaluator that imports the three functions the way detection_3d.py:31 does"""
    pkg = root / "pipelines"
    pkg.mkdir(parents=True)
    (pkg / "rotate_iou.py").write_text("raise ImportError('the reference-like numba.cuda rotate_iou.py was imported')\n")
    (pkg / "detection_3d_standin.py").write_text(
        "from pipelines.rotate_iou import (d3_box_overlap_kernel, image_box_overlap, rotate_iou_gpu_eval)  # noqa: F401\n")
    (root / "main.py").write_text(textwrap.dedent("""
        import os, sys
        import pipelines.detection_3d_standin as s
        import pipelines.rotate_iou as r
        print(os.path.dirname(os.path.abspath(s.__file__)))
        print(os.path.dirname(os.path.abspath(r.__file__)))
        print(int('numba' in sys.modules), int('mpi4py' in sys.modules))
        print(r.div_up(130, 64), sorted(n for n in ('rotate_iou_gpu_eval', 'd3_box_overlap_kernel', 'image_box_overlap', 'div_up')
                                         if callable(getattr(r, n))))
    """))
    return pkg


@pytest.mark.parametrize("launch", ["script", "compat_first"])
def test_compat_rotate_iou_wins_over_the_reference_portion(tmp_path, launch):
    """`python <reference>/main.py` with PYTHONPATH=<compat>:<repo> puts the reference root FIRST on sys.path (the script's directory);
    pipelines.rotate_iou must still resolve to the compat module and every other pipelines module to the reference's directory.  Also
    with the compat directory ahead of the reference root.  numba and mpi4py are never imported."""
    ref = tmp_path / "reference"
    pkg = _reference_like_tree(ref)
    work = tmp_path / "elsewhere"
    work.mkdir()
    if launch == "script":
        env = dict(os.environ, PYTHONPATH=os.pathsep.join([COMPAT, ROOT]))
        cmd = [sys.executable, str(ref / "main.py")]
    else:
        env = dict(os.environ, PYTHONPATH=os.pathsep.join([COMPAT, str(ref), ROOT]))
        cmd = [sys.executable, "-c", "import runpy; runpy.run_path(%r)" % str(ref / "main.py")]
    res = subprocess.run(cmd, env=env, cwd=str(work), capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    lines = res.stdout.strip().splitlines()
    assert os.path.realpath(lines[0]) == os.path.realpath(str(pkg))
    assert os.path.realpath(lines[1]) == os.path.realpath(os.path.join(COMPAT, "pipelines"))
    assert lines[2] == "0 0"
    assert lines[3] == "3 ['d3_box_overlap_kernel', 'div_up', 'image_box_overlap', 'rotate_iou_gpu_eval']"


def test_no_host_fallback_without_gpu(g16):
    """without a GPU every entry point raises SdfrError instead of computing on the host"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: tests/test_gpu_box_iou.py covers the device path")
    sys.path.insert(0, COMPAT)
    try:
        import pipelines.rotate_iou as R
    finally:
        sys.path.remove(COMPAT)
        sys.modules.pop("pipelines.rotate_iou", None)
        sys.modules.pop("pipelines", None)
    from sdflabel_amd import SdfrError, box_iou
    b, q = g16["bev_random_boxes"][:3], g16["bev_random_qboxes"][:2]
    b3, q3 = g16["d3_cam_random_boxes"][:3], g16["d3_cam_random_qboxes"][:2]
    calls = [lambda: R.rotate_iou_gpu_eval(b, q), lambda: R.d3_box_overlap_kernel(b3, q3, np.ones((3, 2), np.float32), -1, True),
             lambda: R.image_box_overlap(g16["img_boxes"][:3], g16["img_qboxes"][:2]), lambda: box_iou.rotate_iou(b, q),
             lambda: box_iou.box3d_iou(b3, q3), lambda: box_iou.image_box_iou(g16["img_boxes"], g16["img_qboxes"]),
             lambda: box_iou.rotate_iou_frames([b], [q])]
    for call in calls:
        with pytest.raises(SdfrError):
            call()
