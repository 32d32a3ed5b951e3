"""G16: golden vectors of the reference's box overlaps (pipelines/rotate_iou.py: devRotateIoUEval, d3_box_overlap_kernel, image_box_overlap).

Runs the reference's own module (tools/_ref_import.py: read-only) with numba, numba.cuda and mpi4py stubbed -- neither is installed here:
`numba.jit(...)` / `cuda.jit(...)` return the function unchanged, `cuda.local.array` / `cuda.shared.array` return float32 zeros,
MPI.COMM_WORLD.Get_rank() is 0 and torch.cuda.device_count() is 1 for the import-time `select_device`.  The device functions then run as
plain Python on numpy float32 scalars, which under NumPy >= 2 promotion (a Python float meets a float32 as a float32) is the float32
arithmetic of the kernel; the tool refuses to run under older promotion rules.  Pair (n, k) is devRotateIoUEval(qboxes[k], boxes[n], c),
the kernel's index map (rotate_iou.py:283-286).

quadrilateral_intersection is wrapped to record every pair's candidate count.  A pair with more than 8 candidates overruns the reference's
16-float array (an IndexError under the stub; undefined behaviour on a GPU): it is recorded with defined = 0 and its value is NaN.

usage: python tools/make_golden_iou.py      -> tests/golden/g16_box_iou.npz
"""
import math
import os
import sys
import types

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _ref_import  # noqa: E402

_ref_import.setup()

import numpy as np  # noqa: E402
import torch  # noqa: E402

assert isinstance(np.float32(1) * 1.5, np.float32), "NumPy >= 2 scalar promotion needed: the golden would become float64 arithmetic"

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "..", "tests", "golden", "g16_box_iou.npz")
CRITERIA = (-1, 0, 1, 2)


def _stub_modules():
    def passthrough(*a, **k):
        if len(a) == 1 and callable(a[0]) and not k:
            return a[0]
        return lambda f: f

    numba = types.ModuleType("numba")
    numba.jit = passthrough
    numba.float32 = np.float32
    cuda = types.ModuleType("numba.cuda")
    cuda.jit = passthrough
    cuda.select_device = lambda i: None
    arr = types.SimpleNamespace(array=lambda shape, dtype=None: np.zeros(shape, np.float32))
    cuda.local = arr
    cuda.shared = arr
    numba.cuda = cuda
    mpi = types.ModuleType("mpi4py")
    mpi.MPI = types.SimpleNamespace(COMM_WORLD=types.SimpleNamespace(Get_rank=lambda: 0))
    sys.modules.update({"numba": numba, "numba.cuda": cuda, "mpi4py": mpi})
    torch.cuda.device_count = lambda: 1


_stub_modules()
import pipelines.rotate_iou as R  # noqa: E402

assert R.local_rank == 0

_COUNT = [0]
_orig_qi = R.quadrilateral_intersection


def _recording_qi(pts1, pts2, int_pts):
    big = np.zeros(48, np.float32)
    _COUNT[0] = _orig_qi(pts1, pts2, big)      # the true candidate count, on an array that cannot overflow
    return _orig_qi(pts1, pts2, int_pts)       # the reference's call (IndexError past 8 points)


R.quadrilateral_intersection = _recording_qi


def bev_case(boxes, qboxes):
    """all four criteria of devRotateIoUEval(qboxes[k], boxes[n]); returns iou [4][N][K], npts [N][K], defined [N][K]"""
    N, K = boxes.shape[0], qboxes.shape[0]
    iou = np.full((len(CRITERIA), N, K), np.nan, np.float32)
    npts = np.zeros((N, K), np.int32)
    defined = np.ones((N, K), np.uint8)
    for n in range(N):
        for k in range(K):
            for ci, c in enumerate(CRITERIA):
                try:
                    iou[ci, n, k] = R.devRotateIoUEval(qboxes[k], boxes[n], c)
                except IndexError:
                    defined[n, k] = 0
                npts[n, k] = _COUNT[0]
    return iou, npts, defined


def kitti_bev(rng, n, spread=40.0, size=(1.5, 5.0)):
    b = np.empty((n, 5), np.float32)
    b[:, 0:2] = rng.uniform(-spread, spread, (n, 2))
    b[:, 2:4] = rng.uniform(size[0], size[1], (n, 2))
    b[:, 4] = rng.uniform(-np.pi, np.pi, n)
    return b


def touching(rng, n):
    """pairs sharing an edge: box, and the same box moved by its own width along its x axis (axis-aligned and rotated)"""
    b = kitti_bev(rng, n, 10.0)
    b[: n // 2, 4] = 0.0
    q = b.copy()
    c, s = np.cos(b[:, 4].astype(np.float64)), np.sin(b[:, 4].astype(np.float64))
    q[:, 0] = (b[:, 0] + c * b[:, 2]).astype(np.float32)
    q[:, 1] = (b[:, 1] - s * b[:, 2]).astype(np.float32)
    return b, q


def boxes3d(rng, n, spread, camera):
    """[x, y, z, d0, d1, d2, ry] float64; camera: y is the box's bottom (the vertical extent is [y - d1, y]); else z is its bottom"""
    b = np.empty((n, 7), np.float64)
    b[:, 0] = rng.uniform(-spread, spread, n)
    b[:, 3] = rng.uniform(3.0, 4.8, n)            # length
    b[:, 6] = rng.uniform(-np.pi, np.pi, n)
    if camera:
        b[:, 2] = rng.uniform(10.0, 10.0 + 2 * spread, n)
        b[:, 1] = rng.uniform(1.2, 2.2, n)
        b[:, 4] = rng.uniform(1.3, 1.9, n)        # height
        b[:, 5] = rng.uniform(1.4, 2.0, n)        # width
    else:
        b[:, 1] = rng.uniform(-spread, spread, n)
        b[:, 2] = rng.uniform(-2.2, -1.2, n)
        b[:, 4] = rng.uniform(1.4, 2.0, n)        # width
        b[:, 5] = rng.uniform(1.3, 1.9, n)        # height
    return b


def d3_case(boxes, qboxes, camera):
    cols = [0, 2, 3, 5, 6] if camera else [0, 1, 3, 4, 6]
    bev_b = boxes[:, cols].astype(np.float32)
    bev_q = qboxes[:, cols].astype(np.float32)
    N, K = boxes.shape[0], qboxes.shape[0]
    rinc = np.zeros((N, K), np.float32)
    defined = np.ones((N, K), np.uint8)
    for n in range(N):
        for k in range(K):
            try:
                rinc[n, k] = R.devRotateIoUEval(bev_q[k], bev_b[n], 2)
            except IndexError:
                defined[n, k] = 0
    outs = []
    for c in CRITERIA:
        r = rinc.copy()
        R.d3_box_overlap_kernel(boxes, qboxes, r, c, camera)
        r[defined == 0] = np.nan
        outs.append(r)
    rinc[defined == 0] = np.nan
    return rinc, np.stack(outs), defined


def image_boxes(rng, n, spread):
    xy = rng.uniform(0, spread, (n, 2))
    wh = rng.uniform(10, 200, (n, 2))
    return np.concatenate([xy, xy + wh], 1)


def main():
    rng = np.random.default_rng(16)
    data = {}
    cases = {}
    cases["random"] = (kitti_bev(rng, 150), kitti_bev(rng, 97))
    cases["cluster"] = (kitti_bev(rng, 70, 1.5), kitti_bev(rng, 67, 1.5))
    ident = kitti_bev(rng, 24, 3.0)
    cases["identical"] = (ident, ident.copy())
    cases["touching"] = touching(rng, 24)
    rot = kitti_bev(rng, 40, 3.0)
    rq = rot.copy()
    rq[0::2, 4] = (rot[0::2, 4] + np.float32(np.pi)).astype(np.float32)
    rq[1::2, 4] = (rot[1::2, 4] - np.float32(np.pi)).astype(np.float32)
    cases["rot_pi"] = (rot, rq)
    near = kitti_bev(rng, 40, 3.0)
    nq = near.copy()
    nq[:, 4] = (near[:, 4] + rng.uniform(-2e-5, 2e-5, 40)).astype(np.float32)
    cases["near_identical"] = (near, nq)
    data["bev_cases"] = np.array(list(cases))
    for name, (b, q) in cases.items():
        iou, npts, defined = bev_case(b, q)
        data["bev_%s_boxes" % name] = b
        data["bev_%s_qboxes" % name] = q
        data["bev_%s_iou" % name] = iou
        data["bev_%s_npts" % name] = npts
        data["bev_%s_defined" % name] = defined
        print("bev %-15s %3d x %3d  overlapping %5d  max points %2d  undefined %d" % (
            name, b.shape[0], q.shape[0], int((iou[3] > 0).sum()), int(npts.max()), int((defined == 0).sum())))
    d3 = {}
    for camera in (True, False):
        fr = "cam" if camera else "lidar"
        d3["%s_random" % fr] = (boxes3d(rng, 60, 20.0, camera), boxes3d(rng, 45, 20.0, camera))
        d3["%s_cluster" % fr] = (boxes3d(rng, 40, 1.5, camera), boxes3d(rng, 37, 1.5, camera))
    data["d3_cases"] = np.array(list(d3))
    for name, (b, q) in d3.items():
        camera = name.startswith("cam")
        rinc, outs, defined = d3_case(b, q, camera)
        data["d3_%s_boxes" % name] = b
        data["d3_%s_qboxes" % name] = q
        data["d3_%s_camera" % name] = np.int32(camera)
        data["d3_%s_rinc" % name] = rinc
        data["d3_%s_iou" % name] = outs
        data["d3_%s_defined" % name] = defined
        print("d3  %-15s %3d x %3d  overlapping %5d" % (name, b.shape[0], q.shape[0], int((outs[0] > 0).sum())))
    ib, iq = image_boxes(rng, 60, 400.0), image_boxes(rng, 50, 400.0)
    ib[:5] = iq[:5]                                     # identical pairs
    ib[5:10, 0] = iq[5:10, 2]                           # touching along x: iw == 0
    data["img_boxes"] = ib
    data["img_qboxes"] = iq
    data["img_iou"] = np.stack([R.image_box_overlap(ib, iq, c) for c in CRITERIA])
    data["criteria"] = np.array(CRITERIA, np.int32)
    np.savez_compressed(OUT, **data)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
