"""Box overlaps of the reference's evaluator (pipelines/rotate_iou.py, numba.cuda there) on the device, behind sdfr_rotate_iou,
sdfr_box3d_iou and sdfr_image_box_iou (csrc/box_iou.hip).

Every function takes numpy arrays or tensors, uploads host inputs through pinned memory with asynchronous copies, launches on the current
stream and returns device tensors without a host synchronisation.  Nothing is computed on the host: without a GPU they raise SdfrError.

Argument order, as in the reference: out[n][k] pairs boxes[n] with qboxes[k].  For the BEV IoU the reference evaluates
devRotateIoUEval(qboxes[k], boxes[n]) (rotate_iou.py:286), so criterion 0 divides the intersection by the QUERY box's area and criterion 1
by the box's; for the 3-D and image IoU (d3_box_overlap_kernel, image_box_overlap) criterion 0 divides by the box's volume / area and 1 by the
query box's.  Criterion -1 is the IoU, any other value returns the intersection itself (the 3-D IoU: 1 where the boxes overlap).

The `*_frames` variants take one array per frame for each side and evaluate only the pairs inside a frame, in one launch: a list of
[n_f][k_f] device tensors (views of one packed buffer), the blocks the evaluator slices out of its per-shard matrices
(detection_3d.py:550-632).
"""
import numpy as np
import torch

from . import _lib

_COLS = {"bev": 5, "3d": 7, "image": 4}
_NP = {torch.float32: np.float32, torch.float64: np.float64}


def _device(device, *arrays):
    if device is None:
        for a in arrays:
            if torch.is_tensor(a) and a.is_cuda:
                return a.device
    if not torch.cuda.is_available():
        raise _lib.SdfrError("box IoU runs on the GPU only (no GPU is present); there is no CPU fallback")
    if device is None:
        return torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    if device.type != "cuda":
        raise _lib.SdfrError("box IoU runs on the GPU only; there is no CPU fallback")
    return device


def _upload(host, device):
    """host tensor -> device without waiting: staged through pinned memory, copied asynchronously on the current stream"""
    return host.contiguous().pin_memory().to(device, non_blocking=True)


def _rows(a, cols, dtype, device, name):
    """[n][cols] array of `dtype` on `device`: device tensors are cast there, host arrays are cast on the host (numpy's astype, as the
    reference casts) and uploaded"""
    if torch.is_tensor(a):
        t = a.detach()
        if t.is_cuda:
            t = t.to(device=device, dtype=dtype)
        else:
            t = _upload(t.to(dtype), device)
    else:
        a = np.asarray(a)
        t = _upload(torch.from_numpy(np.ascontiguousarray(a.astype(_NP[dtype], copy=False))), device)
    if t.numel() == 0:
        return t.reshape(0, cols)
    if t.dim() != 2 or t.shape[1] != cols:
        raise ValueError("%s must be [n][%d], got %s" % (name, cols, tuple(t.shape)))
    return t.contiguous()


def _host_rows(a, cols, np_dtype, name):
    a = (a.detach().numpy() if torch.is_tensor(a) else np.asarray(a)).astype(np_dtype, copy=False)
    if a.size == 0:
        return a.reshape(0, cols)
    if a.ndim != 2 or a.shape[1] != cols:
        raise ValueError("%s must be [n][%d], got %s" % (name, cols, a.shape))
    return a


def _criterion(criterion):
    c = int(criterion)
    if c != criterion:
        raise ValueError("criterion must be an integer, got %r" % (criterion,))
    return c


def _launch(kind, b, q, G, offs, criterion, camera, out, rinc=None):
    h = _lib.lib()
    N, K = b.shape[0], q.shape[0]
    boff, qoff, ooff = offs if offs is not None else (None, None, None)
    args = (_lib.ptr(b), N, _lib.ptr(q), K, G, _lib.ptr(boff), _lib.ptr(qoff), _lib.ptr(ooff), criterion)
    with _lib.guard(out):
        if kind == "bev":
            rc = h.sdfr_rotate_iou(*args, _lib.ptr(out), out.numel(), _lib.stream_ptr())
        elif kind == "3d":
            rc = h.sdfr_box3d_iou(*args, int(bool(camera)), _lib.ptr(rinc), _lib.ptr(out), out.numel(), _lib.stream_ptr())
        else:
            rc = h.sdfr_image_box_iou(*args, _lib.ptr(out), out.numel(), _lib.stream_ptr())
        _lib.check(rc, "sdfr_%s_iou" % {"bev": "rotate", "3d": "box3d", "image": "image_box"}[kind])


_IN = {"bev": torch.float32, "3d": torch.float64, "image": torch.float64}
_OUT = {"bev": torch.float32, "3d": torch.float32, "image": torch.float64}


def _dense(kind, boxes, qboxes, criterion, camera=False, device=None):
    dev = _device(device, boxes, qboxes)
    c = _criterion(criterion)
    b = _rows(boxes, _COLS[kind], _IN[kind], dev, "boxes")
    q = _rows(qboxes, _COLS[kind], _IN[kind], dev, "qboxes")
    out = torch.empty((b.shape[0], q.shape[0]), dtype=_OUT[kind], device=dev)      # the launch writes every pair
    if out.numel():
        _launch(kind, b, q, 0, None, c, camera, out)
    return out


def _frames(kind, boxes_list, qboxes_list, criterion, camera=False, device=None):
    if len(boxes_list) != len(qboxes_list):
        raise ValueError("one boxes array and one qboxes array per frame: got %d and %d" % (len(boxes_list), len(qboxes_list)))
    dev = _device(device, *boxes_list, *qboxes_list)
    c = _criterion(criterion)
    G = len(boxes_list)
    if any(torch.is_tensor(a) and a.is_cuda for a in list(boxes_list) + list(qboxes_list)):
        bs = [_rows(a, _COLS[kind], _IN[kind], dev, "boxes") for a in boxes_list]
        qs = [_rows(a, _COLS[kind], _IN[kind], dev, "qboxes") for a in qboxes_list]
        nb = np.array([t.shape[0] for t in bs], np.int64)
        nq = np.array([t.shape[0] for t in qs], np.int64)
    else:       # host frames: cast and concatenate on the host, one upload per side
        hb = [_host_rows(a, _COLS[kind], _NP[_IN[kind]], "boxes") for a in boxes_list]
        hq = [_host_rows(a, _COLS[kind], _NP[_IN[kind]], "qboxes") for a in qboxes_list]
        nb = np.array([a.shape[0] for a in hb], np.int64)
        nq = np.array([a.shape[0] for a in hq], np.int64)
        bs = [_rows(np.concatenate(hb) if G else np.zeros((0, _COLS[kind])), _COLS[kind], _IN[kind], dev, "boxes")]
        qs = [_rows(np.concatenate(hq) if G else np.zeros((0, _COLS[kind])), _COLS[kind], _IN[kind], dev, "qboxes")]
    boff = np.concatenate([[0], np.cumsum(nb)])
    qoff = np.concatenate([[0], np.cumsum(nq)])
    ooff = np.concatenate([[0], np.cumsum(nb * nq)])
    if boff[-1] >= 2 ** 31 or qoff[-1] >= 2 ** 31:
        raise ValueError("too many boxes for one launch")
    out = torch.empty(int(ooff[-1]), dtype=_OUT[kind], device=dev)      # the launch writes every block
    if G and out.numel():
        b = torch.cat(bs) if len(bs) > 1 else bs[0]
        q = torch.cat(qs) if len(qs) > 1 else qs[0]
        offs = torch.from_numpy(np.concatenate([boff.astype(np.int32), qoff.astype(np.int32)]))
        offs = _upload(offs, dev)
        oo = _upload(torch.from_numpy(ooff), dev)
        _launch(kind, b, q, G, (offs[:G + 1], offs[G + 1:], oo), c, camera, out)
    return [t.view(n, k) for t, n, k in zip(out.split((nb * nq).tolist()), nb.tolist(), nq.tolist())]


@_lib.traced("packed_iou")
def packed_iou(kind, boxes, qboxes, G, offs, total, criterion=-1, camera=False):
    """Grouped overlaps of boxes that are packed on the device already: kind "bev" (float32 [n][5]), "3d" (float64 [n][7]) or "image"
    (float64 [n][4]); offs = (boff int32 [G + 1], qoff int32 [G + 1], ooff int64 [G + 1]) device tensors; total = ooff[G], known to the
    caller (no read-back).  One launch, no host synchronisation; returns the flat tensor of the groups' [n_g][k_g] blocks."""
    if boxes.dtype != _IN[kind] or qboxes.dtype != _IN[kind] or not boxes.is_cuda or not qboxes.is_cuda:
        raise ValueError("packed %s boxes must be %s device tensors" % (kind, _IN[kind]))
    if boxes.dim() != 2 or qboxes.dim() != 2 or boxes.shape[1] != _COLS[kind] or qboxes.shape[1] != _COLS[kind]:
        raise ValueError("packed %s boxes must be [n][%d]" % (kind, _COLS[kind]))
    out = torch.empty(int(total), dtype=_OUT[kind], device=boxes.device)      # the launch writes every block
    if G and out.numel():
        _launch(kind, boxes.contiguous(), qboxes.contiguous(), int(G), offs, _criterion(criterion), camera, out)
    return out


@_lib.traced("rotate_iou")
def rotate_iou(boxes, qboxes, criterion=-1, device=None):
    """Rotated BEV overlap [N][K] float32 of boxes [N][5] and query boxes [K][5] = [x, y, dx, dy, angle], cast to float32 as the
    reference casts.  criterion -1: IoU; 0: intersection / area of the QUERY box qboxes[k]; 1: intersection / area of boxes[n];
    other: the intersection area."""
    return _dense("bev", boxes, qboxes, criterion, device=device)


@_lib.traced("box3d_iou")
def box3d_iou(boxes, qboxes, criterion=-1, camera_frame=True, device=None):
    """3-D overlap [N][K] float32 of boxes [N][7] and query boxes [K][7] = [x, y, z, d0, d1, d2, ry] (float64, as the evaluator passes
    them): Detection3DEvaluator.box_3d_overlap in one launch.  The BEV intersection of columns [0, 2, 3, 5, 6] (camera frame, vertical
    axis y, boxes hanging down from y) or [0, 1, 3, 4, 6] (vertical axis z, boxes standing on z) in float32, then the vertical overlap,
    the volumes and the ratio in float64.  criterion -1: IoU; 0: / the volume of boxes[n]; 1: / the volume of qboxes[k]."""
    return _dense("3d", boxes, qboxes, criterion, camera_frame, device=device)


@_lib.traced("image_box_iou")
def image_box_iou(boxes, qboxes, criterion=-1, device=None):
    """Axis-aligned overlap [N][K] float64 of image boxes [N][4] and [K][4] = [x1, y1, x2, y2] (float64, no +1 pixel convention).
    criterion -1: IoU; 0: / the area of boxes[n]; 1: / the area of qboxes[k]; other: the intersection area."""
    return _dense("image", boxes, qboxes, criterion, device=device)


@_lib.traced("rotate_iou_frames")
def rotate_iou_frames(boxes_list, qboxes_list, criterion=-1, device=None):
    """rotate_iou of every frame (boxes_list[f] against qboxes_list[f]) in one launch: a list of [n_f][k_f] float32 device tensors"""
    return _frames("bev", boxes_list, qboxes_list, criterion, device=device)


@_lib.traced("box3d_iou_frames")
def box3d_iou_frames(boxes_list, qboxes_list, criterion=-1, camera_frame=True, device=None):
    """box3d_iou of every frame in one launch: a list of [n_f][k_f] float32 device tensors"""
    return _frames("3d", boxes_list, qboxes_list, criterion, camera_frame, device=device)


@_lib.traced("image_box_iou_frames")
def image_box_iou_frames(boxes_list, qboxes_list, criterion=-1, device=None):
    """image_box_iou of every frame in one launch: a list of [n_f][k_f] float64 device tensors"""
    return _frames("image", boxes_list, qboxes_list, criterion, device=device)
