"""pipelines/rotate_iou.py of the reference (numba.cuda + mpi4py there) on sdflabel_amd.box_iou: same names and signatures.

The package next to this file (__init__.py) makes pipelines.rotate_iou (and pipelines.detection_3d) resolve here and the other pipelines modules to the
reference's directory, whichever of the two comes first on sys.path.  Imports neither numba nor mpi4py; every overlap is computed on the device (no
GPU: SdfrError).

Dtypes: the reference computes d3_box_overlap_kernel and image_box_overlap in the dtype of its inputs (numba).  Here they compute in
float64 with rinc read as float32: the reference's bits for float64 boxes and a float32 rinc, which is what Detection3DEvaluator passes
(location / dimensions / rotation_y / bbox arrays of float64, rinc from rotate_iou_gpu_eval).  Float32 boxes or a float64 rinc give
float64-accurate results that can differ from the reference's in the last bits.
"""
import numpy as np

from sdflabel_amd import box_iou as _b


def div_up(m, n):
    return m // n + (m % n > 0)


def rotate_iou_gpu_eval(boxes, query_boxes, criterion=-1, device_id=0):
    """[N][K] float32 rotated BEV overlap of boxes [N][5] and query_boxes [K][5] (cast to float32).  Always float32, as the reference:
    it re-binds `boxes` to its float32 copy before the final astype.  criterion 0 divides by the QUERY box's area, 1 by the box's
    (the reference evaluates devRotateIoUEval(query_boxes[k], boxes[n]))."""
    boxes = np.asarray(boxes).astype(np.float32)
    query_boxes = np.asarray(query_boxes).astype(np.float32)
    N, K = boxes.shape[0], query_boxes.shape[0]
    if N == 0 or K == 0:
        return np.zeros((N, K), dtype=np.float32)
    return _b.rotate_iou(boxes, query_boxes, criterion, device="cuda:%d" % device_id).cpu().numpy()


def d3_box_overlap_kernel(boxes, qboxes, rinc, criterion=-1, camera_coordinate=False):
    """Updates rinc [N][K] (the BEV intersections of rotate_iou_gpu_eval(..., 2)) in place with the 3-D overlap of boxes [N][7] and
    qboxes [K][7], computed on the device (sdfr_box3d_iou on the given rinc): pairs with rinc <= 0 keep it, pairs without vertical
    overlap get 0, the others inc / ua in float64 rounded to float32 (criterion 0: / the volume of boxes[i], 1: / the volume of
    qboxes[j]).  Boxes are read as float64 and rinc as float32, the dtypes the evaluator passes; other dtypes are converted first, so
    their results can differ from the reference's same-dtype arithmetic in the last bits (see the module docstring)."""
    import torch
    N, K = np.shape(boxes)[0], np.shape(qboxes)[0]
    if N == 0 or K == 0:
        return
    dev = _b._device(None, boxes, qboxes)
    b = _b._rows(boxes, 7, torch.float64, dev, "boxes")
    q = _b._rows(qboxes, 7, torch.float64, dev, "qboxes")
    r = _b._upload(torch.from_numpy(np.ascontiguousarray(rinc, dtype=np.float32).reshape(N, K)), dev)
    _b._launch("3d", b, q, 0, None, _b._criterion(criterion), bool(camera_coordinate), r, rinc=r)
    rinc[...] = r.cpu().numpy()


def image_box_overlap(boxes, query_boxes, criterion=-1):
    """[N][K] axis-aligned overlap of image boxes [N][4] and query_boxes [K][4], computed in float64, returned in boxes.dtype: the
    reference's bits for float64 boxes (the evaluator's); float32 boxes can differ from its float32 arithmetic in the last bits."""
    boxes = np.asarray(boxes)
    N, K = boxes.shape[0], np.shape(query_boxes)[0]
    if N == 0 or K == 0:
        return np.zeros((N, K), dtype=boxes.dtype)
    return _b.image_box_iou(boxes, query_boxes, criterion).cpu().numpy().astype(boxes.dtype, copy=False)
