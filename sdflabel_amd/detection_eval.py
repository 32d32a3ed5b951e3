"""The evaluator of the reference (pipelines/detection_3d.py) with its match degrees, matching, thresholds and PR accumulation on the
device, behind sdfr_eval_* (csrc/detection_eval.hip) and the grouped box overlaps of csrc/box_iou.hip.

A list of annotation dicts is packed ONCE (`pack`): names mapped to small integers in one vectorised pass, every numeric column
concatenated, per-frame offsets.  The data filters (`clean_kitti_flags`, `distance_flags`: the two shipped ones, vectorised in numpy over
the packed columns; `callable_flags`: any other callable, called per frame as the reference calls it) give the flags of every (class,
difficulty).  `Session` uploads columns and flags in one copy each and computes, per metric and without a host synchronisation, the match
degrees of every frame in one launch, pass A, the thresholds (sort and recall walk) and pass B: the `pr` tables, thresholds and threshold counts as
device tensors.  `finish`, `mean_ap` and `format_result` are plain numpy on the few thousand numbers of those tables and need no GPU.

Nothing is computed on the host that the reference computes in its jitted functions: without a GPU `Session` raises SdfrError.
"""
import numpy as np
import torch

from . import _lib
from . import box_iou as _b

BBOX_2D, BEV_3D, BBOX_3D_KITTI, BBOX_3D_NU = 0, 1, 2, 3
LIDAR, VEHICLE, CAMERA = 0, 1, 2
_FLOAT_KEYS = (("truncated", 0), ("occluded", 0), ("alpha", 0), ("bbox", 4), ("dimensions", 3), ("location", 3), ("rotation_y", 0), ("score", 0))


# ---- packing ---------------------------------------------------------------------------------------------------------------------------

def _column(annos, key, width):
    """the concatenated float64 column `key` of all frames ([n] or [n][width]); None when a frame lacks it.  Device tensors are
    concatenated on their device and copied once."""
    try:
        vals = [a[key] for a in annos]
    except KeyError:
        return None
    shape = (0, width) if width else (0,)
    if not vals:
        return np.zeros(shape)
    if torch.Tensor in set(map(type, vals)):
        dev = next(v.device for v in vals if torch.is_tensor(v))
        ts = [(v.detach() if torch.is_tensor(v) else torch.as_tensor(np.asarray(v))).to(device=dev, dtype=torch.float64).reshape((-1,) + shape[1:])
              for v in vals]
        return torch.cat(ts).cpu().numpy()
    try:                    # arrays of one rank: a single concatenate
        col = np.concatenate(vals)
        if col.ndim == len(shape) and col.shape[1:] == shape[1:]:
            return col.astype(np.float64, copy=False)
    except (ValueError, TypeError):
        pass
    return np.concatenate([np.asarray(v, np.float64).reshape((-1,) + shape[1:]) for v in vals])


class Side:
    """one side (ground truths or detections) of a packed dataset: num [G], off [G + 1], name_id [n] and the float64 columns"""

    def __init__(self, annos):
        self.num = np.array([len(a["name"]) for a in annos], np.int64)
        self.off = np.concatenate([[0], np.cumsum(self.num)]).astype(np.int64)
        names = [n for a in annos for n in a["name"]]                     # lists or arrays of str, any mix
        self.names = np.char.lower(np.array(names, dtype=str)) if names else np.zeros(0, dtype="U1")
        self.n = int(self.off[-1])
        for key, width in _FLOAT_KEYS:
            col = _column(annos, key, width)
            if col is not None and col.shape[0] != self.n:
                raise ValueError("'%s' has %d rows for %d names" % (key, col.shape[0], self.n))
            setattr(self, key, col)


class Packed:
    """gt / dt: Side; vocab: the lower-case names of both sides, gt.name_id / dt.name_id index it"""

    def __init__(self, gt_annos, dt_annos):
        if len(gt_annos) != len(dt_annos):
            raise AssertionError("Must provide a prediction for every ground truth sample")
        self.G = len(gt_annos)
        self.gt, self.dt = Side(gt_annos), Side(dt_annos)
        vocab, inv = np.unique(np.concatenate([self.gt.names, self.dt.names]), return_inverse=True)
        self.vocab = [str(v) for v in vocab]
        self.gt.name_id = inv[:self.gt.n].astype(np.int32)
        self.dt.name_id = inv[self.gt.n:].astype(np.int32)
        self.ooff = np.concatenate([[0], np.cumsum(self.gt.num * self.dt.num)]).astype(np.int64)
        if self.gt.n >= 2 ** 31 or self.dt.n >= 2 ** 31:
            raise ValueError("too many boxes for one launch")

    def name_id(self, name):
        name = name.lower()
        return self.vocab.index(name) if name in self.vocab else -1


def pack(gt_annos, dt_annos):
    return Packed(list(gt_annos), list(dt_annos))


# ---- filters ---------------------------------------------------------------------------------------------------------------------------

class Flags:
    """flags of ML (class, difficulty) pairs: ign_gt int8 [ML][NG], ign_dt int8 [ML][ND], num_valid int64 [ML], the DontCare boxes
    dc_boxes float64 [n][4] and dc_off int32 [ML][G + 1] into them"""

    def __init__(self, ign_gt, ign_dt, num_valid, dc_boxes, dc_off):
        self.ign_gt, self.ign_dt, self.num_valid = np.ascontiguousarray(ign_gt, np.int8), np.ascontiguousarray(ign_dt, np.int8), np.asarray(num_valid, np.int64)
        self.dc_boxes, self.dc_off = np.ascontiguousarray(dc_boxes, np.float64).reshape(-1, 4), np.ascontiguousarray(dc_off, np.int32)

    def dc_lists(self, ml):
        return [self.dc_boxes[a:b] for a, b in zip(self.dc_off[ml][:-1], self.dc_off[ml][1:])]


KITTI_MAX_OCCLUSION = (0, 1, 2)
KITTI_MAX_TRUNCATION = (0.15, 0.3, 0.5)
KITTI_MIN_HEIGHT = (40, 25, 25)


def _kitti_one(P, cls_name, difficulty):
    cls_name = cls_name.lower()
    cur = P.name_id(cls_name)
    same = P.gt.name_id == cur
    close = np.zeros(P.gt.n, bool)
    for cls, neighbour in (("pedestrian", "person_sitting"), ("car", "van")):
        if cls_name == cls:
            close = P.gt.name_id == P.name_id(neighbour)
    height = P.gt.bbox[:, 3] - P.gt.bbox[:, 1]
    hard = (P.gt.occluded > KITTI_MAX_OCCLUSION[difficulty]) | (P.gt.truncated > KITTI_MAX_TRUNCATION[difficulty]) | \
        (height <= KITTI_MIN_HEIGHT[difficulty])                                  # ground truths: <=; detections below: <
    ign_gt = np.where(same & ~hard, 0, np.where((close & ~same) | (same & hard), 1, -1)).astype(np.int8)
    dheight = np.abs(P.dt.bbox[:, 3] - P.dt.bbox[:, 1])
    ign_dt = np.where(dheight < KITTI_MIN_HEIGHT[difficulty], 1, np.where(P.dt.name_id == cur, 0, -1)).astype(np.int8)
    return ign_gt, ign_dt


def _per_frame_counts(mask, off):
    c = np.concatenate([[0], np.cumsum(mask)])
    return c[off]                 # offsets [G + 1] into the selected rows


def clean_kitti_flags(P, class_names, difficulties):
    """clean_kitti_data for every (class, difficulty), vectorised over the packed columns.  DontCare boxes do not depend on the pair."""
    rows = [_kitti_one(P, c, d) for c in class_names for d in difficulties]
    dc = P.gt.name_id == P.name_id("dontcare")
    off = _per_frame_counts(dc, P.gt.off)
    ML = len(rows)
    return Flags(np.stack([r[0] for r in rows]) if ML else np.zeros((0, P.gt.n)), np.stack([r[1] for r in rows]) if ML else np.zeros((0, P.dt.n)),
                 [int((r[0] == 0).sum()) for r in rows], P.gt.bbox[dc], np.tile(off, (ML, 1)))


def distance_flags(P, class_names, difficulties, coordinate_frame, max_depth=(30, 80, 150), min_height=20):
    """difficulty_by_distance for every (class, difficulty)"""
    loc = P.gt.location
    dist = loc[:, 2] if coordinate_frame == CAMERA else np.sqrt(loc[:, 0] ** 2 + loc[:, 1] ** 2)
    dheight = np.abs(P.dt.bbox[:, 3] - P.dt.bbox[:, 1])
    ig, idt = [], []
    for c in class_names:
        cur = P.name_id(c)
        same = P.gt.name_id == cur
        for d in difficulties:
            far = dist > max_depth[d]
            ig.append(np.where(same & ~far, 0, np.where(same & far, 1, -1)).astype(np.int8))
            idt.append(np.where(dheight < min_height, 1, np.where(P.dt.name_id == cur, 0, -1)).astype(np.int8))
    ML = len(ig)
    return Flags(np.stack(ig) if ML else np.zeros((0, P.gt.n)), np.stack(idt) if ML else np.zeros((0, P.dt.n)),
                 [int((r == 0).sum()) for r in ig], np.zeros((0, 4)), np.zeros((ML, P.G + 1), np.int32))


def callable_flags(fn, gt_annos, dt_annos, class_ids, difficulties, id_to_name, coordinate_frame):
    """any filter with the reference's signature, called per (class, difficulty, frame); its flags and boxes are packed"""
    ig, idt, nv, boxes, offs = [], [], [], [], []
    for c in class_ids:
        for d in difficulties:
            a, b, n, off = [], [], 0, [len(boxes)]
            for g, p in zip(gt_annos, dt_annos):
                num_valid, ignored_gt, ignored_dt, ignored_boxes = fn(g, p, c, d, id_to_name, coordinate_frame)
                n += num_valid
                a += list(ignored_gt)
                b += list(ignored_dt)
                boxes += [np.asarray(x, np.float64).reshape(4) for x in ignored_boxes]
                off.append(len(boxes))
            ig.append(a)
            idt.append(b)
            nv.append(n)
            offs.append(off)
    ML = len(ig)
    return Flags(np.array(ig, np.int8).reshape(ML, -1), np.array(idt, np.int8).reshape(ML, -1), nv, np.array(boxes, np.float64).reshape(-1, 4),
                 np.array(offs, np.int32).reshape(ML, len(gt_annos) + 1))


def _single(gt_anno, dt_anno):
    return pack([gt_anno], [dt_anno])


def clean_kitti_data(gt_anno, dt_anno, current_class, difficulty, id_to_name, coordinate_frame=CAMERA):
    """the reference's filter for one frame: (num_valid_gt, ignored_gt, ignored_dt, DontCare boxes) as Python lists"""
    P = _single(gt_anno, dt_anno)
    F = clean_kitti_flags(P, [id_to_name[current_class]], [difficulty])
    return int(F.num_valid[0]), [int(v) for v in F.ign_gt[0]], [int(v) for v in F.ign_dt[0]], [b for b in F.dc_boxes]


def difficulty_by_distance(gt_anno, dt_anno, current_class, difficulty, id_to_name, coordinate_frame=LIDAR, max_depth=(30, 80, 150), min_height=20):
    P = _single(gt_anno, dt_anno)
    F = distance_flags(P, [id_to_name[current_class]], [difficulty], int(coordinate_frame), max_depth, min_height)
    return int(F.num_valid[0]), [int(v) for v in F.ign_gt[0]], [int(v) for v in F.ign_dt[0]], []


# ---- device ----------------------------------------------------------------------------------------------------------------------------

def _upload_blob(arrays, device):
    """{name: numpy array} -> {name: device tensor}: one pinned buffer, ONE asynchronous copy, views at 8-byte aligned offsets"""
    metas, at = [], 0
    for name, a in arrays.items():
        a = np.ascontiguousarray(a)
        metas.append((name, a, at))
        at += (a.nbytes + 7) // 8 * 8
    host = torch.empty(at + 8, dtype=torch.uint8).pin_memory()      # (+ 8: an empty last array still points inside the buffer)
    hv = host.numpy()
    for name, a, o in metas:
        hv[o:o + a.nbytes] = a.reshape(-1).view(np.uint8)
    blob = host.to(device, non_blocking=True)
    out = {}
    for name, a, o in metas:
        t = blob[o:o + a.nbytes].view(getattr(torch, str(a.dtype)))
        out[name] = t.reshape(a.shape)
    return out


def _device(device):
    if not torch.cuda.is_available():
        raise _lib.SdfrError("the evaluator's statistics run on the GPU only (no GPU is present); there is no CPU fallback")
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if device.type != "cuda":
        raise _lib.SdfrError("the evaluator's statistics run on the GPU only; there is no CPU fallback")
    return device


class Frames:
    """the per-frame offsets and the columns the statistics read, on the device.  From host arrays: one upload."""

    def __init__(self, gt_num, dt_num, dt_score, gt_yaw=None, dt_yaw=None, gt_alpha=None, dt_alpha=None, dt_bbox=None, extra=None, device=None):
        self.device = _device(device)
        gt_num, dt_num = np.asarray(gt_num, np.int64), np.asarray(dt_num, np.int64)
        self.G, self.NG, self.ND = len(gt_num), int(gt_num.sum()), int(dt_num.sum())
        self.max_nd = int(dt_num.max()) if self.G else 0
        self.cells = int((gt_num * dt_num).sum())
        arrays = dict(goff=np.concatenate([[0], np.cumsum(gt_num)]).astype(np.int32), doff=np.concatenate([[0], np.cumsum(dt_num)]).astype(np.int32),
                      ooff=np.concatenate([[0], np.cumsum(gt_num * dt_num)]).astype(np.int64), dt_score=np.asarray(dt_score, np.float64))
        for k, v in dict(gt_yaw=gt_yaw, dt_yaw=dt_yaw, gt_alpha=gt_alpha, dt_alpha=dt_alpha, dt_bbox=dt_bbox, **(extra or {})).items():
            if v is not None:
                arrays[k] = np.asarray(v, np.float64)
        self.t = _upload_blob(arrays, self.device)

    def get(self, name):
        return self.t.get(name)


def upload_flags(flags, device):
    return _upload_blob(dict(ign_gt=flags.ign_gt, ign_dt=flags.ign_dt, num_valid=flags.num_valid, dc_boxes=flags.dc_boxes, dc_off=flags.dc_off), device)


@_lib.traced("eval_center_dist")
def center_distances(fr, camera_frame):
    """minus the planar centre distance of every (detection, ground truth) pair inside a frame: flat float64 blocks [nd][ng] (needs the
    `dt_location` / `gt_location` columns in `fr`)"""
    out = torch.empty(fr.cells, dtype=torch.float64, device=fr.device)
    if fr.cells:
        with _lib.guard(out):
            rc = _lib.lib().sdfr_eval_center_dist(_lib.ptr(fr.t["dt_location"]), fr.ND, _lib.ptr(fr.t["gt_location"]), fr.NG, fr.G, _lib.ptr(fr.t["doff"]),
                                                  _lib.ptr(fr.t["goff"]), _lib.ptr(fr.t["ooff"]), int(bool(camera_frame)), _lib.ptr(out), out.numel(),
                                                  _lib.stream_ptr())
            _lib.check(rc, "sdfr_eval_center_dist")
    return out


@_lib.traced("eval_statistics")
def statistics(fr, overlaps, dflags, ML, K, min_overlap, sample_points=41, angular=False, dontcare=False, frames_per_chunk=0):
    """pass A, thresholds (sort and recall walk) and pass B of C = ML * K combinations on the device: four launches of the library
    and two fills, whatever the number of frames; no host synchronisation.

    fr: Frames; overlaps: flat float32 / float64 device tensor of the frames' [nd][ng] blocks; dflags: upload_flags(...); min_overlap: [C]
    (host).  Returns device tensors: pr [C][S][7], thr [C][S], nthr [C] int32, scores [C][NG] (pass A: a true positive's score at its
    ground truth, NaN elsewhere), count [C] int32."""
    h = _lib.lib()
    dev, S, C = fr.device, int(sample_points), int(ML) * int(K)
    min_overlap = np.asarray(min_overlap, np.float64).reshape(-1)
    if len(min_overlap) != C:
        raise ValueError("min_overlap must hold ML * K = %d values, got %d" % (C, len(min_overlap)))
    if overlaps.dtype not in (torch.float32, torch.float64) or overlaps.numel() != fr.cells or not overlaps.is_cuda:
        raise ValueError("overlaps must be a flat float32 / float64 device tensor of %d elements" % fr.cells)
    overlaps = overlaps.contiguous()
    f32 = int(overlaps.dtype == torch.float32)
    mo = _b._upload(torch.from_numpy(min_overlap), dev)
    ws_bytes = int(h.sdfr_eval_ws_bytes(fr.G, fr.NG, C, S, fr.max_nd, int(frames_per_chunk)))
    if ws_bytes < 0:
        raise ValueError("bad sizes for the evaluator's workspace")
    ws = torch.empty((ws_bytes + 7) // 8, dtype=torch.int64, device=dev)
    scores = torch.full((C, fr.NG), float("nan"), dtype=torch.float64, device=dev)
    pr = torch.empty((C, S, 7), dtype=torch.float64, device=dev)
    thr = torch.empty((C, S), dtype=torch.float64, device=dev)
    nthr = torch.empty((C,), dtype=torch.int32, device=dev)
    count = torch.empty((C,), dtype=torch.int32, device=dev)
    t = fr.t
    p = _lib.ptr
    with _lib.guard(pr):
        st = _lib.stream_ptr()
        _lib.check(h.sdfr_eval_match_scores(p(overlaps), f32, overlaps.numel(), p(t["ooff"]), p(t["doff"]), p(t["goff"]), fr.G, fr.ND, fr.NG,
                                            p(t["dt_score"]), p(dflags["ign_dt"]), p(dflags["ign_gt"]), ML, K, p(mo), fr.max_nd, p(ws), ws_bytes,
                                            p(scores), st), "sdfr_eval_match_scores")
        _lib.check(h.sdfr_eval_thresholds(p(scores), fr.NG, p(dflags["num_valid"]), ML, K, S, p(ws), ws_bytes, p(thr), p(nthr), p(count), st),
                   "sdfr_eval_thresholds")
        use_dc = bool(dontcare)
        _lib.check(h.sdfr_eval_pr(p(overlaps), f32, overlaps.numel(), p(t["ooff"]), p(t["doff"]), p(t["goff"]), fr.G, fr.ND, fr.NG, p(t["dt_score"]),
                                  p(t.get("dt_yaw")) if angular else None, p(t.get("dt_alpha")) if angular else None,
                                  p(t.get("gt_yaw")) if angular else None, p(t.get("gt_alpha")) if angular else None,
                                  p(t.get("dt_bbox")) if use_dc else None, p(dflags["ign_dt"]), p(dflags["ign_gt"]),
                                  p(dflags["dc_boxes"]) if use_dc else None, int(dflags["dc_boxes"].shape[0]) if use_dc else 0,
                                  p(dflags["dc_off"]) if use_dc else None, ML, K, p(mo), p(thr), p(nthr), S, int(bool(angular)), fr.max_nd,
                                  int(frames_per_chunk), p(ws), ws_bytes, p(pr), st), "sdfr_eval_pr")
    return dict(pr=pr, thr=thr, nthr=nthr, scores=scores, count=count)


class Session:
    """one `evaluate` call on the device: the packed columns uploaded once, reused by all four metrics"""

    def __init__(self, packed, coordinate_frame=LIDAR, device=None):
        self.device = _device(device)
        self.P, self.camera = packed, int(coordinate_frame) == CAMERA
        g, d = packed.gt, packed.dt
        for side, s in (("ground truths", g), ("detections", d)):
            for k in ("bbox", "dimensions", "location", "rotation_y"):
                if getattr(s, k) is None:
                    raise KeyError("%s: '%s' is missing" % (side, k))
        if d.score is None:
            raise KeyError("detections: 'score' is missing")
        extra = dict(gt_location=g.location, dt_location=d.location, gt_dimensions=g.dimensions, dt_dimensions=d.dimensions, gt_bbox=g.bbox)
        self.fr = Frames(g.num, d.num, d.score, g.rotation_y, d.rotation_y, g.alpha, d.alpha, d.bbox, extra=extra, device=self.device)
        self._ov = {}

    def overlaps(self, metric):
        """flat match degrees of a metric ([nd][ng] blocks, detections against ground truths): one launch, cached"""
        metric = int(metric)
        if metric not in self._ov:
            t, fr = self.fr.t, self.fr
            offs = (t["doff"], t["goff"], t["ooff"])
            if metric == BBOX_2D:
                ov = _b.packed_iou("image", t["dt_bbox"], t["gt_bbox"], fr.G, offs, fr.cells)
            elif metric == BBOX_3D_NU:
                ov = center_distances(fr, self.camera)
            else:
                c = 2 if self.camera else 1           # (column slices, not an index list: building an index tensor would synchronise)
                if metric == BEV_3D:
                    boxes = [torch.stack([t[s + "_location"][:, 0], t[s + "_location"][:, c], t[s + "_dimensions"][:, 0], t[s + "_dimensions"][:, c],
                                          t[s + "_yaw"]], 1).to(torch.float32) for s in ("dt", "gt")]
                    ov = _b.packed_iou("bev", boxes[0], boxes[1], fr.G, offs, fr.cells)
                elif metric == BBOX_3D_KITTI:
                    boxes = [torch.cat([t[s + "_location"], t[s + "_dimensions"], t[s + "_yaw"][:, None]], 1) for s in ("dt", "gt")]
                    ov = _b.packed_iou("3d", boxes[0], boxes[1], fr.G, offs, fr.cells, camera=self.camera)
                else:
                    raise ValueError("Unknown metric")
            self._ov[metric] = ov
        return self._ov[metric]

    def flags(self, flags):
        return upload_flags(flags, self.device)

    def statistics(self, metric, dflags, ML, K, min_overlap, sample_points=41, angular=False, frames_per_chunk=0):
        return statistics(self.fr, self.overlaps(metric), dflags, ML, K, min_overlap, sample_points, angular, dontcare=int(metric) == BBOX_2D,
                          frames_per_chunk=frames_per_chunk)


# ---- host: tables -> curves, AP, text -----------------------------------------------------------------------------------------------------

CURVES = ("recall", "precision", "orientation_aoe", "orientation_aos", "tp_mean_error", "tp_mean_confidence_error")


def finish(pr, nthr, shape, distance_metric=False, angular=False):
    """pr [C][S][7] and nthr [C] (numpy) -> the reference's curves, each [M][L][K][S] with shape = (M, L, K): rows past the threshold count
    stay zero, 0 / 0 stays NaN"""
    pr = np.asarray(pr, np.float64)
    C, S = pr.shape[0], pr.shape[1]
    live = np.arange(S)[None, :] < np.asarray(nthr).reshape(C, 1)
    tp, fp, fn = pr[..., 0], pr[..., 1], pr[..., 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        out = dict(recall=tp / (tp + fn), precision=tp / (tp + fp), tp_mean_error=pr[..., 5] / tp, tp_mean_confidence_error=pr[..., 6] / tp)
        if not distance_metric:
            out["tp_mean_error"] = np.abs(1.0 - out["tp_mean_error"])
        out["orientation_aoe"] = pr[..., 3] / (tp + fp) if angular else np.zeros_like(tp)
        out["orientation_aos"] = pr[..., 4] / (tp + fp) if angular else np.zeros_like(tp)
    return {k: np.where(live, out[k], 0.0).reshape(tuple(shape) + (S,)) for k in CURVES}


def mean_ap(precision, recall, sample_points=41):
    """AP [M][L][K]: the precision interpolated at sample_points - 1 evenly spaced recalls (0 excluded), in percent"""
    total = 0
    for i in range(1, sample_points):
        r = 1. / (sample_points - 1) * i
        total = total + ((recall >= r) * precision).max(axis=3)
    return 100.0 * total / (sample_points - 1)


def format_result(ev_name, classes, difficulties, nuscenes, angular, thresholds, ap):
    """the evaluator's text.  classes: names; thresholds [metric][level][difficulty][class] (already restricted to `classes`);
    ap: dict with Box2DAP, BevAP, Box3DAP, AoeAP_iou, AosAP_iou or Box3DAP_Nu, AoeAP_dist"""
    s = ""
    for k, difficulty in enumerate(difficulties):
        s += "============================\n"
        s += "Difficuty Level {}:\n".format(difficulty)
        s += "============================\n"
        for j, name in enumerate(classes):
            for i in range(thresholds.shape[1]):
                s += "{} AP: \n".format(name)
                if nuscenes:
                    s += "NuScenes 3D   @ {:.2f}: {:.4f}\n".format(thresholds[BBOX_3D_NU, i, k, j], ap["Box3DAP_Nu"][j, k, i])
                    if angular:
                        s += "AOE_dist  @ {:.2f}: {:.2f}\n".format(thresholds[BBOX_3D_NU, i, k, j], ap["AoeAP_dist"][j, k, i])
                else:
                    s += "Bbox @ {:.2f}: {:.4f}\n".format(thresholds[BBOX_2D, i, k, j], ap["Box2DAP"][j, k, i])
                    s += "BEV  @ {:.2f}: {:.4f}\n".format(thresholds[BEV_3D, i, k, j], ap["BevAP"][j, k, i])
                    s += "3D   @ {:.2f}: {:.4f}\n".format(thresholds[BBOX_3D_KITTI, i, k, j], ap["Box3DAP"][j, k, i])
                    if angular:
                        s += "AOE_iou  @ {:.2f}: {:.2f}\n".format(thresholds[BBOX_3D_KITTI, i, k, j], ap["AoeAP_iou"][j, k, i])
                        s += "AOS_iou  @ {:.2f}: {:.2f}\n".format(thresholds[BBOX_3D_KITTI, i, k, j], ap["AosAP_iou"][j, k, i])
    return s


def level_thresholds(table, metric, L):
    """min_overlap [C], c = (class * L + difficulty) * K + level, of table [metric][level][difficulty][class] (already restricted to the
    evaluated classes); minus the distance for the distance metric"""
    tab = -1.0 * table[metric] if int(metric) == BBOX_3D_NU else table[metric]
    K, M = tab.shape[0], tab.shape[2]
    return np.array([tab[k, l, m] for m in range(M) for l in range(L) for k in range(K)], np.float64)
