"""G17: golden vectors of the reference's evaluator (pipelines/detection_3d.py: Detection3DEvaluator, clean_kitti_data,
difficulty_by_distance, get_thresholds, compute_statistics_jit, fused_compute_statistics).

Runs the reference's own module (tools/_ref_import.py: read-only) the way tools/make_golden_iou.py runs rotate_iou.py: numba, numba.cuda and
mpi4py stubbed, so the jitted functions run as plain Python -- IEEE arithmetic in source order, which is the definition the port is held to
(numba's fastmath build of the same source is not bit-defined).  rotate_iou_gpu_eval is a loop over devRotateIoUEval(qboxes[k], boxes[n], c).

filter_data_fn, compute_statistics, get_thresholds and fused_compute_statistics are wrapped to record what they see and return; the keys of
the archive are listed in tests/_eval_golden.py.  The conditions that keep a test on this file from hiding a
failure are asserted at the end (and again by the CPU test).

usage: python tools/make_golden_eval.py      -> tests/golden/g17_detection_eval.npz
"""
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(1, os.path.join(HERE, ".."))
import _ref_import  # noqa: E402

_ref_import.setup()

import numpy as np  # noqa: E402
import torch  # noqa: E402

assert isinstance(np.float32(1) * 1.5, np.float32), "NumPy >= 2 scalar promotion needed: the BEV overlaps would become float64 arithmetic"

OUT = os.path.join(HERE, "..", "tests", "golden", "g17_detection_eval.npz")


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

OVERRUN = [0]          # BEV pairs with more than 8 candidate points (the reference is undefined there)
PAIRS = [0]
_orig_qi = R.quadrilateral_intersection


def _counting_qi(pts1, pts2, int_pts):
    big = np.zeros(48, np.float32)
    if _orig_qi(pts1, pts2, big) > 8:
        OVERRUN[0] += 1
    return _orig_qi(pts1, pts2, int_pts)


R.quadrilateral_intersection = _counting_qi
_MEMO = {}


def _rotate_iou_loop(boxes, query_boxes, criterion=-1, device_id=0):
    boxes = boxes.astype(np.float32)
    query_boxes = query_boxes.astype(np.float32)
    key = (boxes.tobytes(), query_boxes.tobytes(), criterion)
    if key not in _MEMO:
        out = np.zeros((boxes.shape[0], query_boxes.shape[0]), np.float32)
        for n in range(boxes.shape[0]):
            for k in range(query_boxes.shape[0]):
                out[n, k] = R.devRotateIoUEval(query_boxes[k], boxes[n], criterion)
        PAIRS[0] += out.size
        _MEMO[key] = out
    return _MEMO[key].copy()


R.rotate_iou_gpu_eval = _rotate_iou_loop
import pipelines.detection_3d as D  # noqa: E402
from pipelines import constants as C  # noqa: E402

assert D.rotate_iou_gpu_eval is _rotate_iou_loop

METRIC_NAMES = ("bbox2d", "bev", "box3d", "nu")
NAMES = ["Car", "Van", "Pedestrian", "Person_sitting", "Cyclist", "Truck"]
ANNO_KEYS = ("truncated", "occluded", "alpha", "bbox", "dimensions", "location", "rotation_y", "score")


# ---- scenes ---------------------------------------------------------------------------------------------------------------------------

def _empty_anno():
    return dict(name=[], truncated=np.zeros(0), occluded=np.zeros(0), alpha=np.zeros(0), bbox=np.zeros((0, 4)), dimensions=np.zeros((0, 3)),
                location=np.zeros((0, 3)), rotation_y=np.zeros(0), score=np.zeros(0))


def _anno(rows):
    if not rows:
        return _empty_anno()
    a = dict(name=[r["name"] for r in rows])
    for k in ANNO_KEYS:
        a[k] = np.array([r[k] for r in rows], np.float64)
    return a


def _gt_object(rng, name):
    z = rng.uniform(6.0, 75.0)
    x = rng.uniform(-35.0, 35.0)
    dims = {"Car": (3.9, 1.5, 1.6), "Van": (5.0, 2.1, 1.9), "Truck": (8.0, 3.0, 2.5)}.get(name, (0.9, 1.75, 0.7))
    dims = tuple(d * rng.uniform(0.85, 1.15) for d in dims)
    hpx = 720.0 * dims[1] / z
    if rng.random() < 0.25:
        hpx = rng.choice([18.0, 24.0, 25.0, 31.0, 39.0, 40.0, 41.0]) + rng.choice([0.0, 0.0, 0.37])     # around the 25 / 40 px limits
    wpx = hpx * rng.uniform(0.5, 2.2)
    cx, cy = 620.0 + 720.0 * x / z, 190.0 + rng.uniform(-20, 20)
    ry = rng.uniform(-np.pi, np.pi)
    return dict(name=name, truncated=float(rng.choice([0.0, 0.0, 0.1, 0.2, 0.4, 0.6])), occluded=float(rng.choice([0, 0, 1, 2, 3])),
                alpha=ry - np.arctan2(x, z), bbox=[cx - wpx / 2, cy - hpx / 2, cx + wpx / 2, cy + hpx / 2], dimensions=list(dims),
                location=[x, 1.6 + rng.uniform(-0.2, 0.2), z], rotation_y=ry, score=0.0)


def _dontcare(rng):
    x1, y1 = rng.uniform(0, 1000), rng.uniform(100, 250)
    return dict(name="DontCare", truncated=-1.0, occluded=-1.0, alpha=-10.0, bbox=[x1, y1, x1 + rng.uniform(60, 200), y1 + rng.uniform(40, 110)],
                dimensions=[-1.0, -1.0, -1.0], location=[-1000.0, -1000.0, -1000.0], rotation_y=-10.0, score=0.0)


def _jitter(rng, g, score, name=None):
    d = dict(g)
    d["name"] = name or g["name"]
    d["location"] = list(np.array(g["location"]) + rng.normal(0, 0.25, 3) * [1, 0.2, 1])
    d["rotation_y"] = g["rotation_y"] + rng.normal(0, 0.15)
    d["alpha"] = g["alpha"] + rng.normal(0, 0.15)
    d["bbox"] = list(np.array(g["bbox"]) + rng.normal(0, 4.0, 4))
    d["dimensions"] = list(np.array(g["dimensions"]) * rng.uniform(0.95, 1.05, 3))
    d["score"] = score
    d["truncated"] = d["occluded"] = 0.0
    return d


def _score(rng):
    return float(np.round(rng.uniform(0.05, 1.0), 1).clip(0.1, 1.0))


def _frame(rng, n_obj, n_dc, p_drop=0.2, p_dup=0.25, n_fp=1):
    gts = [_gt_object(rng, str(rng.choice(NAMES, p=[0.4, 0.1, 0.2, 0.05, 0.2, 0.05]))) for _ in range(n_obj)]
    dcs = [_dontcare(rng) for _ in range(n_dc)]
    order = rng.permutation(len(gts) + len(dcs))
    allg = [(gts + dcs)[i] for i in order]
    dts = []
    for g in gts:
        if rng.random() < p_drop:
            continue
        dts.append(_jitter(rng, g, _score(rng), name=g["name"] if rng.random() < 0.9 else "Car"))
        if rng.random() < p_dup:
            dts.append(_jitter(rng, g, _score(rng)))
    for dc in dcs:                                     # false positives INSIDE DontCare boxes
        if rng.random() < 0.8:
            b = dc["bbox"]
            o = _gt_object(rng, str(rng.choice(["Car", "Pedestrian", "Cyclist"])))
            w, h = (b[2] - b[0]) * 0.5, max((b[3] - b[1]) * 0.9, 41.0)
            o["bbox"] = [b[0] + 2.0, b[1] + 1.0, b[0] + 2.0 + w, b[1] + 1.0 + min(h, b[3] - b[1] - 2.0)]
            o["score"] = _score(rng)
            dts.append(o)
    for _ in range(n_fp):
        if rng.random() < 0.6:
            o = _gt_object(rng, str(rng.choice(["Car", "Pedestrian", "Cyclist"])))
            o["score"] = _score(rng)
            dts.append(o)
    dts = [dts[i] for i in rng.permutation(len(dts))]
    return _anno(allg), _anno(dts)


def scene_kitti(seed=17, frames=57):
    rng = np.random.default_rng(seed)
    gt, dt = [], []
    for f in range(frames):
        if f == 5:                       # neither
            g, d = _empty_anno(), _empty_anno()
        elif f == 11:                    # no detection
            g, d = _frame(rng, 4, 1)
            d = _empty_anno()
        elif f == 23:                    # no ground truth
            g, d = _frame(rng, 3, 0)
            g = _empty_anno()
        else:
            n = int(rng.integers(0, 8))
            g, d = _frame(rng, n, int(rng.integers(0, min(2, 8 - n) + 1)))
        gt.append(g)
        dt.append(d)
    return gt, dt


def scene_ones():
    gt, dt = scene_kitti()
    for d in dt:
        d["score"] = np.ones_like(d["score"])
    return gt, dt


def scene_big(seed=171):
    rng = np.random.default_rng(seed)
    gt, dt = [], []
    for f in range(13):
        if f == 6:
            g, d = _frame(rng, 88, 2, p_drop=0.1, p_dup=0.3, n_fp=8)
        else:
            g, d = _frame(rng, int(rng.integers(1, 5)), int(rng.integers(0, 2)))
        gt.append(g)
        dt.append(d)
    assert len(gt[6]["name"]) == 90 and len(dt[6]["name"]) > 100, (len(gt[6]["name"]), len(dt[6]["name"]))
    return gt, dt


def scene_empty():
    return [_empty_anno() for _ in range(3)], [_empty_anno() for _ in range(3)]


# ---- recording ------------------------------------------------------------------------------------------------------------------------

class Recorder:
    def __init__(self):
        self.filter_calls = []       # (class, difficulty, num_valid, ign_gt, ign_dt, boxes) per frame, in call order
        self.scores = []             # per compute_statistics call
        self.thresholds = []         # per get_thresholds call: (scores in, num_gt, thresholds out)
        self.pr = []                 # distinct pr arrays in order of first sight

    def wrap_filter(self, fn):
        def filt(gt_anno, dt_anno, current_class, difficulty, id_to_name, coordinate_frame):
            r = fn(gt_anno, dt_anno, current_class, difficulty, id_to_name, coordinate_frame)
            self.filter_calls.append((current_class, difficulty) + tuple(r))
            return r
        return filt


def run_config(gt, dt, filter_name, frame, nuscenes, classes, difficulties, angular=True, sample_points=41):
    rec = Recorder()
    orig = (D.compute_statistics, D.get_thresholds, D.fused_compute_statistics)

    def cs(*a, **k):
        r = orig[0](*a, **k)
        rec.scores.append(np.array(r["thresholds"], np.float64))
        return r

    def gt_(scores, num_gt, num_sample_pts=41):
        inp = np.array(scores, np.float64)
        r = orig[1](scores, num_gt, num_sample_pts)
        rec.thresholds.append((inp, num_gt, np.array(r, np.float64)))
        return r

    def fs(overlaps, pr, *a, **k):
        if not rec.pr or rec.pr[-1] is not pr:
            rec.pr.append(pr)
        return orig[2](overlaps, pr, *a, **k)

    D.compute_statistics, D.get_thresholds, D.fused_compute_statistics = cs, gt_, fs
    try:
        ev = D.Detection3DEvaluator(rec.wrap_filter(getattr(D, filter_name)), coordinate_frame=frame, compute_angular_metrics=angular,
                                    compute_nuscenes=nuscenes, sample_points=sample_points)
        text, result = ev.evaluate_detection_3d(gt, dt, list(classes), difficulties=tuple(difficulties))
        overlaps = {}
        for metric in (0, 1, 3 if nuscenes else 2):
            ov, _, _, _ = ev.calculate_match_degree_sharded(gt, dt, D.Metrics(metric), 50)
            overlaps[metric] = ov
    finally:
        D.compute_statistics, D.get_thresholds, D.fused_compute_statistics = orig
    return rec, text, result, overlaps


def pack_annos(annos, prefix, data):
    data[prefix + "num"] = np.array([len(a["name"]) for a in annos], np.int32)
    data[prefix + "name"] = np.array([n for a in annos for n in a["name"]], dtype="U16")
    for k in ANNO_KEYS:
        parts = [np.asarray(a[k], np.float64) for a in annos]
        data[prefix + k] = np.concatenate(parts) if parts else np.zeros(0)


def store_config(data, key, scene, gt, dt, rec, text, result, overlaps, cfg):
    G = len(gt)
    M, L = len(cfg["classes"]), len(cfg["difficulties"])
    metrics = (0, 1, 3 if cfg["nuscenes"] else 2)
    S = cfg["sample_points"]
    data[key + "scene"] = np.array(scene)
    data[key + "filter"] = np.array(cfg["filter"])
    data[key + "frame"] = np.int32(cfg["frame"])
    data[key + "nuscenes"] = np.int32(cfg["nuscenes"])
    data[key + "angular"] = np.int32(cfg["angular"])
    data[key + "sample_points"] = np.int32(S)
    data[key + "classes"] = np.array(cfg["classes"])
    data[key + "difficulties"] = np.array(cfg["difficulties"], np.int32)
    data[key + "text"] = np.array(text)
    for name, v in result.items():
        if isinstance(v, dict):
            for cn, cv in v.items():
                data[key + "res_%s_%s" % (name, cn)] = cv
        else:
            data[key + "res_" + name] = v
    # flags: the filter is called once per (metric, class, difficulty, frame); every metric sees the same flags -- keep the first metric's
    per = M * L * G
    assert len(rec.filter_calls) == 3 * per, (len(rec.filter_calls), per)
    NG, ND = sum(len(a["name"]) for a in gt), sum(len(a["name"]) for a in dt)
    ign_gt, ign_dt = np.zeros((M * L, NG), np.int8), np.zeros((M * L, ND), np.int8)
    num_valid = np.zeros(M * L, np.int64)
    dc_num = np.zeros((M * L, G), np.int32)
    dc_boxes = []
    for ml in range(M * L):
        ig, idt = [], []
        for f in range(G):
            c = rec.filter_calls[ml * G + f]
            for other in (1, 2):                       # the other two metrics recorded the same
                o = rec.filter_calls[other * per + ml * G + f]
                assert c[2] == o[2] and list(c[3]) == list(o[3]) and list(c[4]) == list(o[4]) and len(c[5]) == len(o[5])
            num_valid[ml] += c[2]
            ig += list(c[3])
            idt += list(c[4])
            dc_num[ml, f] = len(c[5])
            dc_boxes += [np.asarray(b, np.float64) for b in c[5]]
        ign_gt[ml], ign_dt[ml] = ig, idt
    data[key + "ign_gt"], data[key + "ign_dt"], data[key + "num_valid"], data[key + "dc_num"] = ign_gt, ign_dt, num_valid, dc_num
    data[key + "dc_boxes"] = np.stack(dc_boxes) if dc_boxes else np.zeros((0, 4))
    # statistics, per metric in call order: combination c = (class m, difficulty l, level k)
    K = 2
    Cn = M * L * K
    assert len(rec.pr) == 3 * Cn and len(rec.thresholds) == 3 * Cn and len(rec.scores) == 3 * Cn * G
    for mi, metric in enumerate(metrics):
        mk = key + METRIC_NAMES[metric] + "_"
        pr = np.zeros((Cn, S, 7))
        thr = np.zeros((Cn, S))
        nthr = np.zeros(Cn, np.int32)
        sc, sc_off = [], [0]
        for c in range(Cn):
            n = mi * Cn + c
            t = rec.thresholds[n][2]
            nthr[c] = len(t)
            thr[c, :len(t)] = t
            pr[c, :len(t)] = rec.pr[n]
            s = np.concatenate(rec.scores[n * G:(n + 1) * G]) if G else np.zeros(0)
            assert np.array_equal(np.sort(s), np.sort(rec.thresholds[n][0]))
            sc.append(s)
            sc_off.append(sc_off[-1] + len(s))
        data[mk + "pr"], data[mk + "thr"], data[mk + "nthr"] = pr, thr, nthr
        data[mk + "scores"], data[mk + "scores_off"] = np.concatenate(sc), np.array(sc_off, np.int64)
        flat = np.concatenate([o.reshape(-1) for o in overlaps[metric]]) if G else np.zeros(0)
        okey = "ov_%s_%d_%s" % (scene, cfg["frame"], METRIC_NAMES[metric])
        stored = flat.astype(np.float32) if metric in (1, 2) else flat.astype(np.float64)
        assert np.array_equal(stored.astype(np.float64), flat)                     # BEV / 3-D overlaps are float32 values
        if okey in data:
            assert np.array_equal(data[okey], stored)
        data[okey] = stored


def main():
    data = {}
    scenes = {"kitti": scene_kitti(), "ones": scene_ones(), "big": scene_big(), "empty": scene_empty()}
    for s, (gt, dt) in scenes.items():
        pack_annos(gt, s + "_gt_", data)
        pack_annos(dt, s + "_dt_", data)
        sc = data[s + "_dt_score"]
        assert np.isfinite(sc).all() and (sc > 0).all() and (sc <= 1).all()
    data["id_to_name_ids"] = np.array(list(C.KITTI_CLASS_NAMES), np.int32)
    data["id_to_name_names"] = np.array(list(C.KITTI_CLASS_NAMES.values()))
    data["overlap_thresholds"] = C.KITTI_OVERLAP_THRESHOLDS
    data["dist_thresholds"] = C.NU_OVERLAP_THRESHOLDS
    CAM, LID = int(D.CoordinateFrame.CAMERA), int(D.CoordinateFrame.LIDAR)
    full = dict(filter="clean_kitti_data", frame=CAM, classes=["Car", "Pedestrian", "Cyclist"], difficulties=[0, 1, 2], angular=True,
                sample_points=41)
    car = dict(full, classes=["Car"])
    configs = [
        ("kitti_cam_kitti", "kitti", dict(full, nuscenes=False)),
        ("kitti_cam_nu", "kitti", dict(full, nuscenes=True)),
        ("kitti_lidar_nu", "kitti", dict(car, filter="difficulty_by_distance", frame=LID, nuscenes=True)),
        ("kitti_noang", "kitti", dict(car, nuscenes=False, angular=False)),
        ("kitti_sp11", "kitti", dict(car, nuscenes=True, sample_points=11)),
        ("kitti_dump_kitti", "kitti", dict(car, nuscenes=False, difficulties=[0, 1])),
        ("kitti_dump_nu", "kitti", dict(car, nuscenes=True, difficulties=[0, 1])),
        ("ones_cam_kitti", "ones", dict(full, nuscenes=False)),
        ("ones_cam_nu", "ones", dict(car, nuscenes=True)),
        ("big_cam_kitti", "big", dict(car, nuscenes=False)),
        ("big_cam_nu", "big", dict(car, nuscenes=True)),
        ("empty_cam_kitti", "empty", dict(car, nuscenes=False)),
        ("empty_cam_nu", "empty", dict(car, nuscenes=True)),
    ]
    data["configs"] = np.array([c[0] for c in configs])
    for name, scene, cfg in configs:
        gt, dt = scenes[scene]
        rec, text, result, overlaps = run_config(gt, dt, cfg["filter"], D.CoordinateFrame(cfg["frame"]), bool(cfg["nuscenes"]), cfg["classes"],
                                                 cfg["difficulties"], cfg["angular"], cfg["sample_points"])
        store_config(data, name + "_", scene, gt, dt, rec, text, result, overlaps, cfg)
        print("%-18s BEV pairs so far %7d, overruns %d" % (name, PAIRS[0], OVERRUN[0]))
        print(text.replace("\n", " | ")[:400])
    assert OVERRUN[0] == 0, "%d BEV pairs with more than 8 candidate points: the reference is undefined there" % OVERRUN[0]
    data["bev_pairs"] = np.int64(PAIRS[0])
    data["bev_overruns"] = np.int64(OVERRUN[0])
    from tests._eval_golden import golden_conditions
    print("conditions:", golden_conditions(data))
    np.savez_compressed(OUT, **data)
    size = os.path.getsize(OUT)
    print("wrote %s (%d bytes)" % (OUT, size))
    assert size < 1000000


if __name__ == "__main__":
    main()
