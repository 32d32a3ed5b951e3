"""GPU timing of the evaluator (sdflabel_amd.detection_eval, csrc/detection_eval.hip) on a KITTI-val-shaped annotation list: the 3 769
frames tools/iou_time.py generates (30 063 ground-truth / 30 505 detected boxes), with names, scores, 2-D boxes, occlusion and truncation
added from a seed.  Car / Pedestrian / Cyclist x difficulties (0, 1, 2), both compute_nuscenes settings.

  evaluate      milliseconds from host annotation lists to result_dict (host clock around the call, which ends with the read-back)
  split         packing, upload, filters (+ their upload), the overlap launches per metric, the statistics (pass A, sort, thresholds,
                pass B) per metric between device events, the read-back and `finish`
  sync          host synchronisations per evaluate call (torch's sync debug mode: every synchronising torch call warns once)
  frames 377    the same for the first 377 frames: launches and synchronisations must not grow with the frame count
  overlap stage the parent's faster path from host arrays (box3d_dense_shards_from_host of tools/iou_time.py) against the packed path
                from host annotations (pack + upload + one grouped launch), alternating in the same run; the baseline's own spread
  pass B        inner-loop visits from shapes: sum over frames of gt x dt, times the sum over combinations of their threshold counts

Kernel times and launch counts come from separate profiled runs of `--calls FRAMES` (N evaluate calls, nothing else):
  rocprofv3 --kernel-trace --stats -d RP_DIR -o ev --output-format csv -- python tools/eval_time.py OUT_DIR --calls 3769
  python tools/eval_time.py OUT_DIR --trace RP_DIR_3769 RP_DIR_377
adds kernel_stats (per kernel: launches per evaluate call and time per call, at both frame counts), visits per second and the active
lanes per wave of pass B to OUT_DIR/eval_time.json.  The reference's own time is not measured: numba is not installed where this runs.

usage: python tools/eval_time.py OUT_DIR [--calls FRAMES | --trace RP_DIR_3769 RP_DIR_377]
"""
import csv
import glob
import json
import os
import sys
import time
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, HERE)
from iou_time import FRAMES, SHARDS, kitti_boxes3d, shards  # noqa: E402
from sdflabel_amd import box_iou as B  # noqa: E402
from sdflabel_amd import detection_eval as DE  # noqa: E402
from sdflabel_amd.pipelines import detection_3d as D3  # noqa: E402

WARM, REPS, CALLS = 2, 7, 4
CLASSES, DIFFS = ["Car", "Pedestrian", "Cyclist"], (0, 1, 2)
ID_TO_NAME = {0: "Cyclist", 1: "Van", 2: "Car", 3: "Truck", 4: "Pedestrian", 5: "Person_sitting", 6: "Tram"}


def tables():
    """KITTI-like threshold tables [metric][level][difficulty][class] built here (the tool does not read the reference)"""
    strict = np.array([0.5, 0.7, 0.7, 0.5, 0.5, 0.7, 0.5])
    loose = np.array([0.25, 0.5, 0.5, 0.25, 0.25, 0.5, 0.5])
    iou = np.stack([np.stack([np.tile(strict, (3, 1)), np.tile(strict if m == 0 else loose, (3, 1))]) for m in range(4)])
    dist = np.stack([np.stack([np.full((3, 7), 0.5), np.full((3, 7), 1.0)])] * 4)
    return iou, dist


def kitti_val_annotations():
    """tools/iou_time.py's frame list (same generator state), as annotation dicts"""
    rng = np.random.default_rng(0)
    for n in (1024, 4096):                       # the dense cases iou_time.py draws first
        kitti_boxes3d(rng, n), kitti_boxes3d(rng, n)
    ng, nd = rng.integers(1, 16, FRAMES), rng.integers(1, 16, FRAMES)
    gt = [kitti_boxes3d(rng, int(k)) for k in ng]
    src, dt = [], []
    for g, k in zip(gt, nd):
        idx = rng.integers(0, len(g), int(k))
        src.append(idx)
        dt.append(g[idx] + rng.normal(0, 0.3, (int(k), 7)) * [1, 0.1, 1, 0.1, 0.1, 0.1, 0.2])
    assert int(ng.sum()) == 30063 and int(nd.sum()) == 30505, (int(ng.sum()), int(nd.sum()))
    r2 = np.random.default_rng(1)
    names = np.array(["Car", "Car", "Car", "Pedestrian", "Cyclist", "Van", "DontCare"])
    gts, dts = [], []
    for g, d, idx in zip(gt, dt, src):
        n, k = len(g), len(d)
        gname = names[r2.integers(0, len(names), n)]
        z = np.abs(g[:, 2]) + 6.0
        h = 720.0 * g[:, 4] / z
        cx, cy, w = 620.0 + 720.0 * g[:, 0] / z, 190.0 + r2.uniform(-20, 20, n), h * r2.uniform(0.5, 2.2, n)
        gbox = np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], 1)
        gts.append(dict(name=list(gname), truncated=r2.choice([0.0, 0.0, 0.2, 0.4, 0.6], n), occluded=r2.choice([0.0, 0.0, 1.0, 2.0, 3.0], n),
                        alpha=g[:, 6] - np.arctan2(g[:, 0], z), bbox=gbox, dimensions=g[:, 3:6].copy(), location=g[:, 0:3].copy(),
                        rotation_y=g[:, 6].copy(), score=np.zeros(n)))
        dname = np.where(gname[idx] == "DontCare", "Car", gname[idx])
        dts.append(dict(name=list(dname), alpha=d[:, 6] - np.arctan2(d[:, 0], np.abs(d[:, 2]) + 6.0), bbox=gbox[idx] + r2.normal(0, 4.0, (k, 4)),
                        dimensions=d[:, 3:6].copy(), location=d[:, 0:3].copy(), rotation_y=d[:, 6].copy(),
                        score=np.round(r2.uniform(0.05, 1.0, k), 2).clip(0.01, 1.0)))
    return gts, dts, gt, dt


def evaluator(nuscenes):
    iou, dist = tables()
    return D3.Detection3DEvaluator(D3.clean_kitti_data, ID_TO_NAME, iou, dist, coordinate_frame=D3.CoordinateFrame.CAMERA, compute_nuscenes=nuscenes)


def host_ms(fn, reps=REPS, warm=WARM):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def med(v):
    return round(float(np.median(v)), 4)


def count_syncs(fn):
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            fn()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    return sum("synchroniz" in str(x.message).lower() for x in w)


def split(gts, dts, nuscenes):
    """one evaluate call taken apart, each part timed on the host clock around a synchronise (median of REPS)"""
    iou, dist = tables()
    ids = [2, 4, 0]
    parts = {}

    def timed(name, fn):
        vals, res = [], None
        for i in range(WARM + REPS):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = fn()
            torch.cuda.synchronize()
            if i >= WARM:
                vals.append((time.perf_counter() - t0) * 1e3)
        parts[name] = med(vals)
        return res

    P = timed("packing", lambda: DE.pack(gts, dts))
    s = timed("upload", lambda: DE.Session(P, DE.CAMERA))
    flags = timed("filters", lambda: DE.clean_kitti_flags(P, CLASSES, list(DIFFS)))
    dflags = timed("filters_upload", lambda: s.flags(flags))
    metrics = (0, 1, 3 if nuscenes else 2)
    stats = {}
    for m in metrics:
        def ov(m=m):
            s._ov.pop(m, None)
            return s.overlaps(m)
        timed("overlaps_%s" % ("bbox2d", "bev", "box3d", "nu")[m], ov)
        table = dist if m == 3 else iou
        mo = DE.level_thresholds(table[:, :, :, ids], m, 3)
        stats[m] = timed("statistics_%s" % ("bbox2d", "bev", "box3d", "nu")[m], lambda m=m, mo=mo: s.statistics(m, dflags, 9, 2, mo, 41, m in (2, 3)))
    host = timed("read_back", lambda: {m: (v["pr"].cpu().numpy(), v["nthr"].cpu().numpy()) for m, v in stats.items()})
    timed("finish", lambda: [DE.finish(pr, nthr, (3, 3, 2), m == 3, m in (2, 3)) for m, (pr, nthr) in host.items()])
    cells = int((P.gt.num * P.dt.num).sum())
    shape = {("bbox2d", "bev", "box3d", "nu")[m]: {"thresholds_summed_over_combinations": int(nthr.sum()), "pass_b_inner_visits": cells * int(nthr.sum()),
                                                  "active_lanes_per_wave": round(float(nthr.sum()) / (-(-18 * 41 // 256) * 4), 2)}
             for m, (pr, nthr) in host.items()}
    return parts, shape


def overlap_stage(gts, dts, gt, dt, rounds=9):
    """parent's path (dense 3-D IoU per shard from host arrays) and the packed path from host annotations, alternating"""
    sh = shards(FRAMES, SHARDS)
    cuts = np.cumsum([0] + sh)

    def base():
        return [B.box3d_iou(np.concatenate(dt[a:b]), np.concatenate(gt[a:b])) for a, b in zip(cuts[:-1], cuts[1:])]

    def new():
        return DE.Session(DE.pack(gts, dts), DE.CAMERA).overlaps(2)

    for _ in range(WARM):
        base(), new()
    b, n = [], []
    for _ in range(rounds):
        b += host_ms(base, 1, 0)
        n += host_ms(new, 1, 0)
    return {"baseline_box3d_dense_shards_from_host_ms": med(b), "baseline_min_ms": round(min(b), 4), "baseline_max_ms": round(max(b), 4),
            "packed_from_host_annotations_ms": med(n), "packed_min_ms": round(min(n), 4), "packed_max_ms": round(max(n), 4), "rounds": rounds,
            "note": "host clock around a synchronise; the packed path packs every annotation column (names, 2-D boxes, scores, ...) and "
                    "uploads them once for all metrics, the baseline only concatenates [n][7] box arrays"}


def run_calls(frames):
    gts, dts, _, _ = kitti_val_annotations()
    gts, dts = gts[:frames], dts[:frames]
    for nuscenes in (False, True):
        ev = evaluator(nuscenes)
        for _ in range(CALLS):
            ev.evaluate_detection_3d(gts, dts, CLASSES, difficulties=DIFFS)
    torch.cuda.synchronize()
    print("ran %d evaluate calls per setting on %d frames" % (CALLS, frames))


def add_trace(out_dir, rp_dirs):
    p = os.path.join(out_dir, "eval_time.json")
    d = json.load(open(p))
    d["kernel_stats"] = {"source": "rocprofv3 --kernel-trace --stats over `--calls FRAMES`: %d evaluate calls per compute_nuscenes setting, "
                                   "nothing else" % CALLS}
    for frames, rp in zip((3769, 377), rp_dirs):
        hits = sorted(glob.glob(os.path.join(rp, "**", "*kernel_stats.csv"), recursive=True))
        if not hits:
            raise SystemExit("no *kernel_stats.csv under %s" % rp)
        rows = list(csv.DictReader(open(hits[0])))
        calls = 2 * CALLS
        ks = [{"kernel": r["Name"][:90], "launches_per_evaluate": round(int(r["Calls"]) / calls, 2),
               "us_per_evaluate": round(float(r["TotalDurationNs"]) / 1e3 / calls, 1)} for r in rows]
        d["kernel_stats"]["frames_%d" % frames] = {"launches_per_evaluate": round(sum(int(r["Calls"]) for r in rows) / calls, 2),
                                                   "launches_per_eval_metric": round(sum(int(r["Calls"]) for r in rows) / calls / 3, 2),
                                                   "kernel_us_per_evaluate": round(sum(float(r["TotalDurationNs"]) for r in rows) / 1e3 / calls, 1),
                                                   "kernels": ks}
    prk = [k for k in d["kernel_stats"]["frames_3769"]["kernels"] if "eval_pr_kernel" in k["kernel"]]
    if prk:
        visits = np.mean([sum(v["pass_b_inner_visits"] for v in d["frames_3769"][s]["shapes"].values()) for s in ("kitti", "nuscenes")])
        d["pass_b"] = {"inner_visits_per_evaluate": int(visits), "kernel_us_per_evaluate": prk[0]["us_per_evaluate"],
                       "visits_per_s": visits / (prk[0]["us_per_evaluate"] * 1e-6)}
    json.dump(d, open(p, "w"), indent=1)
    print(json.dumps(d["kernel_stats"], indent=1)[:3000])


def main():
    out_dir = sys.argv[1] if len(sys.argv) > 1 else "."
    os.makedirs(out_dir, exist_ok=True)
    if len(sys.argv) > 3 and sys.argv[2] == "--calls":
        return run_calls(int(sys.argv[3]))
    if len(sys.argv) > 4 and sys.argv[2] == "--trace":
        return add_trace(out_dir, sys.argv[3:5])
    gts, dts, gt, dt = kitti_val_annotations()
    res = {"device": torch.cuda.get_device_name(0), "warmup": WARM, "reps": REPS, "classes": CLASSES, "difficulties": list(DIFFS),
           "reference_time": "not measured (numba is not installed here and the reference does not run on this machine)"}
    for frames in (FRAMES, 377):
        g, d = gts[:frames], dts[:frames]
        row = {"gt_boxes": int(sum(len(a["name"]) for a in g)), "dt_boxes": int(sum(len(a["name"]) for a in d))}
        for nuscenes in (False, True):
            ev = evaluator(nuscenes)
            call = lambda: ev.evaluate_detection_3d(g, d, CLASSES, difficulties=DIFFS)  # noqa: E731
            ms = host_ms(call)
            parts, shape = split(g, d, nuscenes)
            row["nuscenes" if nuscenes else "kitti"] = {"evaluate_ms": med(ms), "evaluate_min_ms": round(min(ms), 4), "evaluate_max_ms": round(max(ms), 4),
                                                        "host_synchronisations_per_evaluate": count_syncs(call), "split_ms": parts, "shapes": shape}
        res["frames_%d" % frames] = row
        print(json.dumps(row, indent=1))
    res["overlap_stage"] = overlap_stage(gts, dts, gt, dt)
    print(json.dumps(res["overlap_stage"], indent=1))
    json.dump(res, open(os.path.join(out_dir, "eval_time.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
