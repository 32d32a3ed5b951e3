"""GPU timing of the evaluator's box overlaps (sdflabel_amd.box_iou, csrc/box_iou.hip).

  dense     rotate_iou and box3d_iou (camera frame) of N x N KITTI-scale boxes (cars 1.5-5 m, positions +-40 m, all angles), N = 1k, 4k;
            inputs already on the device, timed with device events around the call (output allocation + one launch)
  frames    a KITTI-val-shaped frame list (3 769 frames, 1-15 ground-truth and 1-15 detected boxes each):
              *_frames_from_host         grouped mode from host frame lists (one upload per side, one launch, per-frame views)
              box3d_dense_shards_from_host   the evaluator's way: 50 shards (detection_3d.py:362, get_shards), each concatenated on the
                                         host and computed as one dense matrix
              box3d_dense_shards_on_device   the same shard matrices with inputs already on the device
Every figure is the median of REPS calls after WARM warm-up calls; ms_device spans the whole call (host work included) between device
events.  The kernel is VALU-bound (20 B in per box, 4 B out per pair), so the figures are pairs/s, not bandwidth.

Kernel time comes from a separate profiled run of the same launch sequence:
  rocprofv3 --kernel-trace --stats -d RP_DIR -o iou --output-format csv -- python tools/iou_time.py RUN_DIR
  python tools/iou_time.py OUT_DIR --trace RP_DIR
adds kernel_stats, kernel_trace (kernel time per phase) and frames.kernel_only to OUT_DIR/iou_time.json.

usage: python tools/iou_time.py OUT_DIR
       python tools/iou_time.py OUT_DIR --trace RP_DIR
"""
import csv
import glob
import json
import os
import re
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from sdflabel_amd import box_iou as B  # noqa: E402

WARM, REPS = 3, 10
FRAMES, SHARDS = 3769, 50


def kitti_boxes3d(rng, n):
    b = np.empty((n, 7), np.float64)
    b[:, 0] = rng.uniform(-40, 40, n)
    b[:, 1] = rng.uniform(1.2, 2.2, n)
    b[:, 2] = rng.uniform(-40, 40, n)
    b[:, 3] = rng.uniform(1.5, 5.0, n)
    b[:, 4] = rng.uniform(1.3, 1.9, n)
    b[:, 5] = rng.uniform(1.5, 5.0, n)
    b[:, 6] = rng.uniform(-np.pi, np.pi, n)
    return b


def timed(fn):
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    ms, host = [], []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        host.append((time.perf_counter() - t0) * 1e3)
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), float(np.median(host))


def shards(num, num_shards):
    per, rem = num // num_shards, num % num_shards
    return [per] * (num_shards * (per > 0)) + ([rem] if rem else [])


KINDS = {0: "rotate_iou", 1: "box3d_iou", 2: "image_box_iou"}      # iou_kernel<KIND, ...> of csrc/box_iou.hip


def _kind(name):
    m = re.search(r"iou_kernel<(\d+)", name)
    return KINDS[int(m.group(1))] if m else None


def add_trace(out_dir, rp_dir):
    """Merge a rocprofv3 --kernel-trace --stats run of this tool (CSV output under rp_dir) into OUT_DIR/iou_time.json: the per-kernel
    totals (kernel_stats) and, by walking the dispatches in launch order along the tool's own launch_sequence, each phase's kernel
    time (kernel_trace) and the grouped-versus-shards kernel comparison (frames.kernel_only)."""
    def find(suffix):
        hits = sorted(glob.glob(os.path.join(rp_dir, "**", "*" + suffix), recursive=True))
        if not hits:
            raise SystemExit("no *%s under %s" % (suffix, rp_dir))
        return hits[0]
    p = os.path.join(out_dir, "iou_time.json")
    d = json.load(open(p))
    stats = [r for r in csv.DictReader(open(find("kernel_stats.csv"))) if _kind(r["Name"])]
    tot = sum(float(r["TotalDurationNs"]) for r in stats)
    d["kernel_stats"] = {
        "source": "rocprofv3 --kernel-trace --stats over one run of this tool (warm-up included)",
        "iou_kernels": [{"kernel": _kind(r["Name"]), "calls": int(r["Calls"]), "total_us": round(float(r["TotalDurationNs"]) / 1e3, 1),
                         "avg_us": round(float(r["AverageNs"]) / 1e3, 2), "share_of_all_kernels_pct": round(float(r["Percentage"]), 2),
                         "share_of_iou_kernels_pct": round(100.0 * float(r["TotalDurationNs"]) / tot, 1)} for r in stats]}
    rows = [r for r in csv.DictReader(open(find("kernel_trace.csv"))) if _kind(r["Kernel_Name"])]
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))
    seq = d["launch_sequence"]
    if len(rows) != sum(ph["dispatches"] for ph in seq):
        raise SystemExit("trace holds %d box-IoU dispatches, the launch sequence %d" % (len(rows), sum(ph["dispatches"] for ph in seq)))
    phases, at = [], 0
    for ph in seq:
        part, at = rows[at:at + ph["dispatches"]], at + ph["dispatches"]
        if any(_kind(r["Kernel_Name"]) != ph["kernel"] for r in part):
            raise SystemExit("phase %s: dispatches of another kernel" % ph["phase"])
        us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in part]
        calls = ph["calls"]
        phases.append({"phase": ph["phase"], "kernel": ph["kernel"], "dispatches": len(part), "calls": calls,
                       "workgroups": sorted({int(r["Grid_Size_X"]) // int(r["Workgroup_Size_X"]) for r in part}),
                       "median_dispatch_us": round(float(np.median(us)), 1), "kernel_us_per_call": round(sum(us) / calls, 1)})
    d["kernel_trace"] = {"source": "rocprofv3 --kernel-trace over one run of this tool; dispatches assigned to phases in launch order",
                         "phases": phases}
    by = {ph["phase"]: ph for ph in phases}
    g, sh = by["box3d_frames_from_host"], by["box3d_dense_shards_on_device"]
    d["frames"]["kernel_only"] = {"box3d_grouped_us_per_call": g["kernel_us_per_call"], "box3d_dense_shards_us_per_pass": sh["kernel_us_per_call"],
                                  "note": "kernel time only; the grouped launch evaluates pairs_in_frames pairs, the shard matrices "
                                          "box3d_dense_shards_on_device.pairs"}
    json.dump(d, open(p, "w"), indent=1)
    for ph in phases:
        print(ph)
    print(d["frames"]["kernel_only"])


def main():
    out_dir = sys.argv[1] if len(sys.argv) > 1 else "."
    os.makedirs(out_dir, exist_ok=True)
    if len(sys.argv) > 3 and sys.argv[2] == "--trace":
        add_trace(out_dir, sys.argv[3])
        return
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    res = {"device": torch.cuda.get_device_name(0), "warmup": WARM, "reps": REPS, "dense": [], "frames": {}, "launch_sequence": [],
           "not_measured": ["image_box_iou"]}
    seq = res["launch_sequence"]
    for n in (1024, 4096):
        b3 = torch.from_numpy(kitti_boxes3d(rng, n)).to(dev)
        q3 = torch.from_numpy(kitti_boxes3d(rng, n)).to(dev)
        bev_b = b3[:, [0, 2, 3, 5, 6]].float().contiguous()
        bev_q = q3[:, [0, 2, 3, 5, 6]].float().contiguous()
        for name, fn in (("rotate_iou", lambda: B.rotate_iou(bev_b, bev_q)), ("box3d_iou", lambda: B.box3d_iou(b3, q3))):
            ms, host = timed(fn)
            row = {"op": name, "N": n, "K": n, "ms_device": round(ms, 4), "ms_host": round(host, 4), "pairs_per_s": n * n / (ms * 1e-3),
                   "overlapping_pairs": int((fn() > 0).sum().item())}
            seq.append({"phase": "%s_dense_%d" % (name, n), "kernel": name, "dispatches": WARM + REPS + 1, "calls": WARM + REPS + 1})
            res["dense"].append(row)
            print(row)
    # KITTI-val-shaped frame list
    ng = rng.integers(1, 16, FRAMES)
    nd = rng.integers(1, 16, FRAMES)
    gt = [kitti_boxes3d(rng, int(k)) for k in ng]
    dt = [g[rng.integers(0, len(g), int(k))] + rng.normal(0, 0.3, (int(k), 7)) * [1, 0.1, 1, 0.1, 0.1, 0.1, 0.2] for g, k in zip(gt, nd)]
    pairs_frames = int((ng * nd).sum())
    fr = {"frames": FRAMES, "gt_boxes": int(ng.sum()), "dt_boxes": int(nd.sum()), "pairs_in_frames": pairs_frames}

    def record(key, phase_kernel, fn, launches, pairs, **extra):
        ms, host = timed(fn)
        fr[key] = dict(extra, pairs=pairs, ms_device=round(ms, 4), ms_host=round(host, 4), pairs_per_s=pairs / (ms * 1e-3))
        seq.append({"phase": key, "kernel": phase_kernel, "dispatches": (WARM + REPS) * launches, "calls": WARM + REPS})

    # end to end from host frame lists: one upload per side, one launch, per-frame views (no read-back)
    record("box3d_frames_from_host", "box3d_iou", lambda: B.box3d_iou_frames(dt, gt), 1, pairs_frames)
    dtb = [d[:, [0, 2, 3, 5, 6]] for d in dt]
    gtb = [g[:, [0, 2, 3, 5, 6]] for g in gt]
    record("rotate_frames_from_host", "rotate_iou", lambda: B.rotate_iou_frames(dtb, gtb), 1, pairs_frames)
    # the evaluator's way (detection_3d.py:550-632): per shard, concatenate its frames on the host and compute the dense matrix
    sh = shards(FRAMES, SHARDS)
    cuts = np.cumsum([0] + sh)
    pairs_shards = int(sum(nd[a:b].sum() * ng[a:b].sum() for a, b in zip(cuts[:-1], cuts[1:])))
    record("box3d_dense_shards_from_host", "box3d_iou",
           lambda: [B.box3d_iou(np.concatenate(dt[a:b]), np.concatenate(gt[a:b])) for a, b in zip(cuts[:-1], cuts[1:])], len(sh),
           pairs_shards, shards=len(sh))
    sb = [torch.from_numpy(np.concatenate(dt[a:b])).to(dev) for a, b in zip(cuts[:-1], cuts[1:])]
    sq = [torch.from_numpy(np.concatenate(gt[a:b])).to(dev) for a, b in zip(cuts[:-1], cuts[1:])]
    record("box3d_dense_shards_on_device", "box3d_iou", lambda: [B.box3d_iou(b, q) for b, q in zip(sb, sq)], len(sh), pairs_shards,
           shards=len(sh))
    res["frames"] = fr
    print(json.dumps(fr, indent=1))
    json.dump(res, open(os.path.join(out_dir, "iou_time.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
