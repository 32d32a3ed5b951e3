"""GPU timing of the RANSAC pose initialisation (PoseEstimator.estimate_many): frames of 1 / 8 / 16 / 64 annotations at N = 300 / 1000 /
3000 scene points, M ~ 2 700 model points (the fixture decoder's Grid3D(40) surface), kabsch, both samplers, after two warm-up calls.

Each frame is timed from call to returned dicts (the call ends in its one host wait) twice over: device events recorded on the current
stream before and after the call (`ms_call_to_dicts`, the median of the repetitions), and the host clock around the same call
(`ms_host_clock`).  Pair evaluations/s = sum over crops of (scored hypotheses x N x M) / time; the share of the float32 vector peak
(157.3 TFLOP/s) counts 9 float32 operations per pair evaluation and is an end-to-end figure, not the scoring kernel's.

The kernel split comes from a separate profiled run of this tool (rocprofv3 --kernel-trace writes a database); `--kernel-trace DB` reads
that database on the host and adds its per-kernel totals to OUT_DIR/pose_time.json as `kernel_trace`.

usage: python tools/pose_time.py OUT_DIR
       python tools/pose_time.py OUT_DIR --kernel-trace PATH/TO/results.db
"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import sdflabel_amd  # noqa: E402
from sdflabel_amd.fixtures import ASSET  # noqa: E402
from sdflabel_amd.pipelines.pose import PoseEstimator  # noqa: E402

PEAK_F32 = 157.3e12
OPS_PER_PAIR = 9


def model_cloud(dev):
    dec, _ = sdflabel_amd.setup_dsdf(ASSET + ".pt", precision=torch.float32)
    dec = dec.to(dev)
    grid = sdflabel_amd.Grid3D(40, dev)
    lat = torch.nn.functional.normalize(torch.tensor([0.3, -0.5, 0.8], device=dev), p=2, dim=0)
    with torch.no_grad():
        sdf, _ = dec(torch.cat([lat.expand(grid.points.size(0), -1), grid.points], 1))
    pts, nocs, _ = grid.get_surface_points(sdf)
    return pts.detach().float(), nocs.detach().float()


def frame(m, mc, B, n, rng, dev):
    mh, mch = m.cpu().numpy(), mc.cpu().numpy()
    items = []
    for _ in range(B):
        yaw = rng.uniform(-np.pi, np.pi)
        c, s = np.cos(yaw), np.sin(yaw)
        R = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
        n_in = n - n // 2
        sel = rng.choice(mh.shape[0], n_in)
        p = (R @ (2.0 * mh[sel].astype(np.float64)).T).T + np.array([0.2, 0.1, 8.0]) + rng.normal(0, 0.005, (n_in, 3))
        col = mch[sel] + rng.normal(0, 0.01, (n_in, 3))
        po = rng.uniform(p.min(0) - 0.5, p.max(0) + 0.5, (n // 2, 3))
        co = rng.uniform(0, 1, (n // 2, 3))
        items.append((m, mc, torch.from_numpy(np.concatenate([p, po]).astype(np.float32)).to(dev),
                      torch.from_numpy(np.concatenate([col, co]).astype(np.float32)).to(dev)))
    return items


def add_kernel_trace(out_dir, db):
    """per-kernel totals of the RANSAC kernels from a rocprofv3 --kernel-trace database, merged into OUT_DIR/pose_time.json"""
    import re
    import sqlite3
    rows = sqlite3.connect(db).execute("select name, count(*), sum(duration) from kernels where name like '%::rs_%' group by name "
                                       "order by sum(duration) desc").fetchall()
    tot = sum(r[2] for r in rows)
    ks = [{"kernel": re.search(r"::(rs_[a-z0-9_]+)", n).group(1), "calls": k, "total_us": round(d / 1e3, 1),
           "share_of_ransac_kernels": round(d / tot, 4)} for n, k, d in rows]
    path = os.path.join(out_dir, "pose_time.json")
    d = json.load(open(path))
    d["kernel_trace"] = {"source": "rocprofv3 --kernel-trace over one run of this tool (all frames, warm-up included)", "ransac_kernels": ks}
    json.dump(d, open(path, "w"), indent=1)
    for k in ks:
        print(k)


def main():
    out_dir = sys.argv[1] if len(sys.argv) > 1 else "."
    os.makedirs(out_dir, exist_ok=True)
    if len(sys.argv) > 3 and sys.argv[2] == "--kernel-trace":
        add_kernel_trace(out_dir, sys.argv[3])
        return
    dev = "cuda:0"
    m, mc = model_cloud(dev)
    pe = PoseEstimator(type="kabsch", scale=2.0)
    rows = []
    for sampler in ("device", "numpy"):
        for n in (300, 1000, 3000):
            for B in (1, 8, 16, 64):
                items = frame(m, mc, B, n, np.random.default_rng(B * 7 + n), dev)
                for _ in range(2):
                    pe.estimate_many(items, sampler=sampler, seed=1)
                torch.cuda.synchronize()
                reps, ts, hs = (5 if sampler == "device" else 3), [], []
                for _ in range(reps):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0 = time.perf_counter()
                    e0.record()
                    res, raw = pe.estimate_many(items, sampler=sampler, seed=1, return_raw=True)
                    e1.record()
                    hs.append(time.perf_counter() - t0)
                    e1.synchronize()
                    ts.append(e0.elapsed_time(e1) * 1e-3)
                scored = int(((raw["gate"] & 2) != 0).sum().item())
                pairs = scored * n * m.shape[0]
                t = float(np.median(ts))
                rows.append({"sampler": sampler, "B": B, "N": n, "M": int(m.shape[0]), "ms_call_to_dicts": t * 1e3,
                             "ms_host_clock": float(np.median(hs)) * 1e3, "ms_per_annotation": t * 1e3 / B, "found": int(sum(r is not None for r in res)), "scored_hypotheses": scored,
                             "pair_evals_per_s": pairs / t, "f32_vector_peak_share_end_to_end": pairs * OPS_PER_PAIR / t / PEAK_F32})
                print(json.dumps(rows[-1]))
    json.dump({"model_points": int(m.shape[0]), "rows": rows, "ops_per_pair": OPS_PER_PAIR, "peak_f32_vector": PEAK_F32,
               "timing": "ms_call_to_dicts: device events around the call (median); ms_host_clock: host clock around the same call"},
              open(os.path.join(out_dir, "pose_time.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
