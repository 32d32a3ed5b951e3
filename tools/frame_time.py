"""GPU timing of the frame-labelling stages: labels_many and reproject_many for frames of 1, 8 and 16 annotations.

labels      the frame's labels through frame.labels_many (one decoder / band / surface pass over all latents, one read-back) against the same
            labels produced one annotation at a time through the public modules that existed before it: the decoder call,
            Grid3D.get_surface_points, `.cpu().numpy()` of the points and numpy min / max, then the same host label arithmetic.  Both in the
            decoder's float16 mode at Grid3D(40), the shipped configuration.  The two are timed alternately in the same run (host clock around
            the call; both end in a device -> host copy), median and spread of REPS repetitions after WARM warm-up calls.
reproject   frame.reproject_many on crops of a KITTI-like size (one launch sequence, one read of the counts) against one call per crop.
launches    kernel launches per call, counted with torch.profiler; synchronisations per call, counted with torch's sync debug mode.

usage: python tools/frame_time.py OUT_DIR          (writes OUT_DIR/frame_time.json)
"""
import json
import os
import sys
import time
import warnings

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import sdflabel_amd  # noqa: E402
from sdflabel_amd import frame as FR  # noqa: E402
from sdflabel_amd.fixtures import ASSET  # noqa: E402

DEV = "cuda:0"
WARM, REPS = 3, 15


def count_syncs(fn):
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            fn()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    return sum("synchroniz" in str(x.message).lower() for x in w)


def count_launches(fn):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    kernels = [e for e in prof.events() if str(e.device_type).endswith("CUDA") and "memcpy" not in e.name.lower() and "memset" not in e.name.lower()]
    copies = [e for e in prof.events() if str(e.device_type).endswith("CUDA") and "memcpy" in e.name.lower()]
    return len(kernels), len(copies)


def alternate(a, b):
    for _ in range(WARM):
        a(), b()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(REPS):
        for fn, ts in ((a, ta), (b, tb)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
    stat = lambda v: {"median_ms": round(float(np.median(v)), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}      # noqa: E731
    return stat(ta), stat(tb)


def params(B, rng):
    out = []
    for _ in range(B):
        lat = rng.normal(size=3)
        lat = (lat / np.linalg.norm(lat) * rng.uniform(0.8, 1.2)).astype(np.float32)
        out.append({"latent": torch.from_numpy(lat).to(DEV), "scale": torch.tensor([rng.uniform(1.6, 2.4)], dtype=torch.float32, device=DEV),
                    "trans": torch.tensor([rng.uniform(-3, 3), 0.6, rng.uniform(4, 20)], dtype=torch.float32, device=DEV),
                    "yaw": torch.tensor([rng.uniform(-3, 3)], dtype=torch.float32, device=DEV)})
    return out


def labels_loop(dec, grid, ps, p_WC, bboxes):
    """one annotation at a time through the decoder call, Grid3D.get_surface_points and .cpu().numpy() min / max"""
    prec = grid.points.dtype
    out = []
    for p, bbox in zip(ps, bboxes):
        lat = p["latent"].to(prec)
        sdf, _ = dec(torch.cat([lat.expand(grid.points.size(0), -1), grid.points], 1))
        pts, _, _ = grid.get_surface_points(sdf)
        scale = p["scale"].to(prec).detach().cpu().numpy()
        sp = pts.detach().cpu().numpy() * scale[None]
        ext = np.array([[sp[:, 0].min(), sp[:, 0].max(), sp[:, 1].min(), sp[:, 1].max(), sp[:, 2].min(), sp[:, 2].max()]])
        lab, cam_T = FR.assemble_labels(ext, p["yaw"].to(prec).detach().cpu().numpy(), p["trans"].to(prec).detach().cpu().numpy()[None], scale, p_WC, [bbox])
        out.append((lab[0], sp, cam_T[0]))
    return out


def crops(B, rng):
    cs, ds, Ks = [], [], []
    for _ in range(B):
        W = int(rng.integers(60, 420))
        H = max(24, int(W / rng.uniform(1.2, 3.2)))
        d = np.zeros((H, W), np.float32)
        m = rng.random((H, W)) < 0.08
        d[m] = rng.uniform(4, 40, int(m.sum())).astype(np.float32)
        c = rng.random((3, H, W)).astype(np.float32)
        c[:, rng.random((H, W)) < 0.4] = 0
        cs.append(torch.from_numpy(c)), ds.append(torch.from_numpy(d))
        Ks.append(torch.tensor([[721.5, 0, 609.5 - rng.uniform(0, 1000)], [0, 721.5, 172.8 - rng.uniform(100, 250)], [0, 0, 1]], dtype=torch.float32))
    return cs, ds, Ks


def main():
    out_dir = sys.argv[1] if len(sys.argv) > 1 else "."
    os.makedirs(out_dir, exist_ok=True)
    dec = sdflabel_amd.setup_dsdf(ASSET + ".pt", precision=torch.float16)[0].to(DEV)
    grid = sdflabel_amd.Grid3D(40, DEV, torch.float16)
    p_WC = np.eye(4)
    p_WC[:3, 3] = [0.4, -1.1, 0.7]
    res = {"config": "deepsdf_synth, float16 decoder and grid, Grid3D(40); host clock around calls that end in a device -> host copy; "
                     "WARM %d, REPS %d, batched and loop alternating in the same run" % (WARM, REPS), "labels": {}, "reproject": {}}
    for B in (1, 8, 16):
        rng = np.random.default_rng(100 + B)
        ps = params(B, rng)
        bboxes = [[0, 0, 100, 60]] * B
        many = lambda: FR.labels_many(dec, grid, ps, p_WC, bboxes)      # noqa: E731
        loop = lambda: labels_loop(dec, grid, ps, p_WC, bboxes)         # noqa: E731
        a, b = many(), loop()
        worst = max(np.abs(x[0]["location"] - y[0]["location"]).max() for x, y in zip(a, b))
        tm, tl = alternate(many, loop)
        km, cm = count_launches(many)
        kl, cl = count_launches(loop)
        res["labels"]["B%d" % B] = {"labels_many": dict(tm, kernel_launches=km, copies=cm, host_synchronisations=count_syncs(many)),
                                    "one_annotation_at_a_time": dict(tl, kernel_launches=kl, copies=cl, host_synchronisations=count_syncs(loop)),
                                    "largest_location_difference_between_the_two": float(worst),
                                    "band_rows_per_annotation": [len(x[1]) for x in a]}
        print("labels B=%d" % B, json.dumps(res["labels"]["B%d" % B]))
        cs, ds, Ks = crops(B, rng)
        many = lambda: FR.reproject_many(cs, ds, Ks, filter=True)                                       # noqa: E731
        loop = lambda: [FR.reproject_many([c], [d], [k], filter=True) for c, d, k in zip(cs, ds, Ks)]   # noqa: E731
        tm, tl = alternate(many, loop)
        km, cm = count_launches(many)
        kl, cl = count_launches(loop)
        res["reproject"]["B%d" % B] = {"reproject_many": dict(tm, kernel_launches=km, copies=cm, host_synchronisations=count_syncs(many)),
                                       "one_crop_per_call": dict(tl, kernel_launches=kl, copies=cl, host_synchronisations=count_syncs(loop)),
                                       "pixels": int(sum(d.numel() for d in ds)), "points": int(sum(p.shape[0] for p, _ in many()))}
        print("reproject B=%d" % B, json.dumps(res["reproject"]["B%d" % B]))
    json.dump(res, open(os.path.join(out_dir, "frame_time.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
