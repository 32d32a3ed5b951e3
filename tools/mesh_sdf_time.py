"""GPU timing of the signed distance to meshes and of the SDF training samples (sdflabel_amd/sdf_samples.py), with device events.

mesh        the synthetic decoder's shape meshed at R = 64 (about 50 000 triangles), in the lattice frame
stages      mesh_sdf            sdfr_mesh_sdf at 250 000 uniform points, want_sign = 1 (distance and winding number)
            mesh_sdf_unsigned   the same with want_sign = 0 (no winding pass)
            mesh_sdf_few        8 points: the chunk-split launch shape
            surface_points      sdfr_mesh_surface_points, 250 000 samples
whole       one draw_sdf_samples call at its default 500 000 samples, host clock round the call (it reads nothing back)
cpu         the same arithmetic on this machine's CPU for a tenth of the points: csrc/mesh_sdf_cells.h compiled for the host
            (tests/mesh_sdf_host, -O2 -ffp-contract=off), the points split over CPU_PROCS processes, wall clock; checked against the device bit
            for bit (sdf, nearest)
Medians of REPS repetitions after WARM warm-up runs.

usage: python tools/mesh_sdf_time.py OUT_DIR          (writes OUT_DIR/mesh_sdf_time.json)
"""
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import sdflabel_amd  # noqa: E402
from sdflabel_amd import mesh as M  # noqa: E402
from sdflabel_amd import sdf_samples as S  # noqa: E402
from sdflabel_amd.fixtures import ASSET, GT_LATENT  # noqa: E402

DEV = "cuda:0"
WARM, REPS = 1, 5
NPTS, NSURF, NDRAW = 250000, 250000, 500000
CPU_PROCS = 16
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


def event_ms(fn, reps=REPS):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    vals = []
    for _ in range(WARM + reps):
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        vals.append(a.elapsed_time(b))
    return float(np.median(vals[WARM:]))


def host_ms(fn, reps=3):
    vals = []
    for _ in range(WARM + reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        vals.append((time.perf_counter() - t) * 1e3)
    return float(np.median(vals[WARM:]))


def cpu_baseline(v, f, pts, tmp):
    """wall seconds of the host build of the header over `pts`, CPU_PROCS processes; returns (seconds, sdf, nearest)"""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        return None, None, None
    exe = os.path.join(tmp, "mesh_sdf_host")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(ROOT, "sdflabel_amd", "csrc"),
                           os.path.join(ROOT, "tests", "mesh_sdf_host", "mesh_sdf_host.cpp"), "-o", exe])
    parts = np.array_split(pts, CPU_PROCS)
    for i, p in enumerate(parts):
        with open(os.path.join(tmp, "in%d.bin" % i), "wb") as fh:
            fh.write(np.array([1, 1], np.int32).tobytes() + np.array([len(v), len(f), len(p), 0], np.int64).tobytes())
            for a in (np.array([0, len(v)], np.int64), np.array([0, len(f)], np.int64), np.array([0, len(p)], np.int64), np.array([0, 0], np.int64),
                      v, f, p):
                fh.write(np.ascontiguousarray(a).tobytes())
    t = time.perf_counter()
    procs = [subprocess.Popen([exe, os.path.join(tmp, "in%d.bin" % i), os.path.join(tmp, "out%d.bin" % i)]) for i in range(CPU_PROCS)]
    rc = [p.wait() for p in procs]
    secs = time.perf_counter() - t
    assert not any(rc), rc
    sdf, nearest = [], []
    for i, p in enumerate(parts):
        raw, n = open(os.path.join(tmp, "out%d.bin" % i), "rb").read(), len(p)
        sdf.append(np.frombuffer(raw, np.float32, n, 0))
        nearest.append(np.frombuffer(raw, np.int32, n, 16 * n))
    return secs, np.concatenate(sdf), np.concatenate(nearest)


def main():
    out_dir = sys.argv[1] if len(sys.argv) > 1 else "."
    os.makedirs(out_dir, exist_ok=True)
    dec = sdflabel_amd.setup_dsdf(ASSET + ".pt", precision=torch.float32)[0].to(DEV)
    (m,) = M.meshes_many(dec, [torch.tensor(GT_LATENT)], resolution=64)
    mb = S.MeshBatch([m])
    rng = np.random.default_rng(1)
    pts = torch.from_numpy(rng.uniform(-1, 1, (NPTS, 3)).astype(np.float32)).to(DEV)
    few = pts[:8].contiguous()
    g = torch.Generator().manual_seed(3)
    res = {"config": "deepsdf_synth's shape at R = 64: %d vertices, %d triangles; %d query points uniform in the cube; device events on the "
                     "current stream (host clock for draw_sdf_samples and the CPU); WARM %d, REPS %d, medians" % (mb.V, mb.T, NPTS, WARM, REPS)}
    stage = {
        "mesh_sdf": event_ms(lambda: S.mesh_sdf_many(mb, [pts])),
        "mesh_sdf_unsigned": event_ms(lambda: S.mesh_sdf_many(mb, [pts], want_sign=False)),
        "mesh_sdf_few": event_ms(lambda: S.mesh_sdf_many(mb, [few])),
        "surface_points": event_ms(lambda: S.surface_points_many(mb, [NSURF], g)),
    }
    res["stage_ms"] = {k: round(x, 4) for k, x in stage.items()}
    pairs = float(NPTS) * mb.T
    res["pairs_per_s"] = {"mesh_sdf": round(pairs / stage["mesh_sdf"] * 1e3, 0), "mesh_sdf_unsigned": round(pairs / stage["mesh_sdf_unsigned"] * 1e3, 0)}
    print(json.dumps(res), flush=True)
    res["draw_sdf_samples_ms"] = round(host_ms(lambda: S.draw_sdf_samples(mb, n=NDRAW, generator=g)), 3)
    print("draw_sdf_samples", res["draw_sdf_samples_ms"], flush=True)
    out = S.mesh_sdf_many(mb, [pts], return_nearest=True)
    n10 = NPTS // 10
    with tempfile.TemporaryDirectory() as tmp:
        secs, sdf, nearest = cpu_baseline(m.vertices_numpy(), m.faces_numpy(), pts[:n10].cpu().numpy(), tmp)
    if secs is not None:
        res["cpu"] = {"points": n10, "processes": CPU_PROCS, "seconds": round(secs, 2), "pairs_per_s": round(n10 * mb.T / secs, 0),
                      "agrees_bit_for_bit": bool(sdf.tobytes() == out.sdf[:n10].cpu().numpy().tobytes()
                                                 and nearest.tobytes() == out.nearest[:n10].cpu().numpy().tobytes())}
    print(json.dumps(res), flush=True)
    json.dump(res, open(os.path.join(out_dir, "mesh_sdf_time.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
