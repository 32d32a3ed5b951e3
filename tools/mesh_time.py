"""GPU timing of the mesh extraction (sdflabel_amd/mesh.py) by stage, with device events.

stages      lattice   sdfr_mesh_lattice_inputs + the decoder forward over the lattice (mesh.lattice_sdf)
            inputs    sdfr_mesh_lattice_inputs alone (a second, separate measurement: its share of `lattice`)
            count     sdfr_mesh_count: the per-point records, the in-block prefixes and the scan of the block sums
            emit      sdfr_mesh_emit (after the host read of the totals, which is not inside any timed interval)
            polish    decoder forward with masks, Jacobian and Newton projection at the vertices (mesh.decoder_at)
cases       B = 1 / 16 shapes at R = 32 / 64 / 128 on the synthetic decoder, in its float32 and float16 modes; median of REPS repetitions
            after WARM warm-up runs.
floor       rows x sdfr_decoder_macs x 2 FLOP at the MFMA peak of the selected precision (157.3 TFLOP/s exact f32, 2500 TFLOP/s f16 dense):
            what the lattice forward cannot beat.
launches    kernel launches, copies and host synchronisations of one meshes_many call (torch.profiler, torch's sync debug mode).

usage: python tools/mesh_time.py OUT_DIR          (writes OUT_DIR/mesh_time.json)
"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import sdflabel_amd  # noqa: E402
from sdflabel_amd import _lib  # noqa: E402
from sdflabel_amd import mesh as M  # noqa: E402
from sdflabel_amd.fixtures import ASSET  # noqa: E402
from tools.frame_time import count_launches, count_syncs  # noqa: E402

DEV = "cuda:0"
WARM, REPS = 2, 7
PEAK_TFLOPS = {"float32": 157.3, "float16": 2500.0}


def latents(B):
    rng = np.random.default_rng(200 + B)
    lat = rng.normal(size=(B, 3))
    return torch.from_numpy((lat / np.linalg.norm(lat, axis=1, keepdims=True) * rng.uniform(0.8, 1.1, (B, 1))).astype(np.float32)).to(DEV)


def staged(dec, lat, R):
    """one extraction with an event at every stage boundary; returns the stage times in ms and the counts"""
    L = _lib.lib()
    B, Ld = int(lat.shape[0]), int(lat.shape[1])
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(8)]
    st = _lib.stream_ptr()
    P = _lib.ptr
    scratch = torch.empty((min(B * R ** 3, M.STAGING_BYTES // (4 * (Ld + 3))), Ld + 3), device=DEV)
    ev[0].record()
    sdf = M.lattice_sdf(dec, lat, R)
    ev[1].record()
    nb = int(L.sdfr_mesh_ws_bytes(R, B))
    ws = torch.empty((nb,), dtype=torch.uint8, device=DEV)
    cnt = torch.empty((2, B), dtype=torch.int32, device=DEV)
    ev[2].record()
    _lib.check(L.sdfr_mesh_count(P(sdf), R, B, P(cnt[0]), P(cnt[1]), P(ws), nb, st), "sdfr_mesh_count")
    ev[3].record()
    host = cnt.cpu().numpy().astype(np.int64)
    voff, toff = np.concatenate([[0], np.cumsum(host[0])]), np.concatenate([[0], np.cumsum(host[1])])
    V, T = int(voff[-1]), int(toff[-1])
    verts = torch.empty((V, 3), device=DEV)
    faces = torch.empty((T, 3), dtype=torch.int32, device=DEV)
    ev[4].record()
    _lib.check(L.sdfr_mesh_emit(P(sdf), R, B, voff.ctypes.data, toff.ctypes.data, P(ws), nb, P(verts), V, P(faces), T, st), "sdfr_mesh_emit")
    ev[5].record()
    shape_of = torch.repeat_interleave(torch.arange(B, device=DEV), torch.as_tensor(np.diff(voff), device=DEV))
    M.decoder_at(dec, lat, shape_of, verts)
    ev[6].record()
    rows = min(int(scratch.shape[0]), R ** 3)
    _lib.check(L.sdfr_mesh_lattice_inputs(P(lat), Ld, R, 1, 0, rows, P(scratch), st), "sdfr_mesh_lattice_inputs")
    ev[7].record()
    torch.cuda.synchronize()
    t = {"lattice": ev[0].elapsed_time(ev[1]), "count": ev[2].elapsed_time(ev[3]), "emit": ev[4].elapsed_time(ev[5]),
         "polish": ev[5].elapsed_time(ev[6]), "inputs": ev[6].elapsed_time(ev[7]) * (B * R ** 3 / rows)}
    return t, V, T


def main():
    out_dir = sys.argv[1] if len(sys.argv) > 1 else "."
    os.makedirs(out_dir, exist_ok=True)
    res = {"config": "deepsdf_synth (8 x 512, latent 3); device events on the current stream; WARM %d, REPS %d, medians; `inputs` is one "
                     "shape's launch scaled to the batch" % (WARM, REPS), "cases": {}}
    for prec, name in ((torch.float32, "float32"), (torch.float16, "float16")):
        dec = sdflabel_amd.setup_dsdf(ASSET + ".pt", precision=prec)[0].to(DEV)
        macs = int(_lib.lib().sdfr_decoder_macs(dec.handle(torch.device(DEV)).h))
        for R in (32, 64, 128):
            for B in (1, 16):
                lat = latents(B)
                runs = [staged(dec, lat, R) for _ in range(WARM + REPS)][WARM:]
                med = {k: float(np.median([r[0][k] for r in runs])) for k in runs[0][0]}
                V, T = runs[0][1], runs[0][2]
                rows = B * R ** 3
                floor = 2.0 * macs * rows / (PEAK_TFLOPS[name] * 1e12) * 1e3
                whole = med["lattice"] + med["count"] + med["emit"] + med["polish"]
                new = med["inputs"] + med["count"] + med["emit"]
                call = lambda: M.meshes_many(dec, lat, resolution=R)          # noqa: E731
                k, c = count_launches(call)
                entry = {"stage_ms": {a: round(b, 4) for a, b in med.items()}, "vertices": V, "triangles": T, "lattice_rows": rows,
                         "lattice_forward_floor_ms": round(floor, 4), "lattice_over_floor": round(med["lattice"] / floor, 2),
                         "share_of_the_three_new_kernels": round(new / whole, 4), "kernel_launches": k, "copies": c,
                         "host_synchronisations": count_syncs(call)}
                res["cases"]["%s_R%d_B%d" % (name, R, B)] = entry
                print("%s R=%d B=%d" % (name, R, B), json.dumps(entry), flush=True)
    json.dump(res, open(os.path.join(out_dir, "mesh_time.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
