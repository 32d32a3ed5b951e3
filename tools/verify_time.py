"""GPU timing of the autolabel verification (sdflabel_amd/verify.py) by stage, with device events.

stages      raster        sdfr_mesh_raster: the init, raster and resolve launches
            mask_counts   sdfr_verify_mask_counts
            point_rows    sdfr_verify_point_rows over all points
            decoder       the decoder forward at those rows (an existing kernel; here for scale)
            band_counts   sdfr_verify_band_counts
whole       one verify_many call, host clock round the call (it ends with its one host read), and beside it what meshes_many adds at R = 64
cases       B = 1 / 16 annotations: shapes of the synthetic decoder in its float16 mode, meshed at R = 64, 3 - 30 m in front of a KITTI-sized
            camera (1242 x 375, f = 720), each with its projected box as the label and 1500 lidar-like points on its surface
numpy       the restatement tests/_verify_ref.py on this machine's CPU for the B = 1 case (one run)
Medians of REPS repetitions after WARM warm-up runs.

usage: python tools/verify_time.py OUT_DIR          (writes OUT_DIR/verify_time.json)
"""
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import sdflabel_amd  # noqa: E402
from sdflabel_amd import _lib  # noqa: E402
from sdflabel_amd import mesh as M  # noqa: E402
from sdflabel_amd import verify as V  # noqa: E402
from sdflabel_amd.fixtures import ASSET  # noqa: E402
from tests import _verify_ref as VR  # noqa: E402
from tools.frame_time import count_launches, count_syncs  # noqa: E402

DEV = "cuda:0"
WARM, REPS = 3, 9
W, H, F = 1242, 375, 720.0
K = np.array([[F, 0, 621.0], [0, F, 187.5], [0, 0, 1]])
NPTS = 1500


def problem(B):
    rng = np.random.default_rng(300 + B)
    lat = rng.normal(size=(B, 3))
    lat = (lat / np.linalg.norm(lat, axis=1, keepdims=True) * rng.uniform(0.8, 1.1, (B, 1))).astype(np.float32)
    params = []
    for b in range(B):
        z = float(rng.uniform(3.0, 30.0)) if B > 1 else 8.0
        scale = float(rng.uniform(1.8, 2.2))
        x = float(rng.uniform(-0.35, 0.35)) * z
        params.append({"latent": torch.from_numpy(lat[b]), "scale": torch.tensor([scale]), "yaw": torch.tensor([float(rng.uniform(-3, 3))]),
                       "trans": torch.tensor([x / scale, 1.0 / scale, z / scale])})
    return params


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    vals = []
    for _ in range(WARM + REPS):
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        vals.append(a.elapsed_time(b))
    return float(np.median(vals[WARM:]))


def host_ms(fn):
    vals = []
    for _ in range(WARM + REPS):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        vals.append((time.perf_counter() - t) * 1e3)
    return float(np.median(vals[WARM:]))


def main():
    out_dir = sys.argv[1] if len(sys.argv) > 1 else "."
    os.makedirs(out_dir, exist_ok=True)
    L = _lib.lib()
    P = _lib.ptr
    dec = sdflabel_amd.setup_dsdf(ASSET + ".pt", precision=torch.float16)[0].to(DEV)
    handle, fwd, _ = M._decoder_mode(dec, torch.device(DEV))
    res = {"config": "deepsdf_synth (8 x 512, latent 3) in its float16 mode; meshes at R = 64; image %d x %d, f = %g; %d points per annotation; "
                     "device events on the current stream (host clock for the whole calls); WARM %d, REPS %d, medians" % (W, H, F, NPTS, WARM, REPS),
           "cases": {}}
    for B in (1, 16):
        params = problem(B)
        meshes = [m.to_camera() for m in M.meshes_many(dec, params, resolution=64)]
        boxes, clouds = [], []
        rng = np.random.default_rng(B)
        for m in meshes:
            v = m.vertices_numpy()
            u, w = VR.project(F, K[0, 2], v[:, 0], v[:, 2]), VR.project(F, K[1, 2], v[:, 1], v[:, 2])
            boxes.append([float(np.floor(u.min())), float(np.floor(w.min())), float(np.ceil(u.max())), float(np.ceil(w.max()))])
            clouds.append(m.vertices[torch.from_numpy(rng.choice(len(v), NPTS, replace=len(v) < NPTS)).to(DEV)].contiguous())
        size = (W, H)
        _, win = V.label_windows(boxes, size)
        rb = V.raster_batch(meshes, K, win, size, 0.1)
        keys = torch.empty((rb.P,), dtype=torch.int64, device=DEV)
        _, d = V.band_counts(dec, params, clouds, return_details=True)
        k4 = (ctypes.c_double * 4)(F, F, K[0, 2], K[1, 2])
        st = _lib.stream_ptr()
        Vn, Tn, N = int(rb.vertices.shape[0]), int(rb.faces.shape[0]), int(d["points"].shape[0])
        Ld = int(d["latents"].shape[1])
        counts8 = torch.empty((B, 8), dtype=torch.int32, device=DEV)
        counts3 = torch.empty((B, 3), dtype=torch.int32, device=DEV)
        stage = {
            "raster": event_ms(lambda: _lib.check(L.sdfr_mesh_raster(
                P(rb.vertices), Vn, P(rb.faces), Tn, P(rb.d_voff), P(rb.d_toff), P(rb.d_win), P(rb.d_poff), rb.P, B, W, H, k4, 0.1,
                P(keys), P(rb.mask), P(rb.depth), P(rb.triangle), P(rb.flags), st), "sdfr_mesh_raster")),
            "mask_counts": event_ms(lambda: _lib.check(L.sdfr_verify_mask_counts(
                P(rb.mask), None, P(rb.d_win), P(rb.d_poff), rb.P, B, W, H, P(counts8), st), "sdfr_verify_mask_counts")),
            "point_rows": event_ms(lambda: _lib.check(L.sdfr_verify_point_rows(
                P(d["points"]), N, P(d["d_ptoff"]), B, P(d["pose"]), P(d["latents"]), Ld, 0, N, P(d["rows"]), P(d["in_cube"]), st),
                "sdfr_verify_point_rows")),
            "decoder": event_ms(lambda: _lib.check(fwd(handle.h, P(d["rows"]), N, P(d["sdf"]), None, st), "decoder forward")),
            "band_counts": event_ms(lambda: _lib.check(L.sdfr_verify_band_counts(
                P(d["sdf"]), P(d["in_cube"]), N, P(d["d_ptoff"]), B, P(d["pose"]), 0.2, P(counts3), st), "sdfr_verify_band_counts")),
        }
        call = lambda: V.verify_many(dec, params, meshes, clouds, K, boxes, size)          # noqa: E731
        verdicts = call()
        kl, cp = count_launches(call)
        entry = {"stage_ms": {a: round(b, 4) for a, b in stage.items()},
                 "verify_many_ms": round(host_ms(call), 4),
                 "meshes_many_R64_ms": round(host_ms(lambda: M.meshes_many(dec, params, resolution=64)), 4),
                 "triangles": Tn, "window_pixels": rb.P, "points": N, "kernel_launches": kl, "copies": cp,
                 "host_synchronisations": count_syncs(call), "accepted": sum(r["ok"] for r in verdicts),
                 "iou_box": [round(r["iou_box"], 4) for r in verdicts], "share": [round(r["share"], 4) for r in verdicts]}
        if B == 1:
            v, f = meshes[0].vertices_numpy(), meshes[0].faces_numpy()
            pts, pose, lat, sdf = d["points"].cpu().numpy(), d["pose"].cpu().numpy(), d["latents"].cpu().numpy(), d["sdf"].cpu().numpy()
            t0 = time.perf_counter()
            rm = VR.raster(v, f, (F, F, K[0, 2], K[1, 2]), win[0])
            t1 = time.perf_counter()
            c8 = VR.mask_counts(rm[0], win[0])
            _, inside = VR.point_rows(pts, d["ptoff"], pose, lat)
            c3 = VR.band_counts(sdf, inside, d["ptoff"], pose, 0.2)
            t2 = time.perf_counter()
            entry["numpy_restatement_ms"] = {"raster": round((t1 - t0) * 1e3, 1), "counts_rows_band": round((t2 - t1) * 1e3, 3)}
            entry["numpy_agrees"] = bool(rm[0].tobytes() == rb.mask.cpu().numpy().tobytes() and c8[0] == verdicts[0]["area"]
                                         and c3[0].tolist() == [verdicts[0]["n_pts"], verdicts[0]["n_cube"], verdicts[0]["n_band"]])
        res["cases"]["B%d" % B] = entry
        print("B=%d" % B, json.dumps(entry), flush=True)
    json.dump(res, open(os.path.join(out_dir, "verify_time.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
