"""GPU timing of the joint fit of one shape to several views (sdflabel_amd/track.py) on the 8x512 decoder, float32 and float16.

iteration   1 x 1, 4 x 4 and 16 x 4 tracks x views, 8 000 rows per view, every row on every iteration: align_tracks (latent, yaw, trans and
            scale fitted, one latent and one scale per track) against align.align_many on the same V views IN THE SAME PROCESS -- align_many's
            code and kernels are what they were before the joint fit existed, so it stands for the parent commit.  align_many is clocked in
            TWO windows of every round, before and after align_tracks: the ratio of the two is the run-to-run spread a ratio is read against.
kernel      sdfr_track_step alone against sdfr_align_step alone on the same V views, in windows of CALLS = 2 000 back-to-back calls.

Device events around windows of ITERS iterations; the median of REPS windows after WARM warm-up windows, the sides alternating within the
same run (tools/encode_time.py's clock, tools/align_time.py's method).

usage: python tools/track_time.py OUT_DIR         (writes OUT_DIR/track_time.json)
"""
import ctypes
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from align_time import CALLS, FIT, OFFSET, SCALE, TRANS, YAW  # noqa: E402
from encode_time import DEV, ITERS, REPS, ROWS, WARM, alternate, plain_forward  # noqa: E402
from sdflabel_amd import _lib  # noqa: E402
from sdflabel_amd.align import align_many  # noqa: E402
from sdflabel_amd.complete import BoundSamples  # noqa: E402
from sdflabel_amd.deepsdf.workspace import setup_dsdf  # noqa: E402
from sdflabel_amd.fixtures import ASSET  # noqa: E402
from sdflabel_amd.track import align_tracks  # noqa: E402

SHAPES = ((1, 1), (4, 4), (16, 4))                     # tracks x views per track


def main():
    assert torch.cuda.is_available(), "track_time.py measures on the GPU only"
    out_dir = sys.argv[1] if len(sys.argv) > 1 else "."
    os.makedirs(out_dir, exist_ok=True)
    L, P = _lib.lib(), _lib.ptr
    res = {"config": "8x512 decoder (latent 3, latent_in [4], weight norm); %d rows per view, every row on every iteration; device events around "
                     "windows of %d iterations (%d calls for a kernel alone), median of %d after %d warm-up, the sides alternating; align_many "
                     "clocked twice per round (before and after align_tracks)" % (ROWS, ITERS, CALLS, REPS, WARM),
           "device": torch.cuda.get_device_name(0), "precisions": {}}
    dec32 = setup_dsdf(ASSET + ".pt", precision=torch.float32)[0].to(DEV).eval()
    for p in dec32.parameters():
        p.requires_grad_(False)
    for prec, dtype in (("float32", torch.float32), ("float16", torch.float16)):
        dec = setup_dsdf(ASSET + ".pt", precision=dtype)[0].to(DEV).eval()
        for p in dec.parameters():
            p.requires_grad_(False)
        g = torch.Generator().manual_seed(3)
        sizes = {}
        for T, n in SHAPES:
            V = T * n
            own = torch.arange(T).repeat_interleave(n)
            z_true = torch.nn.functional.normalize(torch.randn(T, 3, generator=g), dim=1)[own].to(DEV)
            xyz = (torch.rand(V, ROWS, 3, generator=g) * 1.8 - 0.9).to(DEV)
            with torch.no_grad():
                sdf = plain_forward(dec32, torch.cat([z_true.repeat_interleave(ROWS, 0), xyz.reshape(-1, 3)], 1)).reshape(V, ROWS, 1)
            width = (torch.rand(V, ROWS, 2, generator=g) * 0.05).to(DEV)
            kind = torch.arange(ROWS, device=DEV)[None, :, None] % 3
            bounds = torch.cat([sdf - width[:, :, :1] * (kind == 2), sdf + width[:, :, 1:] * (kind >= 1)], 2)
            yaw = (YAW + 2.1 * (torch.arange(V) % n).float()).to(DEV)                                    # the views of a track see it from different sides
            c, sn = torch.cos(yaw)[:, None], torch.sin(yaw)[:, None]
            xs = xyz * torch.tensor([1.0, -1.0, 1.0], device=DEV)
            cam = SCALE * (torch.stack([c * xs[:, :, 0] + sn * xs[:, :, 2], xs[:, :, 1], -sn * xs[:, :, 0] + c * xs[:, :, 2]], 2) + torch.tensor(TRANS, device=DEV))
            metric = torch.cat([cam, SCALE * bounds], 2).contiguous()
            samples = [BoundSamples(metric[b]) for b in range(V)]
            z0 = (-z_true).contiguous()
            theta0 = (torch.cat([yaw[:, None], torch.tensor([[*TRANS, SCALE]], device=DEV).repeat(V, 1)], 1) + torch.tensor([OFFSET], device=DEV)).contiguous()
            params = [{"yaw": theta0[b, 0:1], "trans": theta0[b, 1:4], "scale": theta0[b, 4:5], "latent": z0[b]} for b in range(V)]
            tracks = [{"latent": z0[t * n], "scale": theta0[t * n, 4:5], "views": [{"yaw": theta0[b, 0:1], "trans": theta0[b, 1:4]} for b in range(t * n, (t + 1) * n)]}
                      for t in range(T)]
            many = lambda: align_many(dec, params, None, samples=samples, iters=ITERS, rows_per_iter=ROWS, fit=FIT)        # noqa: E731
            t = alternate([many, lambda: align_tracks(dec, tracks, samples=samples, iters=ITERS, rows_per_iter=ROWS, fit=FIT), many], ITERS)
            r = {"tracks": T, "views": V, "rows": V * ROWS, "iteration_align_many": t[0], "iteration_align_tracks": t[1], "iteration_align_many_again": t[2],
                 "align_tracks_over_align_many": round(t[1]["median_ms"] / t[0]["median_ms"], 4),
                 "align_many_again_over_align_many": round(t[2]["median_ms"] / t[0]["median_ms"], 4)}
            if prec == "float32":
                Ld = 3
                voff = (torch.arange(T + 1, dtype=torch.int64) * n).to(DEV)
                gr = (0.01 * torch.randn(V, Ld + 5, dtype=torch.float64, generator=g)).to(DEV)
                loss = torch.full((V,), 0.01, dtype=torch.float64, device=DEV)
                pose = torch.cat([torch.cos(theta0[:, :1]), torch.sin(theta0[:, :1]), theta0[:, 1:]], 1).contiguous()
                rates = (ctypes.c_float * 5)(1e-4, 1e-4, 1e-4, 1e-4, 1e-4)
                st = _lib.stream_ptr()
                z, m, v = z0.clone(), torch.zeros_like(z0), torch.zeros_like(z0)
                th, tm, tv, ps, fl = theta0.clone(), torch.zeros_like(theta0), torch.zeros_like(theta0), pose.clone(), torch.zeros(V, dtype=torch.int32, device=DEV)
                zt, mt, vt = z0[::n].contiguous(), torch.zeros((T, Ld), device=DEV), torch.zeros((T, Ld), device=DEV)
                sc, sm, sv = theta0[::n, 4].contiguous(), torch.zeros(T, device=DEV), torch.zeros(T, device=DEV)
                th2, tm2, tv2, ps2, fl2 = theta0.clone(), torch.zeros_like(theta0), torch.zeros_like(theta0), pose.clone(), torch.zeros(V, dtype=torch.int32, device=DEV)
                zv, tl, tf = z0.clone(), torch.zeros(T, dtype=torch.float64, device=DEV), torch.zeros(T, dtype=torch.int32, device=DEV)

                def align_step():
                    for i in range(CALLS):
                        _lib.check(L.sdfr_align_step(P(z), P(m), P(v), Ld, V, 1, P(th), P(tm), P(tv), P(ps), P(gr), P(loss), P(fl), 1e-4, 1e-4, rates, i + 1,
                                                     None, 0, st), "sdfr_align_step")

                def track_step():
                    for i in range(CALLS):
                        _lib.check(L.sdfr_track_step(P(zt), P(mt), P(vt), Ld, T, 1, P(sc), P(sm), P(sv), 1, P(voff), V, None, P(th2), P(tm2), P(tv2), P(ps2), P(zv),
                                                     P(gr), P(loss), P(fl2), P(tl), P(tf), 1e-4, 1e-4, rates, i + 1, None, 0, st), "sdfr_track_step")

                t = alternate([align_step, track_step, align_step], CALLS)
                r["step_align"], r["step_track"], r["step_align_again"] = t
                r["step_track_over_step_align"] = round(t[1]["median_ms"] / t[0]["median_ms"], 4)
                assert not bool(tf.any()) and not bool(fl2.any())                                    # every window stepped every track
            sizes["%dx%d" % (T, n)] = r
            print(prec, "%d x %d" % (T, n), json.dumps(r), flush=True)
            del samples, metric, xyz, sdf, cam
            torch.cuda.empty_cache()
        res["precisions"][prec] = sizes
    json.dump(res, open(os.path.join(out_dir, "track_time.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
