"""GPU timing of the pose-and-shape fit to one view (sdflabel_amd/align.py) on the 8x512 decoder, float32 and float16.

iteration   B = 1 / 16 / 64 shapes x 8 000 rows, every row on every iteration: align_many (latent, yaw, trans and scale fitted) against
            complete.fit_many on the same row count IN THE SAME PROCESS -- fit_many's code is what it was before align existed, so it stands
            for the parent commit --, and the same five-parameter fit in plain torch ops under torch's autograd with torch.optim.Adam.
kernels     sdfr_align_rows, sdfr_align_reduce and sdfr_align_step alone, in windows of CALLS = 2 000 back-to-back calls (they take some
            ten microseconds, so a short window would clock the launch rate); sdfr_bound_rows and sdfr_bound_reduce beside them.

Device events around windows of ITERS iterations; the median of REPS windows after WARM warm-up windows, the sides alternating within the
same run (tools/encode_time.py's clock).

usage: python tools/align_time.py OUT_DIR         (writes OUT_DIR/align_time.json)
"""
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from encode_time import DEV, ITERS, REPS, ROWS, WARM, alternate, plain_forward  # noqa: E402
from sdflabel_amd import _lib  # noqa: E402
from sdflabel_amd.align import align_many  # noqa: E402
from sdflabel_amd.complete import BoundSamples, fit_many  # noqa: E402
from sdflabel_amd.deepsdf.workspace import setup_dsdf  # noqa: E402
from sdflabel_amd.fixtures import ASSET  # noqa: E402

CALLS = 2000
YAW, TRANS, SCALE = 0.6, (0.2, -0.1, 3.0), 1.8
OFFSET = (0.02, 0.01, -0.01, 0.01, 0.02)             # the start minus the truth: yaw, tx, ty, tz, scale
FIT = ("yaw", "trans", "scale", "latent")


def torch_align_fit(dec, rows, z0, theta0, iters, lr=5e-3, lr_pose=1e-2, clamp=0.2):
    """rows [B][k][5] camera-frame and metric; the loss of a row is the distance from the clamped scale * sdf(x(theta)) to the clamped
    interval; a row whose x leaves the cube sits out"""
    B, k = rows.shape[0], rows.shape[1]
    z, th = z0.clone().requires_grad_(True), theta0.clone().requires_grad_(True)
    opt = torch.optim.Adam([{"params": [z], "lr": lr, "base": lr}, {"params": [th], "lr": lr_pose, "base": lr_pose}])
    q, lo, hi = rows[:, :, :3], rows[:, :, 3].clamp(-clamp, clamp), rows[:, :, 4].clamp(-clamp, clamp)
    step = max(1, iters // 2)
    for it in range(iters):
        for grp in opt.param_groups:
            grp["lr"] = grp["base"] * 0.1 ** (it // step)
        zn = z / z.norm(dim=1, keepdim=True)
        c, sn, sc = torch.cos(th[:, 0:1]), torch.sin(th[:, 0:1]), th[:, 4:5]
        q0, q1, q2 = q[:, :, 0] / sc - th[:, 1:2], q[:, :, 1] / sc - th[:, 2:3], q[:, :, 2] / sc - th[:, 3:4]
        x = torch.stack([c * q0 - sn * q2, -q1, sn * q0 + c * q2], 2)
        inside = (x.detach().abs() <= 1).all(2)
        x = torch.where(inside[:, :, None], x, torch.zeros_like(x))
        cp = (sc * plain_forward(dec, torch.cat([zn.repeat_interleave(k, 0), x.reshape(-1, 3)], 1))[:, 0].reshape(B, k)).clamp(-clamp, clamp)
        dist = torch.relu(lo - cp) + torch.relu(cp - hi)
        loss = (torch.where(inside, dist, torch.zeros_like(dist)).sum(1) / inside.sum(1).clamp(min=1)).sum()
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
    return z.detach(), th.detach()


def main():
    assert torch.cuda.is_available(), "align_time.py measures on the GPU only"
    out_dir = sys.argv[1] if len(sys.argv) > 1 else "."
    os.makedirs(out_dir, exist_ok=True)
    L, P = _lib.lib(), _lib.ptr
    res = {"config": "8x512 decoder (latent 3, latent_in [4], weight norm); %d rows per shape, every row on every iteration; device events around "
                     "windows of %d iterations (%d calls for the kernels alone), median of %d after %d warm-up, the sides alternating"
                     % (ROWS, ITERS, CALLS, REPS, WARM),
           "device": torch.cuda.get_device_name(0), "precisions": {}}
    dec32 = setup_dsdf(ASSET + ".pt", precision=torch.float32)[0].to(DEV).eval()          # the torch ops run in float32 beside either precision
    for p in dec32.parameters():
        p.requires_grad_(False)
    for prec, dtype in (("float32", torch.float32), ("float16", torch.float16)):
        dec = setup_dsdf(ASSET + ".pt", precision=dtype)[0].to(DEV).eval()
        for p in dec.parameters():
            p.requires_grad_(False)
        g = torch.Generator().manual_seed(3)
        sizes = {}
        for B in (1, 16, 64):
            z_true = torch.nn.functional.normalize(torch.randn(B, 3, generator=g), dim=1).to(DEV)
            xyz = (torch.rand(B, ROWS, 3, generator=g) * 1.8 - 0.9).to(DEV)
            with torch.no_grad():
                sdf = plain_forward(dec32, torch.cat([z_true.repeat_interleave(ROWS, 0), xyz.reshape(-1, 3)], 1)).reshape(B, ROWS, 1)
            width = (torch.rand(B, ROWS, 2, generator=g) * 0.05).to(DEV)
            kind = torch.arange(ROWS, device=DEV)[None, :, None] % 3
            bounds = torch.cat([sdf - width[:, :, :1] * (kind == 2), sdf + width[:, :, 1:] * (kind >= 1)], 2)
            lattice = torch.cat([xyz, bounds], 2).contiguous()
            c, sn = float(np.cos(YAW)), float(np.sin(YAW))
            xs = xyz * torch.tensor([1.0, -1.0, 1.0], device=DEV)
            cam = SCALE * (torch.stack([c * xs[:, :, 0] + sn * xs[:, :, 2], xs[:, :, 1], -sn * xs[:, :, 0] + c * xs[:, :, 2]], 2)
                           + torch.tensor(TRANS, device=DEV))
            metric = torch.cat([cam, SCALE * bounds], 2).contiguous()
            s_lattice = [BoundSamples(lattice[b]) for b in range(B)]
            s_metric = [BoundSamples(metric[b]) for b in range(B)]
            z0 = (-z_true).contiguous()
            theta0 = (torch.tensor([[YAW, *TRANS, SCALE]], device=DEV) + torch.tensor([OFFSET], device=DEV)).repeat(B, 1).contiguous()
            params = [{"yaw": theta0[b, 0:1], "trans": theta0[b, 1:4], "scale": theta0[b, 4:5], "latent": z0[b]} for b in range(B)]
            t = alternate([lambda: fit_many(dec, s_lattice, iters=ITERS, rows_per_iter=ROWS, init=z0),
                           lambda: align_many(dec, params, None, samples=s_metric, iters=ITERS, rows_per_iter=ROWS, fit=FIT),
                           lambda: torch_align_fit(dec32, metric, z0, theta0, ITERS)], ITERS)
            r = {"rows": B * ROWS, "iteration_fit_many": t[0], "iteration_align_many": t[1], "iteration_torch_ops_align": t[2],
                 "align_many_over_fit_many": round(t[1]["median_ms"] / t[0]["median_ms"], 4),
                 "fit_many_spread": round(t[0]["max_ms"] / t[0]["min_ms"], 4),
                 "torch_over_align_many": round(t[2]["median_ms"] / t[1]["median_ms"], 3)}
            if prec == "float32":
                # the kernels alone, on one set of rows, predictions and Jacobians
                n, Ld, NI = B * ROWS, 3, 6
                rows = metric.reshape(-1, 5).contiguous()
                soff = (torch.arange(B + 1, dtype=torch.int64) * ROWS).to(DEV)
                pose = torch.cat([torch.cos(theta0[:, :1]), torch.sin(theta0[:, :1]), theta0[:, 1:]], 1).contiguous()
                inputs, J = torch.empty((n, NI), device=DEV), torch.randn(n, NI, device=DEV)
                camb, lo, hi, pred = torch.empty((n, 3), device=DEV), torch.empty(n, device=DEV), torch.empty(n, device=DEV), torch.randn(n, device=DEV) * 0.05
                zn, fl = torch.empty((B, Ld), device=DEV), torch.zeros(B, dtype=torch.int32, device=DEV)
                nbytes = int(L.sdfr_align_ws_bytes(B, ROWS, Ld))
                ws = torch.empty((nbytes // 8,), dtype=torch.float64, device=DEV)
                loss, gr = torch.empty(B, dtype=torch.float64, device=DEV), torch.empty(B, Ld + 5, dtype=torch.float64, device=DEV)
                z, m, v = z0.clone(), torch.zeros_like(z0), torch.zeros_like(z0)
                th, tm, tv, ps = theta0.clone(), torch.zeros_like(theta0), torch.zeros_like(theta0), pose.clone()
                rates = (ctypes.c_float * 5)(1e-4, 1e-4, 1e-4, 1e-4, 1e-4)
                st = _lib.stream_ptr()

                def align_rows():
                    for _ in range(CALLS):
                        _lib.check(L.sdfr_align_rows(P(rows), n, P(soff), B, 0, ROWS, 0, 7, 0, P(z0), Ld, 1, P(pose), P(inputs), P(camb), P(lo), P(hi), P(zn),
                                                     P(fl), st), "sdfr_align_rows")

                def bound_rows():
                    for _ in range(CALLS):
                        _lib.check(L.sdfr_bound_rows(P(rows), n, P(soff), B, 0, ROWS, 0, 7, 0, P(z0), Ld, 1, P(inputs), P(lo), P(hi), P(zn), P(fl), st),
                                   "sdfr_bound_rows")

                def align_reduce():
                    for _ in range(CALLS):
                        _lib.check(L.sdfr_align_reduce(P(pred), P(lo), P(hi), P(J), NI, P(camb), P(pose), Ld, B, ROWS, 0.2, P(ws), nbytes, P(loss), P(gr),
                                                       P(fl), st), "sdfr_align_reduce")

                def bound_reduce():
                    for _ in range(CALLS):
                        _lib.check(L.sdfr_bound_reduce(P(pred), P(lo), P(hi), P(J), NI, Ld, B, ROWS, 0.2, P(ws), nbytes, P(loss), P(gr), P(fl), st),
                                   "sdfr_bound_reduce")

                def align_step():
                    for i in range(CALLS):
                        _lib.check(L.sdfr_align_step(P(z), P(m), P(v), Ld, B, 1, P(th), P(tm), P(tv), P(ps), P(gr), P(loss), P(fl), 1e-4, 1e-4, rates, i + 1,
                                                     None, 0, st), "sdfr_align_step")

                align_rows()
                t = alternate([bound_rows, align_rows], CALLS)
                r["rows_bound"], r["rows_align"] = t
                t = alternate([bound_reduce, align_reduce], CALLS)
                r["reduce_bound"], r["reduce_align"] = t
                align_reduce()
                r["step_align"] = alternate([align_step], CALLS)[0]
                del rows, inputs, J, camb, lo, hi, pred
            sizes["B%d" % B] = r
            print(prec, "B=%d" % B, json.dumps(r), flush=True)
            del s_lattice, s_metric, lattice, metric, xyz, sdf, cam
            torch.cuda.empty_cache()
        res["precisions"][prec] = sizes
    json.dump(res, open(os.path.join(out_dir, "align_time.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
