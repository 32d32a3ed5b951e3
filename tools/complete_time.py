"""GPU timing of shape completion from one view (sdflabel_amd/complete.py) on the 8x512 decoder, float32.

view        sdfr_view_samples alone: B shapes x 1 143 points with normals and 4 free-space rows (8 001 rows a shape), the C call only.
reduce      sdfr_bound_reduce against sdfr_encode_reduce of the same build on the same predictions and Jacobian (the bounds are lo = hi = the
            target, so both do the same sums): the interval rule's own cost.
iteration   B = 1 / 16 / 64 shapes x 8 000 rows, every row on every iteration: encode_many on exact rows, fit_many on the same rows through
            BoundSamples.from_sdf (the same bits), fit_many on interval rows (a third exact, a third one-sided, a third two-sided), and the
            interval fit in plain torch ops under torch's autograd with torch.optim.Adam.

Device events around windows of ITERS iterations, or of CALLS = 2 000 back-to-back calls for the kernels timed alone (they take about
12 us, so a short window would clock the launch rate); the median of REPS windows after WARM warm-up windows, the sides alternating within
the same run (tools/encode_time.py's clock).  The figures of the kernels alone are calls per second of a stream kept full: two launches
a reduce, one a view.

usage: python tools/complete_time.py OUT_DIR         (writes OUT_DIR/complete_time.json)
"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from encode_time import DEV, ITERS, REPS, ROWS, WARM, alternate, plain_forward  # noqa: E402
from sdflabel_amd import _lib  # noqa: E402
from sdflabel_amd.complete import BoundSamples, fit_many  # noqa: E402
from sdflabel_amd.deepsdf.workspace import setup_dsdf  # noqa: E402
from sdflabel_amd.encode import encode_many  # noqa: E402
from sdflabel_amd.fixtures import ASSET  # noqa: E402
from sdflabel_amd.sdf_samples import SdfSamples  # noqa: E402

POINTS, FREE = 1143, 4
CALLS = 2000           # calls per window of the kernels timed alone: about 12 us each, so a window is some 25 ms, not a few launches


def torch_interval_fit(dec, rows, z0, iters, lr=5e-3, clamp=0.1):
    """rows [B][k][5]; a row's loss is the distance from the clamped prediction to the clamped interval"""
    B, k = rows.shape[0], rows.shape[1]
    z = z0.clone().requires_grad_(True)
    opt = torch.optim.Adam([z], lr=lr)
    xyz, lo, hi = rows[:, :, :3].reshape(-1, 3), rows[:, :, 3].clamp(-clamp, clamp), rows[:, :, 4].clamp(-clamp, clamp)
    step = max(1, iters // 2)
    for it in range(iters):
        opt.param_groups[0]["lr"] = lr * 0.1 ** (it // step)
        zn = z / z.norm(dim=1, keepdim=True)
        cp = plain_forward(dec, torch.cat([zn.repeat_interleave(k, 0), xyz], 1))[:, 0].reshape(B, k).clamp(-clamp, clamp)
        loss = (torch.relu(lo - cp) + torch.relu(cp - hi)).mean(1).sum()
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
    return z.detach()


def main():
    assert torch.cuda.is_available(), "complete_time.py measures on the GPU only"
    out_dir = sys.argv[1] if len(sys.argv) > 1 else "."
    os.makedirs(out_dir, exist_ok=True)
    dec = setup_dsdf(ASSET + ".pt", precision=torch.float32)[0].to(DEV).eval()
    for p in dec.parameters():
        p.requires_grad_(False)
    L, P = _lib.lib(), _lib.ptr
    res = {"config": "8x512 decoder (latent 3, latent_in [4], weight norm), float32; %d rows per shape, every row on every iteration; device events "
                     "around windows of %d iterations (%d calls for the kernels alone), median of %d after %d warm-up, the sides alternating" % (ROWS, ITERS, CALLS, REPS, WARM),
           "device": torch.cuda.get_device_name(0), "sizes": {}}
    g = torch.Generator().manual_seed(3)
    for B in (1, 16, 64):
        z_true = torch.nn.functional.normalize(torch.randn(B, 3, generator=g), dim=1).to(DEV)
        xyz = (torch.rand(B, ROWS, 3, generator=g) * 2 - 1).to(DEV)
        with torch.no_grad():
            sdf = plain_forward(dec, torch.cat([z_true.repeat_interleave(ROWS, 0), xyz.reshape(-1, 3)], 1)).reshape(B, ROWS, 1)
        exact = torch.cat([xyz, sdf], 2).contiguous()
        width = (torch.rand(B, ROWS, 2, generator=g) * 0.05).to(DEV)
        kind = torch.arange(ROWS, device=DEV)[None, :, None] % 3
        bounds = torch.cat([sdf - width[:, :, :1] * (kind == 2), sdf + width[:, :, 1:] * (kind >= 1)], 2)
        mixed = torch.cat([xyz, bounds], 2).contiguous()
        s_exact = [SdfSamples(exact[b]) for b in range(B)]
        s_same = [BoundSamples.from_sdf(s) for s in s_exact]
        s_mixed = [BoundSamples(mixed[b]) for b in range(B)]
        z0 = (-z_true).contiguous()
        t = alternate([lambda: encode_many(dec, s_exact, iters=ITERS, rows_per_iter=ROWS, init=z0),
                       lambda: fit_many(dec, s_same, iters=ITERS, rows_per_iter=ROWS, init=z0),
                       lambda: fit_many(dec, s_mixed, iters=ITERS, rows_per_iter=ROWS, init=z0),
                       lambda: torch_interval_fit(dec, mixed, z0, ITERS)], ITERS)
        r = {"rows": B * ROWS, "iteration_encode_many_exact": t[0], "iteration_fit_many_exact_rows": t[1], "iteration_fit_many_interval_rows": t[2],
             "iteration_torch_ops_interval": t[3], "fit_many_over_encode_many_exact_rows": round(t[1]["median_ms"] / t[0]["median_ms"], 4),
             "torch_over_fit_many_interval_rows": round(t[3]["median_ms"] / t[2]["median_ms"], 3)}
        # the two reduces alone, on one set of predictions
        n, Ld, NI = B * ROWS, 3, 6
        pred, J = torch.randn(n, device=DEV) * 0.05, torch.randn(n, NI, device=DEV)
        tgt = sdf.reshape(-1).contiguous()
        nbytes = int(L.sdfr_encode_ws_bytes(B, ROWS, Ld))
        ws = torch.empty((nbytes // 8,), dtype=torch.float64, device=DEV)
        loss, gz, fl = torch.empty(B, dtype=torch.float64, device=DEV), torch.empty(B, Ld, dtype=torch.float64, device=DEV), torch.zeros(B, dtype=torch.int32, device=DEV)
        st = _lib.stream_ptr()

        def exact_reduce():
            for _ in range(CALLS):
                _lib.check(L.sdfr_encode_reduce(P(pred), P(tgt), P(J), NI, Ld, B, ROWS, 0.1, P(ws), nbytes, P(loss), P(gz), P(fl), st), "sdfr_encode_reduce")

        def bound_reduce():
            for _ in range(CALLS):
                _lib.check(L.sdfr_bound_reduce(P(pred), P(tgt), P(tgt), P(J), NI, Ld, B, ROWS, 0.1, P(ws), nbytes, P(loss), P(gz), P(fl), st), "sdfr_bound_reduce")

        t = alternate([exact_reduce, bound_reduce], CALLS)
        r["reduce_exact"], r["reduce_interval"] = t
        r["reduce_interval_over_exact"] = round(t[1]["median_ms"] / t[0]["median_ms"], 4)
        # the view rows alone
        N = B * POINTS
        pts = (torch.rand(N, 3, generator=g) * 2 + torch.tensor([-1.0, -1.0, 4.0])).to(DEV)
        nrm = torch.randn(N, 3, generator=g, dtype=torch.float64).to(DEV)
        ptoff = (torch.arange(B + 1, dtype=torch.int64) * POINTS).to(DEV)
        pose = torch.tensor([[1.0, 0.0, 0.0, 0.0, 2.5, 2.0]] * B, dtype=torch.float32, device=DEV)
        org = torch.zeros(3, device=DEV)
        rows = torch.empty((N * (3 + FREE), 5), device=DEV)
        vfl = torch.empty(B, dtype=torch.int32, device=DEV)

        def view():
            for _ in range(CALLS):
                _lib.check(L.sdfr_view_samples(P(pts), P(nrm), N, P(ptoff), B, P(pose), P(org), 0, FREE, 0.01, 0.5, 7, P(rows), P(vfl), st), "sdfr_view_samples")

        r["view_samples"] = dict(alternate([view], CALLS)[0], points=N, rows=N * (3 + FREE), valid_rows=int(torch.isfinite(rows[:, 3]).sum()))
        res["sizes"]["B%d" % B] = r
        print("B=%d" % B, json.dumps(r), flush=True)
        del s_exact, s_same, s_mixed, exact, mixed, xyz, sdf, pred, J
        torch.cuda.empty_cache()
    json.dump(res, open(os.path.join(out_dir, "complete_time.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
