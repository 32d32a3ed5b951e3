"""GPU timing of the search for a fit's start (sdflabel_amd/search.py) on the 8x512 decoder, float32 and float16.

scoring     score_many of 1 / 16 shapes x 32 codes x 2 000 rows against what the code offered before the scoring pass for the same losses, IN
            THE SAME PROCESS: complete.fit_many with iters=1, lr=0 on the samples replicated once per start (it pays the Jacobian launch and
            the replicated upload, and draws other rows per replica).  The yardstick is clocked in TWO windows of every round, before and
            after score_many: the ratio of the two is the run-to-run spread a ratio is read against.
kernels     sdfr_search_rows, sdfr_search_reduce and sdfr_search_select alone, in windows of CALLS = 2 000 back-to-back calls.
whole       complete.fit_many(search=dict(codes=32, keep=3)) against fit_many from one start at equal iterations: the added cost is the
            scoring pass plus keep x the fit.

Device events around windows of WINDOW = 20 calls; the median of REPS windows after WARM warm-up windows, the sides alternating within the
same run (tools/encode_time.py's clock).

usage: python tools/search_time.py OUT_DIR         (writes OUT_DIR/search_time.json)
"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from encode_time import DEV, REPS, WARM, alternate, plain_forward  # noqa: E402
from sdflabel_amd import _lib  # noqa: E402
from sdflabel_amd import search as S  # noqa: E402
from sdflabel_amd.complete import BoundSamples, fit_many  # noqa: E402
from sdflabel_amd.deepsdf.workspace import setup_dsdf  # noqa: E402
from sdflabel_amd.fixtures import ASSET  # noqa: E402

WINDOW, CALLS = 20, 2000
CODES, ROWS, SAMPLES, KEEP, FIT_ITERS = 32, 2000, 6000, 3, 120


def repeat(fn, n):
    def run():
        for _ in range(n):
            fn()
    return run


def main():
    assert torch.cuda.is_available(), "search_time.py measures on the GPU only"
    out_dir = sys.argv[1] if len(sys.argv) > 1 else "."
    os.makedirs(out_dir, exist_ok=True)
    L, P = _lib.lib(), _lib.ptr
    res = {"config": "8x512 decoder (latent 3, latent_in [4], weight norm); %d codes x %d rows, %d samples a shape; device events around windows of %d "
                     "calls (%d for a kernel alone), median of %d after %d warm-up, the sides alternating; the yardstick clocked twice per round"
                     % (CODES, ROWS, SAMPLES, WINDOW, CALLS, REPS, WARM),
           "device": torch.cuda.get_device_name(0), "precisions": {}}
    dec32 = setup_dsdf(ASSET + ".pt", precision=torch.float32)[0].to(DEV).eval()
    for p in dec32.parameters():
        p.requires_grad_(False)
    codes = S.sphere_codes(3, CODES).to(DEV)
    for prec, dtype in (("float32", torch.float32), ("float16", torch.float16)):
        dec = setup_dsdf(ASSET + ".pt", precision=dtype)[0].to(DEV).eval()
        for p in dec.parameters():
            p.requires_grad_(False)
        g = torch.Generator().manual_seed(3)
        sizes = {}
        for B in (1, 16):
            z_true = torch.nn.functional.normalize(torch.randn(B, 3, generator=g), dim=1).to(DEV)
            xyz = (torch.rand(B, SAMPLES, 3, generator=g) * 1.8 - 0.9).to(DEV)
            with torch.no_grad():
                sdf = plain_forward(dec32, torch.cat([z_true.repeat_interleave(SAMPLES, 0), xyz.reshape(-1, 3)], 1)).reshape(B, SAMPLES, 1)
            width = (torch.rand(B, SAMPLES, 1, generator=g) * 0.05).to(DEV)
            samples = [BoundSamples(torch.cat([xyz[b], sdf[b], sdf[b] + width[b]], 1).contiguous()) for b in range(B)]
            N = B * CODES
            starts = codes.repeat(B, 1)
            own = torch.arange(B, dtype=torch.int32, device=DEV).repeat_interleave(CODES)
            replicated = [samples[b] for b in range(B) for _ in range(CODES)]

            def score():
                return S.score_many(dec, samples, starts, own, rows=ROWS, clamp=0.1, draw=True)

            def yardstick():
                return fit_many(dec, replicated, iters=1, rows_per_iter=ROWS, lr=0.0, clamp=0.1, init=starts, draw=True)

            t = alternate([repeat(yardstick, WINDOW), repeat(score, WINDOW), repeat(yardstick, WINDOW)], WINDOW)
            entry = {"starts": N, "fit_many_iters1_lr0_before": t[0], "score_many": t[1], "fit_many_iters1_lr0_after": t[2],
                     "ratio_score_to_yardstick": round(t[1]["median_ms"] / (0.5 * (t[0]["median_ms"] + t[2]["median_ms"])), 4),
                     "yardstick_spread": round(abs(t[0]["median_ms"] / t[2]["median_ms"] - 1.0), 4)}
            # the three kernels alone, on the buffers of one scoring pass
            srows = torch.cat([s.rows for s in samples]).contiguous()
            soff = (torch.arange(B + 1, dtype=torch.int64) * SAMPLES).to(DEV)
            inputs = torch.empty((N * ROWS, 6), device=DEV)
            lo, hi, pred = (torch.zeros((N * ROWS,), device=DEV) for _ in range(3))
            zn, flags = torch.empty_like(starts), torch.zeros((N,), dtype=torch.int32, device=DEV)
            loss = torch.zeros((N,), dtype=torch.float64, device=DEV)
            wsb = int(L.sdfr_search_ws_bytes(N, ROWS))
            ws = torch.empty((wsb // 8,), dtype=torch.float64, device=DEV)
            coff = (torch.arange(B + 1, dtype=torch.int64) * CODES).to(DEV)
            order, count = torch.empty((B, KEEP), dtype=torch.int32, device=DEV), torch.empty((B,), dtype=torch.int32, device=DEV)
            st = _lib.stream_ptr()

            def k_rows():
                _lib.check(L.sdfr_search_rows(P(srows), B * SAMPLES, P(soff), B, P(own), N, 0, ROWS, 1, 0, 0, P(starts), 3, 1, None, P(inputs), None, P(lo),
                                              P(hi), P(zn), P(flags), st), "sdfr_search_rows")

            def k_reduce():
                _lib.check(L.sdfr_search_reduce(P(pred), P(lo), P(hi), None, N, ROWS, 0.1, P(ws), wsb, P(loss), P(flags), st), "sdfr_search_reduce")

            def k_select():
                _lib.check(L.sdfr_search_select(P(loss), P(flags), P(coff), B, N, KEEP, P(order), P(count), st), "sdfr_search_select")

            k_rows()
            tk = alternate([repeat(k_rows, CALLS), repeat(k_reduce, CALLS), repeat(k_select, CALLS)], CALLS)
            entry["kernels_us"] = {n: {k.replace("_ms", "_us"): round(v * 1e3, 3) for k, v in x.items()} for n, x in zip(("rows", "reduce", "select"), tk)}
            # the whole fit with and without a search, at equal iterations
            kw = dict(iters=FIT_ITERS, rows_per_iter=ROWS, lr=2e-2, lr_step=80, clamp=0.1, draw=True)
            init = -z_true
            tw = alternate([lambda: fit_many(dec, samples, init=init, **kw), lambda: fit_many(dec, samples, search=dict(codes=codes, keep=KEEP, rows=ROWS), **kw),
                            lambda: fit_many(dec, samples, init=init, **kw)], 1)
            entry["whole_fit_ms"] = {"one_start_before": tw[0], "search_keep%d" % KEEP: tw[1], "one_start_after": tw[2],
                                     "ratio": round(tw[1]["median_ms"] / (0.5 * (tw[0]["median_ms"] + tw[2]["median_ms"])), 4)}
            sizes["%d_shapes" % B] = entry
            print(prec, B, json.dumps(entry), flush=True)
        res["precisions"][prec] = sizes
    with open(os.path.join(out_dir, "search_time.json"), "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
