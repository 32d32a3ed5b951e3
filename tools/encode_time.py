"""GPU timing and peak memory of the shape encoder (sdflabel_amd/encode.py) on the 8x512 decoder: B = 1 / 16 / 64 shapes x 8 000 rows, every row on
every iteration (draw off, so both sides see the same rows), exact float32 and float16.

fused       encode_many: per iteration sdfr_encode_rows, the decoder forward with masks, sdfr_mlp_jacobian, sdfr_encode_reduce, sdfr_encode_step.
            Per-iteration time: device events around a call of ITERS iterations, minus nothing, divided by ITERS (the buffers are allocated inside
            the call; they are a few launches against ITERS x 6).  Whole call: 800 iterations, device events and host wall clock.
torch_ops   the same fit with the decoder in plain torch ops under torch's autograd and torch.optim.Adam on the same GPU, float32: the yardstick
            (the parent commit has no encoding path).  Clocked the same way.

Median of REPS windows after WARM warm-up windows, the two sides alternating.  Peak extra memory: torch.cuda.max_memory_allocated over one call
minus what is allocated before it.

usage: python tools/encode_time.py OUT_DIR [--quick]         (writes OUT_DIR/encode_time.json)
"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from sdflabel_amd.deepsdf.workspace import setup_dsdf  # noqa: E402
from sdflabel_amd.encode import encode_many  # noqa: E402
from sdflabel_amd.fixtures import ASSET  # noqa: E402
from sdflabel_amd.pipelines.train_prior import effective_weights  # noqa: E402
from sdflabel_amd.sdf_samples import SdfSamples  # noqa: E402

DEV = "cuda:0"
ROWS = 8000
WARM, REPS, ITERS = 1, 5, 20


def plain_forward(decoder, inputs):
    Ws, bs = effective_weights(decoder)
    inj = decoder._inject_table()
    n = len(Ws) - 1
    x = inputs
    for l in range(n + 1):
        if inj[l][0]:
            x = torch.cat([x, inputs[:, inj[l][1]:inj[l][1] + inj[l][0]]], 1)
        x = torch.nn.functional.linear(x, Ws[l], bs[l])
        if l < n:
            x = torch.relu(x)
    return torch.tanh(x)


def torch_fit(dec, rows, z0, iters, lr=5e-3, clamp=0.1):
    """rows [B][k][4]; the loss is the sum over shapes of each shape's mean, so every latent sees its own gradient"""
    B, k = rows.shape[0], rows.shape[1]
    z = z0.clone().requires_grad_(True)
    opt = torch.optim.Adam([z], lr=lr)
    xyz, sdf = rows[:, :, :3].reshape(-1, 3), rows[:, :, 3]
    step = max(1, iters // 2)
    for it in range(iters):
        opt.param_groups[0]["lr"] = lr * 0.1 ** (it // step)
        zn = z / z.norm(dim=1, keepdim=True)
        pred = plain_forward(dec, torch.cat([zn.repeat_interleave(k, 0), xyz], 1))[:, 0].reshape(B, k)
        loss = (pred.clamp(-clamp, clamp) - sdf.clamp(-clamp, clamp)).abs().mean(1).sum()
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
    return z.detach()


def events(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3


def alternate(fns, per):
    for _ in range(WARM):
        for f in fns:
            events(f)
    ts = [[] for _ in fns]
    for _ in range(REPS):
        for t, f in zip(ts, fns):
            t.append(events(f)[0] / per)
    return [{"median_ms": round(float(np.median(v)), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)} for v in ts]


def peak_extra(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated() - base)


def main():
    assert torch.cuda.is_available(), "encode_time.py measures on the GPU only"
    out_dir = sys.argv[1] if len(sys.argv) > 1 else "."
    quick = "--quick" in sys.argv
    os.makedirs(out_dir, exist_ok=True)
    dec32 = setup_dsdf(ASSET + ".pt", precision=torch.float32)[0].to(DEV).eval()
    dec16 = setup_dsdf(ASSET + ".pt", precision=torch.float16)[0].to(DEV).eval()
    for p in dec32.parameters():
        p.requires_grad_(False)
    res = {"config": "8x512 decoder (latent 3, latent_in [4], weight norm); %d rows per shape, every row on every iteration; device events around calls "
                     "of %d iterations, median of %d after %d warm-up, the sides alternating; whole calls: 800 iterations, one run each" % (ROWS, ITERS, REPS, WARM),
           "device": torch.cuda.get_device_name(0), "sizes": {}}
    g = torch.Generator().manual_seed(3)
    for B in (1, 16, 64):
        z_true = torch.nn.functional.normalize(torch.randn(B, 3, generator=g), dim=1).to(DEV)
        xyz = (torch.rand(B, ROWS, 3, generator=g) * 2 - 1).to(DEV)
        with torch.no_grad():
            sdf = plain_forward(dec32, torch.cat([z_true.repeat_interleave(ROWS, 0), xyz.reshape(-1, 3)], 1)).reshape(B, ROWS, 1)
        rows = torch.cat([xyz, sdf], 2).contiguous()
        samples = [SdfSamples(rows[b]) for b in range(B)]
        z0 = (-z_true).contiguous()

        def fused32(iters=ITERS):
            return encode_many(dec32, samples, iters=iters, rows_per_iter=ROWS, init=z0)

        def fused16(iters=ITERS):
            return encode_many(dec16, samples, iters=iters, rows_per_iter=ROWS, init=z0)

        def torch_ops(iters=ITERS):
            return torch_fit(dec32, rows, z0, iters)

        t = alternate([fused32, fused16, torch_ops], ITERS)
        r = {"rows": B * ROWS, "iteration_fused_f32": t[0], "iteration_fused_f16": t[1], "iteration_torch_ops": t[2],
             "torch_over_fused_f32": round(t[2]["median_ms"] / t[0]["median_ms"], 3),
             "peak_extra_bytes_fused_f32": peak_extra(fused32), "peak_extra_bytes_fused_f16": peak_extra(fused16),
             "peak_extra_bytes_torch_ops": peak_extra(torch_ops)}
        if not quick and B <= 16:
            kept = {}
            for name, fn in (("fused_f32", fused32), ("fused_f16", fused16), ("torch_ops", torch_ops)):
                ev, wall = events(lambda: kept.__setitem__(name, fn(800)))
                r["call_800_iterations_" + name] = {"device_ms": round(ev, 2), "wall_ms": round(wall, 2)}
            a, b = kept["fused_f32"], kept["torch_ops"]
            r["final_loss_fused_f32"] = [round(float(x), 6) for x in a.loss.tolist()[:4]]
            r["latent_gap_fused_vs_torch_after_800"] = round(float((torch.nn.functional.normalize(b, dim=1) - a.latents).abs().max()), 6)
        res["sizes"]["B%d" % B] = r
        print("B=%d" % B, json.dumps(r), flush=True)
        del samples, rows, xyz, sdf
        torch.cuda.empty_cache()
    json.dump(res, open(os.path.join(out_dir, "encode_time.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
