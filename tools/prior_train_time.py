"""GPU timing, peak memory and launch count of a shape-prior training step of the 8x512 decoder at n = 4 096, 16 384 and 65 536 rows.

fused       the training kernels of csrc/mlp_train.hip: the forward call (sdfr_decoder_train_forward) and the backward call
            (sdfr_decoder_train_backward: input gradient and weight gradient together; the split between the two is in the kernel statistics,
            profiles/prior_train_kernel_stats.csv: train_gemm_kernel<1> is the input gradient, <2> the weight gradient), and a whole
            PriorTrainer.step (fold, latent expansion, loss, backward, Adam) with dropout 0.2.
torch_ops   the same step with the decoder in plain torch ops under torch's autograd on the same GPU, float32, torch's own dropout: the
            yardstick.
floor       3 x 2 x sdfr_decoder_macs x n FLOP at the measured exact-f32 MFMA rate of 155 TFLOP/s.

Device events around windows of INNER steps, the two sides alternating in the same run, median of REPS windows after WARM warm-up windows.
Peak extra memory: torch.cuda.max_memory_allocated over one step minus what is allocated before it.  Launches: the kernels torch's profiler
sees in one step.

usage: python tools/prior_train_time.py OUT_DIR          (writes OUT_DIR/prior_train_time.json)
       python tools/prior_train_time.py --once fused|torch_ops N     (a few steps of one side, for a kernel trace)
"""
import json
import os
import subprocess
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from sdflabel_amd.deepsdf.train import train_backward, train_forward  # noqa: E402
from sdflabel_amd.pipelines.train_prior import PriorTrainer, clamped_l1, default_specs, effective_weights  # noqa: E402

DEV = "cuda:0"
WARM, REPS, INNER = 2, 7, 3
MFMA_F32 = 155e12
SHAPES = 8


def plain_forward(decoder, inputs, drop_p):
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
            if drop_p > 0 and l in decoder.dropout:
                x = torch.nn.functional.dropout(x, p=drop_p, training=True)
    return torch.tanh(x)


def window(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(INNER):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / INNER


def alternate(fns):
    for _ in range(WARM):
        for f in fns:
            window(f)
    ts = [[] for _ in fns]
    for _ in range(REPS):
        for t, f in zip(ts, fns):
            t.append(window(f))
    return [{"median_ms": round(float(np.median(v)), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)} for v in ts]


def peak_extra(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated() - base)


def launches(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return int(sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA))
    except Exception as e:                                                                                              # noqa: BLE001
        return "not counted: %s" % e


def clocks():
    try:
        return subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=30).stdout.strip().splitlines()
    except Exception as e:                                                                                              # noqa: BLE001
        return ["rocm-smi --showclocks: %s" % e]


def sides(n):
    specs = default_specs()
    g = torch.Generator().manual_seed(1)
    rows = torch.cat([torch.rand(n, 3, generator=g) * 2 - 1, torch.randn(n, 1, generator=g) * 0.1], 1).to(DEV)
    shapes = torch.arange(SHAPES, device=DEV)
    tr = PriorTrainer(specs, SHAPES, DEV, seed=1)
    tt = PriorTrainer(specs, SHAPES, DEV, seed=1)
    opt = tt.opt
    k = n // SHAPES

    def fused_step():
        return tr.step((shapes, rows))

    def torch_step():
        z = tt.latents[shapes]
        zn = z / z.norm(dim=1, keepdim=True)
        inputs = torch.cat([zn.repeat_interleave(k, 0), rows[:, :3]], 1)
        loss = clamped_l1(plain_forward(tt.decoder, inputs, 0.2)[:, 0], rows[:, 3], 0.1)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        return loss

    # the passes alone, on fixed weights
    with torch.no_grad():
        Ws, bs = effective_weights(tr.decoder)
        Ws, bs = [w.contiguous() for w in Ws], [b.contiguous() for b in bs]
    desc = tr.desc
    x = torch.cat([torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=1).to(DEV), rows[:, :3]], 1).contiguous()
    ws = desc.workspace(n, torch.device(DEV))
    sdf = torch.empty((n,), device=DEV)
    gs = torch.full((n,), 1.0 / n, device=DEV)
    dW, db = [torch.empty_like(w) for w in Ws], [torch.empty_like(b) for b in bs]
    gin = torch.empty((n, 6), device=DEV)

    def fwd():
        train_forward(desc, Ws, bs, x, 0.2, 7, ws, sdf)

    def bwd():
        train_backward(desc, Ws, gs, ws, dW, db, gin)

    xt = x.clone().requires_grad_(True)
    keep = {}

    def torch_fwd():
        keep["out"] = plain_forward(tt.decoder, xt, 0.2)

    def torch_bwd():
        torch_fwd()
        keep["out"].backward(gs[:, None])
    return fused_step, torch_step, fwd, bwd, torch_fwd, torch_bwd, desc


def main():
    assert torch.cuda.is_available(), "prior_train_time.py measures on the GPU only"
    if len(sys.argv) > 1 and sys.argv[1] == "--once":
        fused_step, torch_step = sides(int(sys.argv[3]))[:2]
        fn = fused_step if sys.argv[2] == "fused" else torch_step
        for _ in range(4):
            fn()
        torch.cuda.synchronize()
        return
    out_dir = sys.argv[1] if len(sys.argv) > 1 else "."
    os.makedirs(out_dir, exist_ok=True)
    res = {"config": "device events around windows of %d steps; the sides alternate in the same run; median of %d windows after %d warm-up "
                     "windows; 8x512 decoder (latent 3, latent_in [4], weight norm), float32, dropout 0.2, %d shapes per batch"
                     % (INNER, REPS, WARM, SHAPES), "device": torch.cuda.get_device_name(0), "clocks_before": clocks(), "sizes": {}}
    for n in (4096, 16384, 65536):
        fused_step, torch_step, fwd, bwd, torch_fwd, torch_bwd, desc = sides(n)
        t = alternate([fused_step, torch_step, fwd, bwd, torch_fwd, torch_bwd])
        floor_ms = 3 * 2 * desc.macs() * n / MFMA_F32 * 1e3
        r = {"step_fused": t[0], "step_torch_ops": t[1], "forward_fused": t[2], "backward_fused_dx_and_dw": t[3], "forward_torch_ops": t[4],
             "forward_plus_backward_torch_ops": t[5], "torch_step_over_fused_step": round(t[1]["median_ms"] / t[0]["median_ms"], 3),
             "floor_ms": round(floor_ms, 4), "fused_passes_over_floor": round((t[2]["median_ms"] + t[3]["median_ms"]) / floor_ms, 2),
             "decoder_macs": desc.macs(), "workspace_bytes": desc.bytes(n),
             "peak_extra_bytes_fused_step": peak_extra(fused_step), "peak_extra_bytes_torch_step": peak_extra(torch_step),
             "launches_fused_step": launches(fused_step), "launches_torch_step": launches(torch_step),
             "launches_fused_forward": launches(fwd), "launches_fused_backward": launches(bwd)}
        res["sizes"]["n%d" % n] = r
        print("n=%d" % n, json.dumps(r), flush=True)
        del fused_step, torch_step, fwd, bwd, torch_fwd, torch_bwd
        torch.cuda.empty_cache()
    res["clocks_after"] = clocks()
    json.dump(res, open(os.path.join(out_dir, "prior_train_time.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
