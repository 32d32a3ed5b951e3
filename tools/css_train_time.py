"""GPU timing and peak memory of the CSS head's training step (losses + backward of the head alone) at 16 and 32 crops of 128 x 128.

fused       sdflabel_amd.css.css_head_loss + css_latent_loss, then .backward() of the summed loss: the fused call returns the unit gradients,
            backward scales them (csrc/css_train.hip).
torch_ops   the same head in plain torch on the same GPU: 1x1 convolutions, log_softmax, the product with the mask, CrossEntropyLoss /
            MSELoss and .backward(), as the training loop of the reference forms it.
floor       compute: 4 x 98 304 FLOP per pixel (logits, dX, the recomputed transposed logits, dW) at the exact-f32 MFMA peak (256 CUs x 4
            SIMDs x 64 FLOP per clock at 2.4 GHz = 157 TFLOP/s); traffic: 4 heads x 64 channels x 4 bytes read twice and written once plus the
            targets, about 3.1 KB per pixel at 8 TB/s.  The larger of the two.

Inputs: random non-negative features, normal weights, Bernoulli(0.55) foreground, uniform classes; the leaves are the five feature maps and
the ten head parameters.  Device events around windows of INNER steps, the two sides alternating in the same run, median of REPS windows
after WARM warm-up windows.  Peak extra memory: torch.cuda.max_memory_allocated over one step minus what is allocated before it (inputs,
parameters), gradients of the leaves included on both sides.  The clock state is recorded as `rocm-smi --showclocks` prints it (a query).

usage: python tools/css_train_time.py OUT_DIR            (writes OUT_DIR/css_train_time.json)
       python tools/css_train_time.py --once fused|torch_ops B     (a few steps of one side, for a kernel trace under rocprofv3)
"""
import json
import os
import subprocess
import sys

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from sdflabel_amd import css  # noqa: E402

DEV = "cuda:0"
WARM, REPS, INNER = 2, 7, 5
PEAK_FLOPS, PEAK_BYTES = 256 * 4 * 64 * 2.4e9, 8.0e12
HEADS = ("u", "v", "w", "mask")


def inputs(B, seed=1):
    g = torch.Generator(device=DEV).manual_seed(seed)
    leaf = lambda *s, scale=1.0, absolute=False: ((torch.randn(*s, device=DEV, generator=g).abs() if absolute else       # noqa: E731
                                                   torch.randn(*s, device=DEV, generator=g)) * scale).requires_grad_(True)
    x = {h: leaf(B, 64, 128, 128, absolute=True) for h in HEADS}
    w = {h: (leaf(2 if h == "mask" else 256, 64, 1, 1, scale=0.09), leaf(2 if h == "mask" else 256, scale=0.1)) for h in HEADS}
    x4, wl, bl = leaf(B, 256, 8, 8, absolute=True), leaf(3, 256, 1, 1, scale=0.1), leaf(3, scale=0.05)
    mask = (torch.rand(B, 128, 128, device=DEV, generator=g) < 0.55).long()
    uvw = torch.randint(0, 256, (B, 3, 128, 128), device=DEV, generator=g) * mask[:, None]
    gt = F.normalize(torch.randn(B, 3, device=DEV, generator=g), dim=1)
    return x, w, (x4, wl, bl), uvw, mask, gt


def leaves(x, w, lat):
    return list(x.values()) + [t for wb in w.values() for t in wb] + list(lat)


def step_fused(x, w, lat, uvw8, mask8, gt):
    lh = css.css_head_loss(x["u"], x["v"], x["w"], x["mask"], w, uvw8, mask8)
    loss = lh["u"] + lh["v"] + lh["w"] + lh["mask"] + css.css_latent_loss(*lat, gt)
    loss.backward()
    return loss


def step_torch(x, w, lat, uvw, mask, gt):
    ce, mse = nn.CrossEntropyLoss(), nn.MSELoss()
    loss = 0
    for i, h in enumerate(("u", "v", "w")):
        lp = F.log_softmax(F.conv2d(x[h], *w[h]), dim=1)
        loss = loss + ce(lp * mask.unsqueeze(1).expand_as(lp).float(), uvw[:, i] * mask)
    loss = loss + ce(F.conv2d(x["mask"], *w["mask"]), mask) * 2
    v = F.conv2d(*lat).flatten(2).mean(dim=2)
    loss = loss + mse(v * (1.0 / (v.norm(dim=1, keepdim=True).detach() + 1e-8)), gt)
    loss.backward()
    return loss


def clear(ts):
    for t in ts:
        t.grad = None


def alternate(a, b):
    def window(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(INNER):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / INNER
    for _ in range(WARM):
        window(a), window(b)
    ta, tb = [], []
    for _ in range(REPS):
        ta.append(window(a))
        tb.append(window(b))
    stat = lambda v: {"median_ms": round(float(np.median(v)), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}      # noqa: E731
    return stat(ta), stat(tb)


def peak_extra(fn, ts):
    clear(ts)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    clear(ts)
    return int(peak)


def clocks():
    try:
        return subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=30).stdout.strip().splitlines()
    except Exception as e:                                                                                              # noqa: BLE001
        return ["rocm-smi --showclocks: %s" % e]


def sides(B):
    x, w, lat, uvw, mask, gt = inputs(B)
    ts = leaves(x, w, lat)
    uvw8, mask8 = uvw.to(torch.uint8), mask.to(torch.uint8)

    def fused():
        clear(ts)
        return step_fused(x, w, lat, uvw8, mask8, gt)

    def plain():
        clear(ts)
        return step_torch(x, w, lat, uvw, mask, gt)
    return fused, plain, ts, x, w


def main():
    assert torch.cuda.is_available(), "css_train_time.py measures on the GPU only"
    if len(sys.argv) > 1 and sys.argv[1] == "--once":
        fused, plain, ts, _, _ = sides(int(sys.argv[3]))
        fn = fused if sys.argv[2] == "fused" else plain
        for _ in range(4):
            fn()
        torch.cuda.synchronize()
        return
    out_dir = sys.argv[1] if len(sys.argv) > 1 else "."
    os.makedirs(out_dir, exist_ok=True)
    res = {"config": "device events around windows of %d steps; the two sides alternate in the same run; median of %d windows after %d warm-up "
                     "windows; 128 x 128 crops, float32; a step is the head's losses and their backward to the five feature maps and the ten "
                     "head parameters" % (INNER, REPS, WARM), "device": torch.cuda.get_device_name(0), "clocks_before": clocks(), "sizes": {}}
    for B in (16, 32):
        fused, plain, ts, x, w = sides(B)
        la, lb = float(fused()), float(plain())
        ga = [t.grad.clone() for t in ts]
        plain()
        diff = max(float((a - t.grad).abs().max()) for a, t in zip(ga, ts))
        del ga
        tf, tp = alternate(fused, plain)
        mf, mp = peak_extra(fused, ts), peak_extra(plain, ts)
        pix = B * 128 * 128
        flops, byts = pix * 4 * 98304, pix * (4 * 64 * 4 * 3 + 4 + 12)
        floor_ms = max(flops / PEAK_FLOPS, byts / PEAK_BYTES) * 1e3
        wide = pix * 256 * 4
        res["sizes"]["B%d" % B] = {"fused": tf, "torch_ops": tp, "torch_over_fused": round(tp["median_ms"] / tf["median_ms"], 2),
                                   "floor_ms": round(floor_ms, 4), "floor_bound": "exact-f32 MFMA" if flops / PEAK_FLOPS > byts / PEAK_BYTES else "HBM",
                                   "fused_over_floor": round(tf["median_ms"] / floor_ms, 2), "peak_extra_bytes_fused": mf,
                                   "peak_extra_bytes_torch_ops": mp, "bytes_of_one_B_256_H_W_tensor": wide,
                                   "published_workspace_bytes": css.head_loss_workspace_bytes(B, 128, 128),
                                   "loss_fused": la, "loss_torch_ops": lb, "largest_gradient_difference_between_the_sides": diff}
        print("B=%d" % B, json.dumps(res["sizes"]["B%d" % B]))
        del fused, plain, ts, x, w
        torch.cuda.empty_cache()
    res["clocks_after"] = clocks()
    json.dump(res, open(os.path.join(out_dir, "css_train_time.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
