"""GPU timing of the CSS network's output head at B = 1, 8, 16 crops of 128 x 128.

head        sdflabel_amd.css.css_head + css_latent on the features of the drop-in network (seed 1, eval mode, random input) against the same
            features through plain torch ops, written as the reference's tail (1x1 convolutions, log_softmax, softmax(100 .), sum k p, argmax).
forward     the whole network: ResNet.forward (features + the two fused launches) against features + the torch tail.
floor       the least time the hardware could take for the fused head: 2 * 64 * 768 FLOP per pixel at the exact-f32 MFMA peak (256 CUs x 4
            SIMDs x 64 FLOP per clock at 2.4 GHz = 157 TFLOP/s) and 4 * 64 * 4 + 9 * 4 bytes per pixel at 8 TB/s; the larger of the two.

Device events around windows of INNER calls, the two sides alternating in the same run, median of REPS windows after WARM warm-up windows;
every shape is warmed up first (MIOpen picks its algorithms on the first call).  The two sides' uvw_sm are compared at every size.

usage: python tools/css_time.py OUT_DIR          (writes OUT_DIR/css_time.json)
"""
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from sdflabel_amd import css  # noqa: E402
from sdflabel_amd.networks.resnet_css import setup_css  # noqa: E402

DEV = "cuda:0"
WARM, REPS, INNER = 2, 9, 10
PEAK_FLOPS, PEAK_BYTES = 256 * 4 * 64 * 2.4e9, 8.0e12


def torch_tail(net, f):
    """networks/resnet_css.py:194-196, :203-249 of the reference in torch ops, on the captured features"""
    out = {}
    lat = net.out_lat(f['x4'])
    lat = lat.view(lat.size(0), lat.size(1), -1).mean(dim=2)
    out['latent'] = lat * (1.0 / (lat.norm(dim=1, keepdim=True) + 1e-8))
    colors = torch.arange(256, device=f['x4'].device, dtype=f['x4'].dtype).view(1, 256, 1, 1)
    cols = []
    for h in ('u', 'v', 'w'):
        lp = F.log_softmax(getattr(net, 'out_' + h)(f['x_' + h]), dim=1)
        out[h] = lp
        cols.append(torch.sum(colors * torch.softmax(lp * 100, dim=1), dim=1, keepdim=True))
    out['uvw_sm'] = torch.cat(cols, dim=1)
    mask = net.out_mask(f['x_mask'])
    out['mask'] = mask
    out['mask_sm'] = torch.softmax(mask * 100, dim=1)[:, 1:2]
    out['uvw_sm_masked'] = out['uvw_sm'] * mask.argmax(dim=1, keepdim=True).expand_as(out['uvw_sm']).float()
    return out


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


def main():
    out_dir = sys.argv[1] if len(sys.argv) > 1 else "."
    os.makedirs(out_dir, exist_ok=True)
    assert torch.cuda.is_available(), "css_time.py measures on the GPU only"
    torch.manual_seed(1)
    net = setup_css(mode="eval").to(DEV)
    with torch.no_grad():
        net.out_mask.conv.bias.copy_(torch.tensor([0.0, 10.0]))         # a random mask head marks nothing
    res = {"config": "device events around windows of %d calls; the two sides alternate in the same run; median of %d windows after %d warm-up "
                     "windows; 128 x 128 crops, float32, eval mode, random weights of seed 1" % (INNER, REPS, WARM), "sizes": {}}
    for B in (1, 8, 16):
        x = torch.randn(B, 3, 128, 128, device=DEV)
        with torch.no_grad():
            f = {k: v.contiguous() for k, v in net.features(x).items()}
            w = net.head_weights()
            fused = lambda: (css.css_head(f['x_u'], f['x_v'], f['x_w'], f['x_mask'], w),                      # noqa: E731
                             css.css_latent(f['x4'], net.out_lat.conv.weight, net.out_lat.conv.bias))
            plain = lambda: torch_tail(net, f)                                                                # noqa: E731
            whole_fused = lambda: net(x)                                                                      # noqa: E731
            whole_plain = lambda: torch_tail(net, net.features(x))                                            # noqa: E731
            a, b = fused()[0], plain()
            diff = float((a['uvw_sm'] - b['uvw_sm']).abs().max())
            same_mask = bool(torch.equal(a['uvw_sm_masked'] != 0, b['uvw_sm_masked'] != 0))
            th, tp = alternate(fused, plain)
            tw, tq = alternate(whole_fused, whole_plain)
        pix = B * 128 * 128
        floor_ms = max(pix * 2 * 64 * 768 / PEAK_FLOPS, pix * (4 * 64 * 4 + 9 * 4) / PEAK_BYTES) * 1e3
        res["sizes"]["B%d" % B] = {"head_fused": th, "head_torch_ops": tp, "forward_fused": tw, "forward_torch_ops": tq,
                                   "floor_ms": round(floor_ms, 4), "floor_bound": "exact-f32 MFMA", "gflop": round(pix * 2 * 64 * 768 / 1e9, 2),
                                   "gbytes": round(pix * (4 * 64 * 4 + 9 * 4) / 1e9, 3), "fused_over_floor": round(th["median_ms"] / floor_ms, 2),
                                   "max_uvw_sm_difference_between_the_sides": diff, "same_foreground_pixels": same_mask}
        print("B=%d" % B, json.dumps(res["sizes"]["B%d" % B]))
    json.dump(res, open(os.path.join(out_dir, "css_time.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
