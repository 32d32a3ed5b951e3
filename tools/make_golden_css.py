"""Golden G20 (tests/golden/g20_css_head.npz): the CSS network's output head, recorded from the reference's own networks.resnet_css.ResNet
(tools/_ref_import.py: read-only) on the CPU.  Only DATA is committed: captured activations, the head's weights and recorded results.

  torch.manual_seed(1); resnet18(pretrained=False).eval(); x = torch.randn(2, 3, 16, 16)
Forward hooks on layer3 and up4_u / up4_v / up4_w / up4_mask capture the five inputs of the head.  The input is 16 x 16, not 32 x 32: the
three [2][256][H][W] log-probability outputs and the four [2][64][H][W] feature maps have to fit a committed file of less than 1 MiB.  For
the same reason u / v / w are stored at every LP_STRIDE-th pixel only (`lp_pix`, indices into the flattened H * W); every other output of the
forward is stored whole.

Weight adjustments (data written into the reference's module before the forward; the reference's code runs unchanged):
  out_mask  the random initialisation gives 0 % foreground, which would make uvw_sm_masked identically zero.  Its weights are redrawn
            (normal, seed 2) and the foreground bias set to put the median pixel on the boundary; the generator REFUSES unless the foreground
            share ends between 30 % and 70 %.
  out_v     weight and bias scaled by 0.05: one head in the mixing regime, where many classes carry weight.
  out_u, out_w stay as initialised.

Recorded next to the outputs:
  err_*            the reference's own float32 error in the head, as [max, rms] per output: against the same module in float64 (.double())
                   whose five output convolutions are fed the captured float32 features (forward pre-hooks), so that only the head's
                   arithmetic differs between the two runs
  sd_names / sd_shapes  the 354 state_dict entries (shapes padded with -1 to four dimensions)
  backbone_max_diff the largest difference between sdflabel_amd.networks.resnet_css's features() and the captured inputs with the reference's
                   state_dict loaded (strict=True), on the CPU; expected 0
  stats            foreground share and, per colour head, the share of pixels whose top-two logit gap is below 0.05
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _ref_import  # noqa: E402

_ref_import.setup()

import numpy as np  # noqa: E402
import torch  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, ".."))
OUT = os.path.join(ROOT, "tests", "golden", "g20_css_head.npz")
SIZE, LP_STRIDE = 16, 8
KEYS = ("uvw_sm", "uvw_sm_masked", "mask", "mask_sm", "latent", "u", "v", "w")
TAPS = {"x4": "layer3", "x_u": "up4_u", "x_v": "up4_v", "x_w": "up4_w", "x_mask": "up4_mask"}


HEAD_OF = {"x4": "out_lat", "x_u": "out_u", "x_v": "out_v", "x_w": "out_w", "x_mask": "out_mask"}


def run(net, x, feed=None):
    """forward with the five head inputs captured; with `feed` the five output convolutions are given THOSE inputs instead (cast to x.dtype)"""
    feats, hooks = {}, []
    for key, name in TAPS.items():
        hooks.append(getattr(net, name).register_forward_hook(lambda m, i, o, key=key: feats.__setitem__(key, o.detach().clone())))
        if feed is not None:
            hooks.append(getattr(net, HEAD_OF[key]).register_forward_pre_hook(lambda m, i, key=key: (feed[key].to(x.dtype),)))
    with torch.no_grad():
        out = net(x)
    for h in hooks:
        h.remove()
    return feats, {k: out[k].detach().clone() for k in KEYS}


def main():
    from networks.resnet_css import resnet18                       # the reference's
    torch.manual_seed(1)
    net = resnet18(pretrained=False).eval()
    x = torch.randn(2, 3, SIZE, SIZE)
    feats, _ = run(net, x)
    with torch.no_grad():
        g = torch.Generator().manual_seed(2)
        wm = torch.randn(2, 64, 1, 1, generator=g) * 0.1
        gap = (feats["x_mask"] * (wm[1] - wm[0]).view(1, 64, 1, 1)).sum(1)
        net.out_mask.conv.weight.copy_(wm)
        net.out_mask.conv.bias.copy_(torch.tensor([0.0, -float(gap.median())]))
        net.out_v.conv.weight.mul_(0.05)
        net.out_v.conv.bias.mul_(0.05)
    feats, out32 = run(net, x)
    _, out64 = run(net.double(), x.double(), feed=feats)        # the head alone in float64, on the float32 features
    net.float()
    fg = float((out32["mask"][:, 1] > out32["mask"][:, 0]).float().mean())
    if not 0.3 <= fg <= 0.7:
        raise SystemExit("foreground share %.3f outside [0.3, 0.7]: refused" % fg)
    z = {"x": x.numpy(), "foreground_share": np.float64(fg)}
    for k, v in feats.items():
        z[k] = v.numpy()
    for h in ("u", "v", "w", "mask", "lat"):
        conv = getattr(net, "out_" + h).conv
        z["w_" + h], z["b_" + h] = conv.weight.detach().numpy().reshape(conv.weight.shape[0], -1).copy(), conv.bias.detach().numpy().copy()
    lp_pix = np.arange(LP_STRIDE // 2, SIZE * SIZE, LP_STRIDE, dtype=np.int64)
    z["lp_pix"] = lp_pix
    gaps = []
    for k in KEYS:
        a32, a64 = out32[k].numpy(), out64[k].numpy()
        d = a32.astype(np.float64) - a64
        z["err_" + k] = np.array([np.abs(d).max(), np.sqrt((d * d).mean())])
        if k in ("u", "v", "w"):
            top = np.sort(a64, axis=1)[:, -2:]
            gaps.append(float(((top[:, 1] - top[:, 0]) < 0.05).mean()))
            a32 = a32.reshape(2, 256, -1)[:, :, lp_pix]
        z["out_" + k] = a32
        print("%-14s %s float32 against float64: max %.3e rms %.3e" % (k, a32.shape, z["err_" + k][0], z["err_" + k][1]))
    z["top_two_gap_below_0p05"] = np.array(gaps)
    print("foreground share %.3f; share of pixels with a top-two gap below 0.05 (u, v, w): %s" % (fg, gaps))
    sd = net.state_dict()
    z["sd_names"] = np.array(list(sd.keys()))
    z["sd_shapes"] = np.array([list(v.shape) + [-1] * (4 - v.dim()) for v in sd.values()], dtype=np.int64)
    print("%d state_dict entries, %d parameters" % (len(sd), sum(p.numel() for p in net.parameters())))
    # the drop-in's backbone on the same weights
    sys.path.insert(0, ROOT)
    from sdflabel_amd.networks import resnet_css as ours
    mine = ours.resnet18().eval()
    mine.load_state_dict(sd, strict=True)
    with torch.no_grad():
        f = mine.features(x)
    z["backbone_max_diff"] = np.float64(max(float((f[k] - feats[k]).abs().max()) for k in TAPS))
    print("backbone_max_diff %g" % z["backbone_max_diff"])
    np.savez_compressed(OUT, **z)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
