"""Golden G21 (tests/golden/g21_css_train.npz): the training losses of the CSS head and their gradients, recorded from the reference's own
networks.resnet_css.ResNet (tools/_ref_import.py: read-only) on the CPU.  Only DATA is committed: targets and recorded results.

The head's inputs and weights are G20's (tests/golden/g20_css_head.npz: x, the five captured feature maps and w_* / b_*); they are read from
that file and not stored again.  As in G20's float64 run, the five output convolutions are fed the captured float32 features through forward
pre-hooks -- here as leaf tensors, so that their gradients are those of the head alone.  pipelines/train_css.py:71-80 of the reference sits
inside its training loop and cannot be called; this tool restates those lines with the same torch criteria (nn.CrossEntropyLoss,
nn.MSELoss) on the reference module's own outputs.

Targets (numpy default_rng(21)):
  mask_gt    Bernoulli(1/2) per pixel: independent of the predicted mask; the generator REFUSES a foreground share outside 30 ... 70 % or a
             mask_gt equal to the prediction
  uvw_gt     uniform 0 ... 255, zeroed on the background; the first two foreground pixels of every channel are set to 0 and 255, and the
             generator checks both classes are present on the foreground
  latent_gt  normal, scaled to the unit sphere
Recorded: the float32 losses (loss_u, loss_v, loss_w, loss_mask, loss_lat), the float32 gradients of the five head inputs (dx_*) and the ten
head parameters (dw_*, db_*), and err_* = [max, rms] of each against the same run in float64 (.double() module, the same float32 features).
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _ref_import  # noqa: E402

_ref_import.setup()

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, ".."))
G20 = os.path.join(ROOT, "tests", "golden", "g20_css_head.npz")
OUT = os.path.join(ROOT, "tests", "golden", "g21_css_train.npz")
HEAD_OF = {"x4": "out_lat", "x_u": "out_u", "x_v": "out_v", "x_w": "out_w", "x_mask": "out_mask"}
NAME = {"x4": "lat", "x_u": "u", "x_v": "v", "x_w": "w", "x_mask": "mask"}


def run(net, x, feats, uvw_gt, mask_gt, latent_gt, dtype):
    """the reference's forward with the head fed `feats` as leaves, its losses and their gradients: {name: numpy array}"""
    net = net.to(dtype)
    leaves = {k: v.detach().clone().to(dtype).requires_grad_(True) for k, v in feats.items()}
    hooks = [getattr(net, HEAD_OF[k]).register_forward_pre_hook(lambda m, i, k=k: (leaves[k],)) for k in leaves]
    pred = net(x.to(dtype))
    for h in hooks:
        h.remove()
    criterion_mse, criterion_ce = nn.MSELoss(), nn.CrossEntropyLoss()
    u_pred, v_pred, w_pred, mask_pred, lat_pred = pred['u'], pred['v'], pred['w'], pred['mask'], pred['latent']
    mask_gt_ext = mask_gt.unsqueeze(1).expand_as(u_pred).to(dtype)
    losses = {"loss_u": criterion_ce(u_pred * mask_gt_ext, uvw_gt[:, 0] * mask_gt),
              "loss_v": criterion_ce(v_pred * mask_gt_ext, uvw_gt[:, 1] * mask_gt),
              "loss_w": criterion_ce(w_pred * mask_gt_ext, uvw_gt[:, 2] * mask_gt),
              "loss_mask": criterion_ce(mask_pred, mask_gt) * 2,
              "loss_lat": criterion_mse(lat_pred.squeeze(0), latent_gt.to(dtype))}
    loss = losses["loss_u"] + losses["loss_v"] + losses["loss_w"] + losses["loss_lat"] + losses["loss_mask"]
    net.zero_grad()
    loss.backward()
    res = {k: v.detach().numpy().copy() for k, v in losses.items()}
    for k, leaf in leaves.items():
        conv = getattr(net, HEAD_OF[k]).conv
        res["dx_" + NAME[k]] = leaf.grad.numpy().copy()
        res["dw_" + NAME[k]] = conv.weight.grad.numpy().reshape(conv.weight.shape[0], -1).copy()
        res["db_" + NAME[k]] = conv.bias.grad.numpy().copy()
    res["pred_fg"] = (mask_pred[:, 1] > mask_pred[:, 0]).numpy()
    return res


def main():
    from networks.resnet_css import resnet18                       # the reference's
    g20 = np.load(G20)
    torch.manual_seed(1)
    net = resnet18(pretrained=False).eval()
    with torch.no_grad():
        for h in ("u", "v", "w", "mask", "lat"):
            conv = getattr(net, "out_" + h).conv
            conv.weight.copy_(torch.from_numpy(g20["w_" + h]).view_as(conv.weight))
            conv.bias.copy_(torch.from_numpy(g20["b_" + h]))
    x = torch.from_numpy(g20["x"])
    feats = {k: torch.from_numpy(g20[k]) for k in HEAD_OF}
    B, _, H, W = g20["x_u"].shape
    rng = np.random.default_rng(21)
    mask = (rng.random((B, H, W)) < 0.5)
    uvw = rng.integers(0, 256, (B, 3, H, W))
    for c in range(3):
        fg = np.argwhere(mask)
        uvw[fg[0][0], c, fg[0][1], fg[0][2]] = 0
        uvw[fg[1][0], c, fg[1][1], fg[1][2]] = 255
    uvw = uvw * mask[:, None]
    lat = rng.standard_normal((B, 3))
    lat /= np.linalg.norm(lat, axis=1, keepdims=True)
    share = float(mask.mean())
    if not 0.3 <= share <= 0.7:
        raise SystemExit("foreground share %.3f outside [0.3, 0.7]: refused" % share)
    for c in range(3):
        on_fg = uvw[:, c][mask]
        if not ((on_fg == 0).any() and (on_fg == 255).any()):
            raise SystemExit("classes 0 and 255 must both be present on the foreground: refused")
    uvw_t, mask_t, lat_t = torch.from_numpy(uvw).long(), torch.from_numpy(mask).long(), torch.from_numpy(lat.astype(np.float32))
    r32 = run(net, x, feats, uvw_t, mask_t, lat_t, torch.float32)
    r64 = run(net, x, feats, uvw_t, mask_t, lat_t.double(), torch.float64)
    if np.array_equal(r32["pred_fg"], mask):
        raise SystemExit("mask_gt equals the predicted mask: refused")
    z = {"uvw_gt": uvw.astype(np.uint8), "mask_gt": mask.astype(np.uint8), "latent_gt": lat.astype(np.float32), "foreground_share": np.float64(share),
         "mask_gt_differs_from_prediction": np.float64((r32["pred_fg"] != mask).mean())}
    for k in sorted(r32):
        if k == "pred_fg":
            continue
        d = r32[k].astype(np.float64) - r64[k]
        z[k] = r32[k]
        z["err_" + k] = np.array([np.abs(d).max(), np.sqrt((d * d).mean())])
        print("%-10s %-18s float32 against float64: max %.3e rms %.3e (largest value %.3e)" % (k, r32[k].shape, z["err_" + k][0], z["err_" + k][1],
                                                                                               np.abs(r64[k]).max()))
    np.savez_compressed(OUT, **z)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))
    if os.path.getsize(OUT) >= 1 << 20:
        raise SystemExit("the file must stay below 1 MiB")


if __name__ == "__main__":
    main()
