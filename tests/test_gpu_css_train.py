"""Training the CSS head on the GPU (csrc/css_train.hip through sdflabel_amd.css, networks.resnet_css.ResNet.loss and pipelines.train_css)
against the float64 restatement of tests/_css_train_ref.py, which tests/test_css_train_cpu.py pins to golden G21 (recorded from the
reference's own module) and to torch's float64 autograd.  The tolerances are the derived ones of _css_train_ref; figures are printed before
they are asserted."""
import numpy as np
import pytest
import torch

from sdflabel_amd import _lib, css
from tests import _css_ref as R
from tests import _css_train_ref as T
from tests._util import gold

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HEADS = ("u", "v", "w", "mask")
LN256 = float(np.log(256.0))


def dev(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def synthetic(B, H, W, seed=1, scale=1.0, fg=0.55):
    """non-negative features (the head's inputs follow a ReLU), normal weights, one head in the mixing regime, random targets"""
    g = np.random.default_rng(seed)
    x = {k: (np.abs(g.standard_normal((B, 64, H, W))) * scale).astype(np.float32) for k in ("x_u", "x_v", "x_w", "x_mask")}
    wts = {h: ((g.standard_normal((256, 64)) * 0.09).astype(np.float32), (g.uniform(-0.125, 0.125, 256)).astype(np.float32)) for h in ("u", "v", "w")}
    wts["v"] = (wts["v"][0] * 0.05, wts["v"][1] * 0.05)
    wts["mask"] = ((g.standard_normal((2, 64)) * 0.1).astype(np.float32), g.uniform(-0.125, 0.125, 2).astype(np.float32))
    mask = (g.random((B, H, W)) < fg).astype(np.uint8)
    uvw = (g.integers(0, 256, (B, 3, H, W)) * mask[:, None]).astype(np.uint8)
    return x, wts, uvw, mask


def flat(r):
    out = {}
    loss = r["loss"].cpu().numpy()
    for i, h in enumerate(HEADS):
        out["loss_" + h] = loss[i]
        out["dx_" + h], out["dw_" + h], out["db_" + h] = (r[k][h].cpu().numpy() for k in ("dx", "dw", "db"))
    return out


def run(x, wts, uvw, mask):
    r = css.head_loss_raw(dev(x["x_u"]), dev(x["x_v"]), dev(x["x_w"]), dev(x["x_mask"]), {h: (dev(w), dev(b)) for h, (w, b) in wts.items()},
                          dev(uvw, np.uint8), dev(mask, np.uint8))
    return flat(r)


def run_latent(x4, wl, bl, gt):
    r = css.latent_loss_raw(dev(x4), dev(wl), dev(bl), dev(gt))
    return {"loss_lat": r["loss"].cpu().numpy()[0], "dx_lat": r["dx"].cpu().numpy(), "dw_lat": r["dw"].cpu().numpy(), "db_lat": r["db"].cpu().numpy()}


def ref(x, wts, uvw, mask):
    return T.head_loss(x["x_u"], x["x_v"], x["x_w"], x["x_mask"], wts, uvw, mask)


def background_is_zero(got, mask):
    for h in ("u", "v", "w"):
        d = got["dx_" + h]
        assert (d[np.broadcast_to(mask[:, None] == 0, d.shape)] == 0).all(), h


def test_golden_g21_through_the_fused_losses():
    z, t = gold("g20_css_head.npz"), gold("g21_css_train.npz")
    x = {k: z[k] for k in ("x_u", "x_v", "x_w", "x_mask")}
    wts = {h: (z["w_" + h], z["b_" + h]) for h in HEADS}
    got = run(x, wts, t["uvw_gt"], t["mask_gt"])
    got.update(run_latent(z["x4"], z["w_lat"], z["b_lat"], t["latent_gt"]))
    out, tol = ref(x, wts, t["uvw_gt"], t["mask_gt"])
    o, tl = T.latent_loss(z["x4"], z["w_lat"], z["b_lat"], t["latent_gt"])
    out.update(o)
    tol.update(tl)
    T.compare(got, out, tol, label="g21:")
    background_is_zero(got, t["mask_gt"])
    for k in ("dw_u", "dx_u", "loss_u"):                    # for the record: the kernel's error next to the reference's own float32 error
        e = float(np.abs(got[k].astype(np.float64) - out[k]).max())
        print("g21: %-7s error against float64 %.3e, the reference's float32 %.3e" % (k, e, float(t["err_" + k][0])))


@pytest.mark.parametrize("B,H,W", [(1, 1, 1), (3, 5, 7), (2, 12, 13), (3, 31, 33)])
def test_synthetic_shapes(B, H, W):
    x, wts, uvw, mask = synthetic(B, H, W)
    if B * H * W == 1:
        mask[:] = 1
        uvw[:] = 77
    got = run(x, wts, uvw, mask)
    out, tol = ref(x, wts, uvw, mask)
    T.compare(got, out, tol, label="%dx%dx%d:" % (B, H, W))
    background_is_zero(got, mask)


@pytest.mark.parametrize("B,h,w", [(1, 1, 1), (3, 3, 5), (2, 17, 19)])
def test_latent_shapes(B, h, w):
    g = np.random.default_rng(1)
    x4 = np.abs(g.standard_normal((B, 256, h, w))).astype(np.float32)
    wl, bl = (g.standard_normal((3, 256)) * 0.1).astype(np.float32), g.uniform(-0.06, 0.06, 3).astype(np.float32)
    gt = g.standard_normal((B, 3))
    gt = (gt / np.linalg.norm(gt, axis=1, keepdims=True)).astype(np.float32)
    got = run_latent(x4, wl, bl, gt)
    out, tol = T.latent_loss(x4, wl, bl, gt)
    T.compare(got, out, tol, label="latent %dx%dx%d:" % (B, h, w))
    again = run_latent(x4, wl, bl, gt)
    for k in got:
        assert np.asarray(got[k]).tobytes() == np.asarray(again[k]).tobytes(), k


@pytest.mark.parametrize("kind", ["background", "foreground", "class0", "class255"])
def test_edge_targets(kind):
    x, wts, uvw, mask = synthetic(2, 5, 7)
    if kind == "background":
        mask[:] = 0
        uvw[:] = 0
    elif kind == "foreground":
        mask[:] = 1
        uvw = np.random.default_rng(3).integers(0, 256, uvw.shape).astype(np.uint8)
    else:
        uvw = (np.full(uvw.shape, 0 if kind == "class0" else 255) * mask[:, None]).astype(np.uint8)
    got = run(x, wts, uvw, mask)
    out, tol = ref(x, wts, uvw, mask)
    T.compare(got, out, tol, label=kind + ":")
    background_is_zero(got, mask)
    if kind == "background":
        for h in ("u", "v", "w"):
            assert (got["dx_" + h] == 0).all() and (got["dw_" + h] == 0).all() and (got["db_" + h] == 0).all()
            print("background: loss_%s - ln 256 = %.3e (tolerance %.3e)" % (h, got["loss_" + h] - LN256, tol["loss_" + h]))
            assert abs(float(got["loss_" + h]) - LN256) <= tol["loss_" + h]
        assert (got["dx_mask"] != 0).any()


def test_large_logits_stay_finite():
    x, wts, uvw, mask = synthetic(2, 5, 7, seed=2)
    lg, _ = R._logits(x["x_u"], *wts["u"])
    s = np.float32(300.0 / np.abs(lg).max())
    x = {k: v * s for k, v in x.items()}
    wts["v"] = (wts["v"][0] * 20, wts["v"][1])
    big = max(np.abs(R._logits(x["x_" + h], *wts[h])[0]).max() for h in ("u", "v", "w"))
    print("largest |logit| %.1f" % big)
    assert big > 250
    got = run(x, wts, uvw, mask)
    assert all(np.isfinite(v).all() for v in got.values())
    out, tol = ref(x, wts, uvw, mask)
    T.compare(got, out, tol, label="large:")


def test_a_crop_alone_is_its_share_of_the_batch():
    x, wts, uvw, mask = synthetic(3, 12, 13)
    three = run(x, wts, uvw, mask)
    one = run({k: v[1:2] for k, v in x.items()}, wts, uvw[1:2], mask[1:2])
    _, tol3 = ref(x, wts, uvw, mask)
    _, tol1 = ref({k: v[1:2] for k, v in x.items()}, wts, uvw[1:2], mask[1:2])
    for h in HEADS:
        k = "dx_" + h
        err = np.abs(one[k].astype(np.float64) - 3.0 * three[k][1:2].astype(np.float64))          # N of the batch / N of the crop = 3
        t = tol1[k] + 3.0 * tol3[k][1:2]
        ratio = np.where(t > 0, err / np.where(t > 0, t, 1.0), 0.0)                                # (t = 0 and err = 0 on the background)
        print("%s alone against 3 x its part of the batch: max %.3e, largest error / tolerance %.3f" % (k, err.max(), ratio.max()))
        assert (err <= t).all()


def test_two_calls_return_the_same_bytes():
    x, wts, uvw, mask = synthetic(3, 31, 33)
    a, b = run(x, wts, uvw, mask), run(x, wts, uvw, mask)
    for k in a:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k


def test_upstream_scalars_scale_each_head():
    x, wts, uvw, mask = synthetic(2, 5, 7)
    unit = run(x, wts, uvw, mask)
    xs = [dev(x[k]).requires_grad_(True) for k in ("x_u", "x_v", "x_w", "x_mask")]
    w = {h: (dev(a).view(a.shape[0], 64, 1, 1).requires_grad_(True), dev(b).requires_grad_(True)) for h, (a, b) in wts.items()}
    losses = css.css_head_loss(*xs, w, dev(uvw, np.int64), dev(mask, np.int64))          # the dataset's int64 targets
    assert sorted(losses) == ["mask", "u", "v", "w"] and all(v.dim() == 0 and v.requires_grad for v in losses.values())
    up = {"u": 2.0, "v": 0.0, "w": -1.0, "mask": 0.5}
    sum(losses[h] * up[h] for h in HEADS).backward()
    for i, h in enumerate(HEADS):
        assert float(losses[h]) == float(unit["loss_" + h])
        assert np.array_equal(xs[i].grad.cpu().numpy(), unit["dx_" + h] * np.float32(up[h])), h
        assert tuple(w[h][0].grad.shape) == tuple(w[h][0].shape)
        assert np.array_equal(w[h][0].grad.cpu().numpy().reshape(unit["dw_" + h].shape), unit["dw_" + h] * np.float32(up[h])), h
        assert np.array_equal(w[h][1].grad.cpu().numpy(), unit["db_" + h] * np.float32(up[h])), h
    # the same refusals as css_head
    ok = [t.detach() for t in xs]
    wd = {h: (a.detach(), b.detach()) for h, (a, b) in w.items()}
    tg = (dev(uvw, np.uint8), dev(mask, np.uint8))
    with pytest.raises(_lib.SdfrError, match="float32"):
        css.css_head_loss(ok[0].half(), *ok[1:], wd, *tg)
    with pytest.raises(_lib.SdfrError, match="64"):
        css.css_head_loss(*(v[:, :32].contiguous() for v in ok), wd, *tg)
    cl = torch.zeros(2, 64, 5, 7, device=DEV).contiguous(memory_format=torch.channels_last)
    with pytest.raises(_lib.SdfrError, match="contiguous"):
        css.css_head_loss(ok[0], cl, ok[2], ok[3], wd, *tg)
    with pytest.raises(_lib.SdfrError, match="uint8 or int64"):
        css.css_head_loss(*ok, wd, tg[0].float(), tg[1])
    with pytest.raises(_lib.SdfrError, match="float32"):
        css.css_latent_loss(torch.zeros(1, 256, 2, 2, device=DEV, dtype=torch.float16), torch.zeros(3, 256), torch.zeros(3), torch.zeros(1, 3, device=DEV))
    empty = css.css_head_loss(*(v[:0] for v in ok), wd, tg[0][:0], tg[1][:0])
    assert all(v.dim() == 0 for v in empty.values())


def batch_16(seed=4):
    g = torch.Generator().manual_seed(seed)
    mask = (torch.rand(2, 16, 16, generator=g) < 0.6).long()
    gt = torch.randn(2, 3, generator=g)
    return {"rgb": torch.randn(2, 3, 16, 16, generator=g), "mask": mask, "uvw": torch.randint(0, 256, (2, 3, 16, 16), generator=g) * mask[:, None],
            "latent": gt / gt.norm(dim=1, keepdim=True)}


def test_network_loss_reaches_every_trainable_parameter():
    from sdflabel_amd.networks.resnet_css import setup_css
    torch.manual_seed(1)
    net = setup_css(mode="train").to(DEV)
    b = {k: v.to(DEV) for k, v in batch_16().items()}
    losses = net.loss(b["rgb"], b["uvw"], b["mask"], b["latent"])
    assert sorted(losses) == ["latent", "loss", "mask", "uvw"]
    assert abs(float(losses["loss"]) - float(losses["uvw"] + losses["mask"] + losses["latent"])) <= 1e-6 * abs(float(losses["loss"]))
    losses["loss"].backward()
    used = [n for n, p in net.named_parameters() if not n.startswith("layer4.")]           # layer4 is never run (kept for the state_dict)
    missing = [n for n, p in net.named_parameters() if p.requires_grad and n in used and (p.grad is None or not bool(torch.isfinite(p.grad).all()))]
    assert not missing, missing
    assert bool((net.out_u.conv.weight.grad != 0).any()) and bool((net.layer2[0].conv1.weight.grad != 0).any())
    for frozen in (net.conv1, net.bn1, net.layer1):
        assert all(p.grad is None for p in frozen.parameters())
    with torch.no_grad():                                   # forward() stays the detached inference path
        assert all(not v.requires_grad for v in net(b["rgb"]).values())


def test_one_sgd_step_moves_the_head_by_the_restatement_gradient():
    from sdflabel_amd.networks.resnet_css import setup_css
    from sdflabel_amd.pipelines.train_css import train_step
    torch.manual_seed(1)
    net = setup_css(mode="train").to(DEV)
    lr = 1.0
    opt = torch.optim.SGD([p for p in net.parameters() if p.requires_grad], lr=lr)
    feats, hooks = {}, []
    for key, name in (("x4", "layer3"), ("x_u", "up4_u"), ("x_v", "up4_v"), ("x_w", "up4_w"), ("x_mask", "up4_mask")):
        hooks.append(getattr(net, name).register_forward_hook(lambda m, i, o, key=key: feats.__setitem__(key, o.detach().cpu().numpy())))
    before = {n: p.detach().cpu().numpy().copy() for n, p in net.named_parameters() if n.startswith("out_")}
    b = batch_16()
    got = train_step(net, opt, b)
    for h in hooks:
        h.remove()
    wts = {h: (before["out_%s.conv.weight" % h], before["out_%s.conv.bias" % h]) for h in HEADS}
    out, tol = T.head_loss(feats["x_u"], feats["x_v"], feats["x_w"], feats["x_mask"], wts, b["uvw"].numpy(), b["mask"].numpy())
    o, t = T.latent_loss(feats["x4"], before["out_lat.conv.weight"], before["out_lat.conv.bias"], b["latent"].numpy())
    out.update(o)
    tol.update(t)
    total = sum(float(out["loss_" + h]) for h in HEADS) + float(out["loss_lat"])
    print("train_step loss %.6f, restatement %.6f" % (float(got["loss"]), total))
    assert abs(float(got["loss"]) - total) <= sum(float(tol["loss_" + h]) for h in HEADS) + float(tol["loss_lat"]) + 2.0 ** -21 * total
    for h in HEADS + ("lat",):
        for kind, name in (("dw", "weight"), ("db", "bias")):
            p0 = before["out_%s.conv.%s" % (h, name)].astype(np.float64)
            p1 = getattr(getattr(net, "out_" + h).conv, name).detach().cpu().numpy().astype(np.float64)
            want = -lr * out["%s_%s" % (kind, h)].reshape(p0.shape)
            err = np.abs((p1 - p0) - want)
            t = lr * tol["%s_%s" % (kind, h)].reshape(p0.shape) + 2.0 ** -23 * (np.abs(p0) + np.abs(want))      # the update's own two roundings
            print("out_%s.%s moved by at most %.3e; against -lr * grad: max %.3e, largest error / tolerance %.3f" % (h, name, np.abs(p1 - p0).max(),
                                                                                                                    err.max(), (err / t).max()))
            assert (err <= t).all() and np.abs(p1 - p0).max() > 0


@pytest.mark.parametrize("B", [2, 8])
def test_nothing_256_channels_wide_is_allocated(B):
    H = W = 64
    x, wts, uvw, mask = synthetic(B, H, W)
    args = [dev(x[k]) for k in ("x_u", "x_v", "x_w", "x_mask")] + [{h: (dev(w), dev(b)) for h, (w, b) in wts.items()}, dev(uvw, np.uint8),
                                                                  dev(mask, np.uint8)]
    css.head_loss_raw(*args)                                 # (the library is loaded and the kernels are on the device)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()                                 # no cached blocks of other sizes: every request below is served at its own size
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    r = css.head_loss_raw(*args)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    returned = sum(t.numel() * t.element_size() for t in [r["loss"]] + [r[k][h] for k in ("dx", "dw", "db") for h in HEADS])
    extra = peak - returned
    bound = css.head_loss_workspace_bytes(B, H, W)
    one_wide = 8 * 256 * 64 * 64 * 4
    print("B = %d: peak %d bytes, returned %d, extra %d; published workspace %d, one [8][256][64][64] tensor %d" % (B, peak, returned, extra, bound,
                                                                                                                 one_wide))
    # torch's caching allocator rounds a request up to 512 bytes and hands out a block up to 1 MiB larger than a request of more than
    # 10 MiB (it does not split off a remainder below 1 MiB): only the workspace is that large
    assert extra <= bound + (1 << 20) + 14 * 512
    assert bound == css.HEAD_LOSS_WORKSPACE_FIXED_BYTES + css.HEAD_LOSS_WORKSPACE_BYTES_PER_PIXEL * B * H * W
    assert extra < one_wide
