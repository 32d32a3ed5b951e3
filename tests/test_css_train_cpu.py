"""Training the CSS head without a GPU: golden G21 (tools/make_golden_css_train.py, recorded from the reference's own module and the torch
criteria of its training loop) against the float64 restatement of tests/_css_train_ref.py that the GPU tests measure against, the
restatement against torch float64 autograd of a plain-torch head, the detached-norm rule of the latent, the ABI and the import shim.
Figures are printed before they are asserted."""
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from sdflabel_amd import _lib
from tests import _css_train_ref as T
from tests._util import ROOT, gold

NEW = ("sdfr_css_head_loss", "sdfr_css_latent_loss")
NAMES = ("u", "v", "w", "mask")


@pytest.fixture(scope="module")
def z20():
    return gold("g20_css_head.npz")


@pytest.fixture(scope="module")
def z21():
    return gold("g21_css_train.npz")


def test_reference_float32_losses_and_gradients_lie_within_the_derived_tolerance(z20, z21):
    wts = {h: (z20["w_" + h], z20["b_" + h]) for h in NAMES}
    out, tol = T.head_loss(z20["x_u"], z20["x_v"], z20["x_w"], z20["x_mask"], wts, z21["uvw_gt"], z21["mask_gt"])
    o, t = T.latent_loss(z20["x4"], z20["w_lat"], z20["b_lat"], z21["latent_gt"])
    out.update(o)
    tol.update(t)
    got = {k: z21[k] for k in out}
    assert len(got) == 20
    res = T.compare(got, out, tol, label="reference float32:")
    assert set(res) == set(out)
    # the fixture exercises what it was built for
    m = z21["mask_gt"] != 0
    assert 0.3 <= float(m.mean()) <= 0.7 and float(z21["mask_gt_differs_from_prediction"]) > 0.1
    for c in range(3):
        on = z21["uvw_gt"][:, c][m]
        assert (on == 0).any() and (on == 255).any() and (z21["uvw_gt"][:, c][~m] == 0).all()
    assert np.abs(np.linalg.norm(z21["latent_gt"].astype(np.float64), axis=1) - 1).max() < 1e-6
    for h in ("u", "v", "w"):
        assert (z21["dx_" + h][np.broadcast_to(~m[:, None], z21["dx_" + h].shape)] == 0).all()      # exactly 0 on the background
        assert (out["dx_" + h][np.broadcast_to(~m[:, None], out["dx_" + h].shape)] == 0).all()
    for k in out:
        assert z21["err_" + k].shape == (2,) and 0 < z21["err_" + k][1] <= z21["err_" + k][0]


def plain_torch(x, wts, uvw_gt, mask_gt, x4, wl, bl, latent_gt, detach=True):
    """the training losses in plain torch, float64: conv, log_softmax, the mask product and the two criteria; returns {name: numpy}"""
    t = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64)).requires_grad_(True)       # noqa: E731
    ce, mse = nn.CrossEntropyLoss(), nn.MSELoss()
    mask = torch.from_numpy(np.asarray(mask_gt).astype(np.int64))
    uvw = torch.from_numpy(np.asarray(uvw_gt).astype(np.int64))
    res, total, leaves = {}, 0, {}
    for i, h in enumerate(NAMES):
        xx, w, b = t(x[h]), t(wts[h][0]), t(wts[h][1])
        leaves[h] = (xx, w, b)
        logits = F.conv2d(xx, w.view(w.shape[0], w.shape[1], 1, 1), b)
        if h == "mask":
            loss = ce(logits, mask) * 2
        else:
            loss = ce(F.log_softmax(logits, dim=1) * mask.unsqueeze(1).expand_as(logits).double(), uvw[:, i] * mask)
        res["loss_" + h] = loss
        total = total + loss
    xx, w, b = t(x4), t(wl), t(bl)
    leaves["lat"] = (xx, w, b)
    v = F.conv2d(xx, w.view(3, 256, 1, 1), b).flatten(2).mean(dim=2)
    n = torch.norm(v, dim=1, keepdim=True)
    lat = v * (1.0 / ((n.detach() if detach else n) + 1e-8))
    res["loss_lat"] = mse(lat, torch.from_numpy(np.asarray(latent_gt, dtype=np.float64)))
    (total + res["loss_lat"]).backward()
    out = {k: v.detach().numpy() for k, v in res.items()}
    for h, (xx, w, b) in leaves.items():
        out["dx_" + h], out["dw_" + h], out["db_" + h] = xx.grad.numpy(), w.grad.numpy(), b.grad.numpy()
    return out


def small_case(B, H, W, seed=5):
    g = np.random.default_rng(seed)
    x = {h: np.abs(g.standard_normal((B, 64, H, W))) for h in NAMES}
    wts = {h: (g.standard_normal((2 if h == "mask" else 256, 64)) * 0.09, g.uniform(-0.125, 0.125, 2 if h == "mask" else 256)) for h in NAMES}
    mask = (g.random((B, H, W)) < 0.6).astype(np.uint8)
    uvw = (g.integers(0, 256, (B, 3, H, W)) * mask[:, None]).astype(np.uint8)
    x4 = np.abs(g.standard_normal((B, 256, max(H // 2, 1), max(W // 2, 1))))
    wl, bl = g.standard_normal((3, 256)) * 0.1, g.uniform(-0.06, 0.06, 3)
    gt = g.standard_normal((B, 3))
    return x, wts, uvw, mask, x4, wl, bl, gt / np.linalg.norm(gt, axis=1, keepdims=True)


@pytest.mark.parametrize("B,H,W", [(1, 1, 1), (2, 5, 7)])
def test_restatement_is_torch_float64_autograd(B, H, W):
    x, wts, uvw, mask, x4, wl, bl, gt = small_case(B, H, W)
    ref = plain_torch(x, wts, uvw, mask, x4, wl, bl, gt)
    out, _ = T.head_loss(x["u"], x["v"], x["w"], x["mask"], wts, uvw, mask)
    out.update(T.latent_loss(x4, wl, bl, gt)[0])
    worst = 0.0
    for k in sorted(out):
        e = float(np.abs(np.asarray(out[k]).reshape(ref[k].shape) - ref[k]).max())
        worst = max(worst, e)
        print("%dx%dx%d %-10s |restatement - autograd| max %.3e" % (B, H, W, k, e))
    assert worst <= 1e-12


def test_latent_length_is_a_constant_of_the_backward():
    x, wts, uvw, mask, x4, wl, bl, gt = small_case(2, 5, 7)
    out, tol = T.latent_loss(x4, wl, bl, gt)
    kept = plain_torch(x, wts, uvw, mask, x4, wl, bl, gt, detach=True)
    full = plain_torch(x, wts, uvw, mask, x4, wl, bl, gt, detach=False)
    for k in ("dx_lat", "dw_lat", "db_lat"):
        e_kept = np.abs(out[k] - kept[k].reshape(out[k].shape))
        e_full = np.abs(out[k] - full[k].reshape(out[k].shape))
        print("%-7s detached norm: max %.3e; differentiated norm: max %.3e, %.1f x the float32 tolerance" % (k, e_kept.max(), e_full.max(),
                                                                                                             (e_full / tol[k]).max()))
        assert e_kept.max() <= 1e-12
        assert (e_full / tol[k]).max() > 100          # a properly differentiated normalisation is far outside the float32 tolerance
    assert abs(float(out["loss_lat"]) - float(full["loss_lat"])) <= 1e-12       # the value itself is the same


def test_new_entry_points_are_exported_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "sdfr.h")).read()
    h = _lib.lib()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _lib.EXPORTS and hasattr(h, name)
    assert int(re.search(r"#define SDFR_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION == h.sdfr_version() >= 407
    from sdflabel_amd import css
    assert callable(css.css_head_loss) and callable(css.css_latent_loss)
    assert int(re.search(r"#define SDFR_CSS_LOSS_WS_FIXED (\d+)ll", header).group(1)) == css.HEAD_LOSS_WORKSPACE_FIXED_BYTES
    # argument validation happens before any HIP call
    a = [None] * 34
    a[32] = 0
    a[4:8] = [1, 32, 4, 4]
    assert h.sdfr_css_head_loss(*a) == -1 and b"64" in h.sdfr_last_error()
    a[4:8] = [1, 64, 4, 4]
    assert h.sdfr_css_head_loss(*a) == -1 and b"NULL" in h.sdfr_last_error()
    a[4:8] = [0, 64, 4, 4]
    assert h.sdfr_css_head_loss(*a) == 0
    a[4:8] = [1, 64, 0, 4]
    assert h.sdfr_css_head_loss(*a) == 0
    lat = lambda B, C, hh: [None, B, C, hh, 2] + [None] * 8 + [0, None]      # noqa: E731
    assert h.sdfr_css_latent_loss(*lat(1, 64, 2)) == -1 and b"256" in h.sdfr_last_error()
    assert h.sdfr_css_latent_loss(*lat(1, 256, 2)) == -1 and b"NULL" in h.sdfr_last_error()
    assert h.sdfr_css_latent_loss(*lat(0, 256, 2)) == 0 and h.sdfr_css_latent_loss(*lat(2, 256, 0)) == 0
    # the Python boundary refuses host tensors
    x = torch.zeros(1, 64, 4, 4)
    w = {k: (torch.zeros(2 if k == "mask" else 256, 64), torch.zeros(2 if k == "mask" else 256)) for k in NAMES}
    with pytest.raises(_lib.SdfrError):
        css.css_head_loss(x, x, x, x, w, torch.zeros(1, 3, 4, 4, dtype=torch.uint8), torch.zeros(1, 4, 4, dtype=torch.uint8))
    with pytest.raises(_lib.SdfrError):
        css.css_latent_loss(torch.zeros(1, 256, 2, 2), torch.zeros(3, 256), torch.zeros(3), torch.zeros(1, 3))


def test_network_and_pipeline_expose_the_training_path():
    from sdflabel_amd.networks.resnet_css import setup_css
    from sdflabel_amd.pipelines import train_css as P
    net = setup_css(mode="train")
    assert callable(net.loss) and callable(P.train_step) and callable(P.train_css)
    with pytest.raises(_lib.SdfrError):                                    # no host computation of the losses
        net.loss(torch.zeros(2, 3, 16, 16), torch.zeros(2, 3, 16, 16, dtype=torch.uint8), torch.zeros(2, 16, 16, dtype=torch.uint8),
                 torch.zeros(2, 3))


def test_compat_import_path_resolves_train_css(monkeypatch):
    monkeypatch.syspath_prepend(os.path.join(ROOT, "sdflabel_amd", "compat"))
    for m in [m for m in sys.modules if m == "pipelines" or m.startswith("pipelines.")]:
        monkeypatch.delitem(sys.modules, m)
    from pipelines.train_css import train_css, train_step
    from sdflabel_amd.pipelines import train_css as P
    assert train_css is P.train_css and train_step is P.train_step
    for m in [m for m in sys.modules if m == "pipelines" or m.startswith("pipelines.")]:
        monkeypatch.delitem(sys.modules, m)
