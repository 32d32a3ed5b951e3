"""The CSS network's output head without a GPU: golden G20 (tools/make_golden_css.py, recorded from the reference's own module), the float64
restatement of tests/_css_ref.py that the GPU tests measure against, the drop-in network's parameter names and shapes, the import shims and
the ABI.  Figures are printed before they are asserted."""
import os
import re
import sys

import numpy as np
import pytest
import torch

from sdflabel_amd import _lib
from tests import _css_ref as R
from tests._util import ROOT, gold

NEW = ("sdfr_css_head", "sdfr_css_latent")


@pytest.fixture(scope="module")
def z():
    return gold("g20_css_head.npz")


def head_weights(z):
    return {h: (z["w_" + h], z["b_" + h]) for h in ("u", "v", "w", "mask")}


def test_restatement_agrees_with_the_reference_outputs(z):
    """the reference's float32 forward lies within the derived tolerance of the float64 restatement on its own head inputs"""
    out, tol, unsure = R.head(z["x_u"], z["x_v"], z["x_w"], z["x_mask"], head_weights(z))
    lat, lat_tol = R.latent(z["x4"], z["w_lat"], z["b_lat"])
    out["latent"], tol["latent"] = lat, lat_tol
    pix = z["lp_pix"]
    for k in ("u", "v", "w"):                                   # the file holds the log-probabilities at every 8th pixel
        out[k] = out[k].reshape(2, 256, -1)[:, :, pix]
        tol[k] = tol[k].reshape(2, 256, -1)[:, :, pix]
    got = {k: z["out_" + k] for k in ("uvw_sm", "uvw_sm_masked", "mask", "mask_sm", "latent", "u", "v", "w")}
    res = R.compare(got, out, tol, unsure, label="reference float32:")
    assert set(res) == set(got)
    # the fixture exercises what it was built for: both mask classes, a mixing head and peaked heads
    fg = float((z["out_mask"][:, 1] > z["out_mask"][:, 0]).mean())
    print("foreground share %.3f, top-two gap below 0.05 (u, v, w): %s" % (fg, z["top_two_gap_below_0p05"]))
    assert 0.3 <= fg <= 0.7 and fg == float(z["foreground_share"])
    assert (z["out_uvw_sm_masked"] != 0).any() and (z["out_uvw_sm_masked"] == 0).any()
    for k in ("uvw_sm", "mask", "mask_sm", "latent", "u", "v", "w"):
        assert z["err_" + k].shape == (2,) and 0 < z["err_" + k][1] <= z["err_" + k][0]


def test_backbone_is_the_reference_backbone(z):
    assert float(z["backbone_max_diff"]) == 0.0


def test_state_dict_names_and_shapes_are_the_reference_ones(z):
    from sdflabel_amd.networks.resnet_css import resnet18
    net = resnet18()
    sd = net.state_dict()
    names = [str(n) for n in z["sd_names"]]
    shapes = [tuple(int(v) for v in row if v >= 0) for row in z["sd_shapes"]]
    assert len(names) == 354 and list(sd.keys()) == names
    assert [tuple(v.shape) for v in sd.values()] == shapes
    assert sum(p.numel() for p in net.parameters()) == 14921413
    # a checkpoint with the reference's names and shapes loads strictly (what torch.load of a css.pt returns)
    fake = {n: torch.full(s, 0.5, dtype=sd[n].dtype) for n, s in zip(names, shapes)}
    net.load_state_dict(fake, strict=True)
    assert float(net.out_u.conv.weight.detach()[3, 5, 0, 0]) == 0.5
    assert not net.conv1.weight.requires_grad and net.layer2[0].conv1.weight.requires_grad      # the frozen stem


def test_features_run_on_the_cpu_with_the_recorded_shapes(z):
    from sdflabel_amd.networks.resnet_css import setup_css
    torch.manual_seed(1)
    net = setup_css(mode="eval")
    assert not net.training and setup_css().training                     # the reference's default mode is 'train'
    with torch.no_grad():
        f = net.features(torch.from_numpy(z["x"]))
    assert sorted(f) == ["x4", "x_mask", "x_u", "x_v", "x_w"]
    for k in f:
        assert tuple(f[k].shape) == z[k].shape and f[k].dtype == torch.float32, k
    # forward needs the GPU: no host computation of the head
    with pytest.raises(_lib.SdfrError):
        net(torch.from_numpy(z["x"]))


def test_setup_css_never_downloads(tmp_path):
    from sdflabel_amd.networks.resnet_css import resnet18, setup_css
    with pytest.raises(RuntimeError):
        setup_css(pretrained=True)
    with pytest.raises(RuntimeError):
        resnet18(pretrained=True)
    path = str(tmp_path / "css.pt")
    torch.manual_seed(3)
    torch.save(resnet18().state_dict(), path)
    net = setup_css(pretrained=True, model_path=path, mode="eval")       # the strict load overrides everything: accepted
    assert torch.equal(net.out_lat.conv.weight, torch.load(path)["out_lat.conv.weight"])


def test_compat_import_path_resolves(monkeypatch):
    monkeypatch.syspath_prepend(os.path.join(ROOT, "sdflabel_amd", "compat"))
    for m in [m for m in sys.modules if m == "networks" or m.startswith("networks.")]:
        monkeypatch.delitem(sys.modules, m)
    from networks.resnet_css import setup_css
    from networks.unet_parts import outconv, up
    from sdflabel_amd.networks import resnet_css, unet_parts
    assert setup_css is resnet_css.setup_css and up is unet_parts.up and outconv is unet_parts.outconv
    for m in [m for m in sys.modules if m == "networks" or m.startswith("networks.")]:
        monkeypatch.delitem(sys.modules, m)


def test_new_entry_points_are_exported_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "sdfr.h")).read()
    h = _lib.lib()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _lib.EXPORTS and hasattr(h, name)
    assert int(re.search(r"#define SDFR_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION == h.sdfr_version() >= 406
    from sdflabel_amd import css
    assert callable(css.css_head) and callable(css.css_latent)
    # argument validation happens before any HIP call
    nul = [None] * 24
    a = list(nul)
    a[4:8] = [1, 32, 4, 4]
    assert h.sdfr_css_head(*a) == -1 and b"64" in h.sdfr_last_error()
    a[4:8] = [1, 64, 4, 4]
    assert h.sdfr_css_head(*a) == -1 and b"NULL" in h.sdfr_last_error()
    a[4:8] = [0, 64, 4, 4]
    assert h.sdfr_css_head(*a) == 0
    assert h.sdfr_css_latent(None, 1, 64, 2, 2, None, None, None, None) == -1 and b"256" in h.sdfr_last_error()
    assert h.sdfr_css_latent(None, 1, 256, 2, 2, None, None, None, None) == -1
    assert h.sdfr_css_latent(None, 2, 256, 0, 2, None, None, None, None) == 0
    # the Python boundary refuses host tensors, other dtypes, other channel counts and other layouts
    x = torch.zeros(1, 64, 4, 4)
    with pytest.raises(_lib.SdfrError):
        css.css_head(x, x, x, x, {})
    with pytest.raises(_lib.SdfrError):
        css.css_latent(torch.zeros(1, 256, 2, 2), torch.zeros(3, 256), torch.zeros(3))
