"""GPU tests of the tail of the grid forward's compacted product (mlp_kernel.h: gemm_kc_body of the 64-row kernels runs the whole trips of
eight chain steps in its ring loop and the remaining 0 to 7 steps behind the loop's exit; csrc/kc_slots.h, sdfr_kc_steps).
A product that stops one chain step early loses a survivor, one that takes a step from the wrong stage multiplies another tile's weights:
either changes bits.  So per-layer survivor counts on both sides of every step, k-tile and trip boundary -- 1, 2, 3, 7, 8, 9, 15, 16, 17, 23,
24, 25, 31, 33, 511, 512 -- are forced through the bias as tests/test_gpu_kc_dense.py forces them (alive at every point of every tile, so a
tile's count is the forced one), in one layer, in two consecutive layers at once, and in the 506-wide layer 3 whose operand carries the
re-injected input columns behind its survivors (latent_in = [4]) together with layer 4.  64 and 192 rows, through the plain entry and through
sdfr_mlp_forward_ordered.  The default (the tail) must give the sdf bits and every mask word of SDFR_KC_TAIL=0 (whole trips) and of
SDFR_FWD_COMPACT=0 (the full chain), and the full chain's masks must show the forced pattern first.  One whole-grid case per committed
decoder at D = 8."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import sdflabel_amd
from sdflabel_amd import _lib
from sdflabel_amd.fixtures import ASSET, ASSET_ELLIPSOID
from tests.test_gpu_kc_dense import DEV, ORDER64, decoder, force, forward, layer_bits

pytestmark = pytest.mark.gpu
COUNTS = [1, 2, 3, 7, 8, 9, 15, 16, 17, 23, 24, 25, 31, 33, 511, 512]
SIZES = (64, 192)
KEEP = 10.0                              # a forced layer that feeds another forced layer stays small against that layer's -1e4 / +1e3


@pytest.fixture(scope="module")
def rows192():
    pts = sdflabel_amd.Grid3D(8, DEV).points.detach()[:192]
    lat = F.normalize(torch.tensor([[0.3, -0.5, 0.8]], device=DEV), p=2, dim=1)
    return torch.cat([lat.expand(pts.shape[0], -1), pts], 1).contiguous()


@pytest.fixture(scope="module")
def order64():
    return torch.from_numpy(ORDER64).to(DEV)


def alive_set(total, width, seed):
    a = np.zeros(512, bool)
    a[np.random.default_rng(seed).choice(width, min(total, width), replace=False)] = True
    return a


def three_ways(h, x, n, order, monkeypatch):
    """(sdf, masks) of the full chain, of whole trips and of the tail"""
    out = []
    for compact, tail in ((0, "1"), (1, "0"), (1, "1")):
        monkeypatch.setenv("SDFR_KC_TAIL", tail)
        out.append(forward(h, x, n, compact, monkeypatch, order))
    return out


def check(d, x, expect, order64, monkeypatch):
    h = d.to(DEV).handle(torch.device(DEV)).h
    for n in SIZES:
        for o in (None, order64):
            (s0, m0), (s1, m1), (s2, m2) = three_ways(h, x, n, o, monkeypatch)
            for layer, want in expect.items():
                assert (layer_bits(m0, n, layer)[:, :want.shape[0]] == want[None, :]).all(), (n, layer)      # the pattern took hold
            assert torch.isfinite(s0).all()
            assert torch.equal(s2.view(torch.int32), s1.view(torch.int32)) and torch.equal(m2, m1), ("tail vs whole trips", n, o is not None)
            assert torch.equal(s2.view(torch.int32), s0.view(torch.int32)) and torch.equal(m2, m0), ("tail vs full chain", n, o is not None)


@pytest.mark.parametrize("total", COUNTS)
def test_one_layer(total, rows192, order64, monkeypatch):
    d = decoder()
    a = force(d.lin1, alive_set(total, 512, total))
    assert a.sum() == total
    check(d, rows192, {1: a}, order64, monkeypatch)


@pytest.mark.parametrize("i", range(len(COUNTS)))
def test_two_layers_at_once(i, rows192, order64, monkeypatch):
    n1, n2 = COUNTS[i], COUNTS[(i + 5) % len(COUNTS)]
    d = decoder()
    a1 = force(d.lin1, alive_set(n1, 512, 100 + i), keep=KEEP)
    a2 = force(d.lin2, alive_set(n2, 512, 200 + i))
    assert (a1.sum(), a2.sum()) == (n1, n2)
    check(d, rows192, {1: a1, 2: a2}, order64, monkeypatch)


@pytest.mark.parametrize("i", range(len(COUNTS)))
def test_re_injecting_layer_and_the_layer_behind_it(i, rows192, order64, monkeypatch):
    """layer 3 has 506 outputs (511 and 512 mean all of them); the input columns behind them are survivors of their own wherever they are
    non-zero, so layer 4's product walks the forced count plus up to six"""
    n3, n4 = COUNTS[i], COUNTS[(i + 7) % len(COUNTS)]
    d = decoder()
    a3 = force(d.lin3, alive_set(n3, 506, 300 + i), keep=KEEP)
    a4 = force(d.lin4, alive_set(n4, 512, 400 + i))
    assert (a3.sum(), a4.sum()) == (min(n3, 506), n4)
    check(d, rows192, {3: a3[:506], 4: a4}, order64, monkeypatch)


@pytest.mark.parametrize("asset", [ASSET, ASSET_ELLIPSOID], ids=["rounded_box", "ellipsoid"])
def test_whole_grid(asset, monkeypatch):
    """the committed decoders on the 8^3 grid (8 tiles): plain entry and the 4x4x4-block tile order"""
    d, _ = sdflabel_amd.setup_dsdf(asset + ".pt", precision=torch.float32)
    h = d.to(DEV).handle(torch.device(DEV)).h
    pts = sdflabel_amd.Grid3D(8, DEV).points.detach()
    lat = F.normalize(torch.tensor([[0.3, -0.5, 0.8]], device=DEV), p=2, dim=1)
    x = torch.cat([lat.expand(pts.shape[0], -1), pts], 1).contiguous()
    o = np.empty(512, np.int32)
    _lib.check(_lib.lib().sdfr_grid_tile_order(8, o.ctypes.data), "sdfr_grid_tile_order")
    for order in (None, torch.from_numpy(o).to(DEV)):
        (s0, m0), (s1, m1), (s2, m2) = three_ways(h, x, 512, order, monkeypatch)
        assert torch.isfinite(s2).all()
        assert torch.equal(s2.view(torch.int32), s1.view(torch.int32)) and torch.equal(m2, m1)
        assert torch.equal(s2.view(torch.int32), s0.view(torch.int32)) and torch.equal(m2, m0)
