"""GPU tests of the tail of the band Jacobian's compacted product (mlp_kernel.h: gemm_kcj runs the whole trips of four k tiles in its ring
loop and the remaining 0 to 3 tiles behind the loop's exit; csrc/kcj_slots.h, sdfr_kcj_tiles).  A product that stops a tile
early loses survivors, one that takes a tile from the wrong stage or with the wrong operand multiplies another tile's weights: either
changes bits.  sdfr_mlp_jacobian is driven with crafted mask buffers as tests/test_gpu_jac_compact.py drives it, here with the SAME
survivor total in every 16-row tile of the launch (each surviving feature is set in at least one row of every tile): 0, 1, 4, 5, 15, 16, 17,
47, 48, 49, 63, 64, 65, 511 and 512 per layer -- both sides of every k-tile and trip boundary -- the same total in all layers, and different
totals in the layers of one launch; 16, 33 and 48 selected rows (the 48 in two crops of 24).  J and the selected sdf values of the default
(the tail) must be the bits of SDFR_KC_TAIL=0 (whole trips) and of SDFR_JAC_COMPACT=0 (the full chain).  Then the real band of each
committed decoder at D = 8."""
import numpy as np
import pytest
import torch

import sdflabel_amd
from sdflabel_amd import _lib
from sdflabel_amd.fixtures import ASSET, ASSET_ELLIPSOID, K_for
from tests import _decoder_cases as C
from tests.test_gpu_jac_compact import DEV, G, HP, N, forward_values, launch, setup

pytestmark = pytest.mark.gpu
TOTALS = [0, 1, 4, 5, 15, 16, 17, 47, 48, 49, 63, 64, 65, 511, 512]
# selected rows per crop (absolute rows of the 512; the second entry of a pair is the crops' rows_per_crop): one tile, two tiles and a row, and
# two crops of 24 -- a launch holds fewer than 40 rows per crop, and a crop's tiles are consecutive runs of 16 of its selected rows
ROWS = {16: ([np.arange(16) * 31 + 7], G), 33: ([np.arange(33) * 15 + 2], G), 48: ([np.arange(24) * 10 + 5, 256 + np.arange(24) * 9 + 3], G // 2)}


def tile_bits(rng, crops, per_layer, p=0.4):
    """bits (G, layers, HP): feature j of a layer's survivors is set in every selected row with probability p and surely in one row of every
    16-row tile, every other feature in none"""
    bits = np.zeros((G, len(per_layer), HP), bool)
    tiles = [c[t0:t0 + 16] for c in crops for t0 in range(0, len(c), 16)]
    for l, alive in enumerate(per_layer):
        alive = np.asarray(alive, np.int64)
        if not len(alive):
            continue
        for tile in tiles:
            sub = rng.random((len(tile), len(alive))) < p
            sub[rng.integers(0, len(tile), len(alive)), np.arange(len(alive))] = True
            bits[np.ix_(tile, [l], alive)] = sub[:, None, :]
    return bits


def three_ways(bits, crops, rpc, monkeypatch):
    rows = np.concatenate(crops)
    sdf = forward_values(bits, rows)
    got = []
    for compact, tail in (("0", "1"), ("1", "0"), ("1", "1")):
        monkeypatch.setenv("SDFR_KC_TAIL", tail)
        r = launch(bits, sdf, [c - b * rpc for b, c in enumerate(crops)], rpc, compact, monkeypatch)
        assert sorted(r) == rows.tolist()
        got.append((np.stack([r[i][0] for i in rows]), np.array([r[i][1] for i in rows])))
    (J0, s0), (J1, s1), (J2, s2) = got
    assert np.isfinite(J2).all()
    assert np.array_equal(J2.view(np.uint32), J1.view(np.uint32)) and np.array_equal(s2.view(np.uint32), s1.view(np.uint32)), "tail vs whole trips"
    assert np.array_equal(J2.view(np.uint32), J0.view(np.uint32)) and np.array_equal(s2.view(np.uint32), s0.view(np.uint32)), "tail vs full chain"
    assert np.array_equal(s2, sdf[rows])


@pytest.mark.parametrize("n_rows", sorted(ROWS))
@pytest.mark.parametrize("total", TOTALS)
def test_same_total_in_every_layer(total, n_rows, monkeypatch):
    net = setup()[0]
    rng = np.random.default_rng(1000 * n_rows + total)
    per_layer = [rng.permutation(od)[:min(total, od)] for od in net.out_dims]
    three_ways(tile_bits(rng, ROWS[n_rows][0], per_layer), *ROWS[n_rows], monkeypatch)


@pytest.mark.parametrize("shift", range(0, len(TOTALS), 2))
def test_different_totals_in_the_layers_of_one_launch(shift, monkeypatch):
    net = setup()[0]
    rng = np.random.default_rng(77 + shift)
    totals = [TOTALS[(shift + 4 * l) % len(TOTALS)] for l in range(len(net.out_dims))]
    per_layer = [rng.permutation(od)[:min(t, od)] for t, od in zip(totals, net.out_dims)]
    three_ways(tile_bits(rng, ROWS[33][0], per_layer), *ROWS[33], monkeypatch)


@pytest.mark.parametrize("asset", [ASSET, ASSET_ELLIPSOID], ids=["rounded_box", "ellipsoid"])
def test_real_band(asset, monkeypatch):
    """BatchRenderer.forward() at D = 8: J and sdf_band of its band from its own masks"""
    dec = sdflabel_amd.setup_dsdf(asset + ".pt", precision=torch.float32)[0].to(DEV)
    br = sdflabel_amd.BatchRenderer(dec, 8, K_for(64, 64), (64, 64), 1, device=DEV)
    br.set_params(torch.full((1,), 0.7, device=DEV), torch.tensor([[0.05, 0.02, 3.3]], device=DEV), torch.tensor([[0.3, -0.5, 0.8]], device=DEV))
    br.forward()
    torch.cuda.synchronize()
    cnt = int(br.cnt[0])
    assert 0 < cnt <= br.cap
    L, P = _lib.lib(), _lib.ptr
    got = []
    for compact, tail in (("0", "1"), ("1", "0"), ("1", "1")):
        monkeypatch.setenv("SDFR_JAC_COMPACT", compact)
        monkeypatch.setenv("SDFR_KC_TAIL", tail)
        br.J.fill_(C.SENTINEL)
        br.sdf_band.fill_(C.SENTINEL)
        _lib.check(L.sdfr_mlp_jacobian(br.handle.h, P(br.inputs), br.G, 1, P(br.idx), br.cap, P(br.cnt), P(br.J), P(br.sdf_band), P(br.sdf), P(br.mask_ws),
                                       0, _lib.stream_ptr()), "sdfr_mlp_jacobian")
        torch.cuda.synchronize()
        got.append((N(br.J)[0, :cnt].copy(), N(br.sdf_band).reshape(-1)[:cnt].copy()))
    (J0, s0), (J1, s1), (J2, s2) = got
    print("JACTAIL real band: %d rows" % cnt)
    assert np.isfinite(J2).all() and np.isfinite(s2).all()
    assert np.array_equal(J2.view(np.uint32), J1.view(np.uint32)) and np.array_equal(s2.view(np.uint32), s1.view(np.uint32))
    assert np.array_equal(J2.view(np.uint32), J0.view(np.uint32)) and np.array_equal(s2.view(np.uint32), s0.view(np.uint32))
