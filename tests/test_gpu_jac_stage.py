"""The compaction stage of the band Jacobian with chain-order survivor words (mlp_kernel.h KCJ, csrc/kcjd_slots.h):
sdfr_mlp_jacobian on mask workspaces written by the test, with the helpers of tests/test_gpu_jac_compact.py.  J and sdf_band are compared bit
for bit between the default, SDFR_JAC_STAGE=0 (a survivor's place from the running count) and SDFR_JAC_COMPACT=0 (the full K chain), and J
against the float64 Jacobian of the same masks within the bound of tests/test_gpu_decoder_ref.py (judge_jac_masks, ratio <= 1).  The mask
patterns are those of tests/kcjd_host -- 0, 1, 63, 64, 65, 128 and every survivor, an empty wave block, survivors only in the last lane group
of the last wave, densities 0.1, 0.5 and 0.9 -- a different one in every layer of a launch; both committed decoders."""
import functools

import numpy as np
import pytest
import torch

import sdflabel_amd
from sdflabel_amd.fixtures import ASSET, ASSET_ELLIPSOID
from tests import _decoder_ref as R
from tests import test_gpu_jac_compact as JC

pytestmark = pytest.mark.gpu
G, HP = JC.G, JC.HP


@functools.lru_cache(maxsize=None)
def _setup(asset):
    """what tests.test_gpu_jac_compact.setup() returns, for either committed decoder"""
    dec = sdflabel_amd.setup_dsdf(asset + ".pt", precision=torch.float32)[0].eval()
    net = R.Net.from_decoder(dec)
    h = dec.handle(torch.device(JC.DEV))
    pts = JC.N(sdflabel_amd.Grid3D(8, JC.DEV).points).astype(np.float32)
    lat = np.array([0.3, -0.5, 0.8], np.float32)
    lat /= np.linalg.norm(lat)
    x = np.concatenate([np.broadcast_to(lat, (G, net.n_inputs - 3)), pts], 1).astype(np.float32)
    return net, h, x, JC.T(x), dec


@pytest.fixture(params=[ASSET, ASSET_ELLIPSOID], ids=["deepsdf_synth", "deepsdf_synth_ellipsoid"])
def net(request, monkeypatch):
    s = _setup(request.param)
    monkeypatch.setattr(JC, "setup", lambda: s[:4])
    return s[0]


def three_ways(bits, crops, rpc, monkeypatch):
    """default, SDFR_JAC_STAGE=0, SDFR_JAC_COMPACT=0: equal bits; the default's J within the reference bound; sdf_band the supplied value"""
    net, h, x, d_x = JC.setup()
    rows = np.sort(np.concatenate([b * rpc + np.asarray(c) for b, c in enumerate(crops)]))
    sdf = JC.forward_values(bits, rows)
    monkeypatch.setenv("SDFR_JAC_STAGE", "1")
    a = JC.launch(bits, sdf, crops, rpc, "1", monkeypatch)
    monkeypatch.setenv("SDFR_JAC_STAGE", "0")
    b = JC.launch(bits, sdf, crops, rpc, "1", monkeypatch)
    c = JC.launch(bits, sdf, crops, rpc, "0", monkeypatch)
    monkeypatch.delenv("SDFR_JAC_STAGE")
    d = JC.launch(bits, sdf, crops, rpc, "1", monkeypatch)                # (the variable unset: the default)
    assert sorted(a) == rows.tolist()
    Ja = np.stack([a[r][0] for r in rows])
    for name, other in (("SDFR_JAC_STAGE=0", b), ("SDFR_JAC_COMPACT=0", c), ("the variable unset", d)):
        Jo = np.stack([other[r][0] for r in rows])
        assert np.array_equal(Ja.view(np.uint32), Jo.view(np.uint32)), "J differs from " + name
        assert all(a[r][1] == sdf[r] and other[r][1] == sdf[r] for r in rows), "sdf_band is not the supplied value"
    masks = [bits[rows, l, :od] for l, od in enumerate(net.out_dims)]
    ratio = R.judge_jac_masks(net, x[rows], masks, Ja, "f32", "f32")
    print("JACSTAGE max ratio %.4f over %d rows" % (float(ratio.max()), len(rows)))
    assert ratio.max() <= 1, (np.unravel_index(ratio.argmax(), ratio.shape), float(ratio.max()))


def pattern(rng, kind, od):
    """the surviving features of one layer"""
    if isinstance(kind, int):
        return rng.permutation(od)[:min(kind, od)]
    if kind.startswith("empty_wave"):
        wv = int(kind[-1])
        j = np.flatnonzero(rng.random(od) < 0.5)
        return j[j // 128 != wv]
    if kind == "last_group_of_last_wave":
        j = np.arange(od)
        return j[(j >= 384) & ((j >> 2) & 3 == 3)]
    j = np.flatnonzero(rng.random(od) < float(kind))
    return j if len(j) else np.array([0])


KINDS = [0, 1, 63, 64, 65, 128, 512, "empty_wave0", "empty_wave1", "empty_wave2", "empty_wave3", "last_group_of_last_wave", "0.1", "0.5", "0.9"]


@pytest.mark.parametrize("shift", [0, 3, 6, 9, 12])
def test_host_patterns_a_different_one_per_layer(net, shift, monkeypatch):
    """layer l of the launch takes pattern (shift + l) of the list: the five launches put every pattern into layers 1 .. 7, whose masks
    the compacted operands come from"""
    rng = np.random.default_rng(100 + shift)
    per_layer = [pattern(rng, KINDS[(shift + l) % len(KINDS)], od) for l, od in enumerate(net.out_dims)]
    three_ways(JC.layer_bits(rng, JC.ROWS17, per_layer), [JC.ROWS17], G, monkeypatch)


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("n", [1, 15, 16, 17, 33])
def test_band_counts(net, n, B, monkeypatch):
    """1, 15, 16, 17 and 33 band rows; B = 2 with different counts (n and n - 1)"""
    rng = np.random.default_rng(10 * n + B)
    rpc = G // B
    crops = [np.sort(rng.permutation(rpc)[:n]) if b == 0 else np.sort(rng.permutation(rpc)[:max(1, n - 1)]) for b in range(B)]
    rows = np.concatenate([b * rpc + c for b, c in enumerate(crops)])
    bits = np.zeros((G, len(net.out_dims), HP), bool)
    bits[rows] = rng.random((len(rows), len(net.out_dims), HP)) < 0.1
    for l, od in enumerate(net.out_dims):
        bits[:, l, od:] = False
    three_ways(bits, crops, rpc, monkeypatch)
