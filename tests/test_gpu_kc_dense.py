"""GPU tests of the dense image of the 64-row kernels' compacted layers (mlp_kernel.h: kc_store writes every feature to its own row, the
product reads the operand through the k list; csrc/kc_slots.h, sdfr_kcd_*).  8 x 512 decoders whose survivor patterns are
forced as tests/test_gpu_kc_epilogue.py and tests/test_gpu_kc_kmajor.py force them (a bias of -1e4 kills a feature at every point, +1e3
keeps it; a layer-0 weight row of K on the x column, which carries +1 / -1, makes a feature live at chosen rows only), launches of 64, 128
and 192 rows through the plain entry and through sdfr_mlp_forward_ordered (a permutation of 64 rows, so every launch size is a whole number
of them).  SDFR_FWD_COMPACT=1 must give the sdf bits and every mask word of the full chain (=0), the full chain's mask words must show the
forced pattern first, and the output must stay within the per-row bound of tests/_decoder_ref.py against float64.

What the patterns are after: rows of the image that hold another tile's or another layer's values (an empty tile next to a full one, two
layers with disjoint survivor sets -- the dense image never clears a row, it overwrites all of them), K extents around the padding to 16
(1, 15, 16, 17, 512 survivors: pads read the zero row behind the image and Wk's row 512), the first and the last row, the re-injected
columns behind a layer of width 506, and a dead row that must never be read: NaN weights in the k rows of dead features.  The decoder's
finite check declines the compaction for such weights (and keeps doing so); SDFR_FWD_COMPACT=2 forces it for this one test, and the result
must be finite and the bits of the unpoisoned decoder's full chain."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import sdflabel_amd
from sdflabel_amd import _lib
from sdflabel_amd.deepsdf.networks.deep_sdf_decoder_scale import _DecoderHandle
from sdflabel_amd.fixtures import ASSET
from tests import _decoder_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
D = 8                                    # 512 rows = 8 tiles of 64
K = 1.0e3
XCOL = 3                                 # inputs = latent (3) | x y z
SIZES = (64, 128, 192)
ORDER64 = np.random.default_rng(5).permutation(64).astype(np.int32)


def chain_feature(w, c):
    """feature of wave w's chain position c = 2 q + g (register q, lane group g)"""
    q, g = c >> 1, c & 1
    return w * 64 + (q >> 4) * 32 + ((q >> 2) & 3) * 8 + 4 * g + (q & 3)


def set_row(lin, j, col):
    """weight row j = K on input column col, zero elsewhere (weight norm: unit direction, gain K); bias 0"""
    with torch.no_grad():
        if hasattr(lin, "weight_v"):
            lin.weight_v[j].zero_()
            lin.weight_v[j, col] = 1.0
            lin.weight_g[j] = K
        else:
            lin.weight[j].zero_()
            lin.weight[j, col] = K
        lin.bias[j] = 0.0


def force(lin, alive, keep=1.0e3):
    """bias +keep where alive, -1e4 elsewhere: the layer's pattern at every point"""
    n_out = lin.bias.shape[0]
    a = torch.as_tensor(np.asarray(alive, bool)[:n_out])
    with torch.no_grad():
        lin.bias.add_(torch.where(a, torch.tensor(keep), torch.tensor(-1.0e4)).to(lin.bias.dtype))
    return a.numpy()


def layer_bits(mw, n, layer):
    """[n][512] bool: the saved ReLU bits of one layer (mask layout v2: blocks of 128 rows, per layer 128 x 16 dwords; feature j at dword
    j >> 5, bit ((j >> 2) & 1) * 16 + ((j & 31) >> 3) * 4 + (j & 3))"""
    blocks = (n + 127) // 128
    n_layers = mw.numel() // (blocks * 128 * 16)
    words = mw.view(blocks, n_layers, 128, 16)[:, layer].reshape(blocks * 128, 16)[:n].cpu().numpy().astype(np.uint32)
    j = np.arange(512)
    sh = ((j >> 2) & 1) * 16 + ((j & 31) >> 3) * 4 + (j & 3)
    return ((words[:, j >> 5] >> sh[None, :].astype(np.uint32)) & 1).astype(bool)


def forward(h, inp, n, compact, monkeypatch, order=None):
    L = _lib.lib()
    sdf = torch.full((n,), float("nan"), device=DEV)
    mw = torch.zeros(int(L.sdfr_decoder_mask_words(h, n)), dtype=torch.int32, device=DEV)
    monkeypatch.setenv("SDFR_FWD_COMPACT", str(compact))
    if order is None:
        _lib.check(L.sdfr_mlp_forward(h, _lib.ptr(inp), n, _lib.ptr(sdf), _lib.ptr(mw), _lib.stream_ptr()), "sdfr_mlp_forward")
    else:
        _lib.check(L.sdfr_mlp_forward_ordered(h, _lib.ptr(inp), n, _lib.ptr(sdf), _lib.ptr(mw), _lib.ptr(order), order.shape[0],
                                              _lib.stream_ptr()), "sdfr_mlp_forward_ordered")
    torch.cuda.synchronize()
    return sdf, mw


@pytest.fixture(scope="module")
def base_inputs():
    pts = sdflabel_amd.Grid3D(D, DEV).points.detach()
    lat = F.normalize(torch.tensor([[0.3, -0.5, 0.8]], device=DEV), p=2, dim=1)
    return torch.cat([lat.expand(pts.shape[0], -1), pts], 1).contiguous()


@pytest.fixture(scope="module")
def order64():
    return torch.from_numpy(ORDER64).to(DEV)


def coded(base, plus):
    """the first 192 rows with +1 in the x column where plus[row], -1 elsewhere"""
    x = base[:192].clone()
    x[:, XCOL] = torch.where(torch.as_tensor(plus, device=DEV), torch.tensor(1.0, device=DEV), torch.tensor(-1.0, device=DEV))
    return x.contiguous()


def decoder():
    d, _ = sdflabel_amd.setup_dsdf(ASSET + ".pt", precision=torch.float32)
    assert d.lin0.bias.shape[0] == 512 and d.lin3.bias.shape[0] == 512 - 6 and d.latent_in == [4]
    return d


def compare(net, h, x, expect, order64, monkeypatch, h_ref=None, compact=1):
    """=compact on handle h against the full chain on h_ref (default: h), every launch size, both entries; the bound against float64"""
    xs = x.cpu().numpy()
    for n in SIZES:
        r = R.evaluate(net, xs[:n], "f32")
        for o in (None, order64):
            s0, m0 = forward(h_ref or h, x, n, 0, monkeypatch, o)
            for layer, want in expect.items():
                bits = layer_bits(m0, n, layer)[:, :want.shape[-1]]
                assert (bits == (want[:n] if want.ndim == 2 else want[None, :])).all(), (n, layer)   # the pattern took hold
            assert torch.isfinite(s0).all()
            s1, m1 = forward(h, x, n, compact, monkeypatch, o)
            assert torch.isfinite(s1).all()
            assert torch.equal(s0.view(torch.int32), s1.view(torch.int32)), (n, o is not None)
            assert torch.equal(m0, m1), (n, o is not None)
            ratio = R.judge_forward(net, r, s1.cpu().numpy(), "f32")
            assert ratio.max() <= 1, (n, int(ratio.argmax()), float(ratio.max()))


def run(d, x, expect, order64, monkeypatch):
    net = R.Net.from_decoder(d)
    h = d.to(DEV).handle(torch.device(DEV)).h
    compare(net, h, x, expect, order64, monkeypatch)


def test_empty_tile_next_to_a_full_tile(base_inputs, order64, monkeypatch):
    """layer 0: no survivor in the tiles 0 and 2, all 512 in tile 1 of the same launch"""
    d = decoder()
    for j in range(512):
        set_row(d.lin0, j, XCOL)
    plus = (np.arange(192) // 64) == 1
    run(d, coded(base_inputs, plus), {0: np.repeat(plus[:, None], 512, 1)}, order64, monkeypatch)


@pytest.mark.parametrize("total", [1, 15, 16, 17, 512])
def test_survivor_totals_around_the_padding(total, base_inputs, order64, monkeypatch):
    d = decoder()
    alive = np.zeros(512, bool)
    alive[np.random.default_rng(total).choice(512, total, replace=False)] = True
    a = force(d.lin1, alive)
    assert a.sum() == total
    run(d, base_inputs[:192].contiguous(), {1: a}, order64, monkeypatch)


@pytest.mark.parametrize("feature", [0, 511])
def test_single_survivor_in_the_first_and_the_last_row(feature, base_inputs, order64, monkeypatch):
    assert chain_feature(0, 0) == 0 and chain_feature(7, 63) == 511
    d = decoder()
    alive = np.zeros(512, bool)
    alive[feature] = True
    run(d, base_inputs[:192].contiguous(), {1: force(d.lin1, alive)}, order64, monkeypatch)


def test_re_injecting_layer_with_forced_columns(base_inputs, order64, monkeypatch):
    """layer 3 (width 506) appends the input columns behind few survivors: rows 506..511 of the image carry per-point values -- the
    +1 / -1 column among them -- that no ReLU has touched"""
    d = decoder()
    alive = (np.arange(506) % 7) == 0
    a = force(d.lin3, alive)
    run(d, coded(base_inputs, np.arange(192) % 2 == 1), {3: a}, order64, monkeypatch)


def test_consecutive_layers_with_disjoint_survivors(base_inputs, order64, monkeypatch):
    """every row layer 1 left alive is dead in layer 2 and the other way round: a row that kept the previous layer's values would be read"""
    d = decoder()
    even = (np.arange(512) % 2) == 0
    # (layer 1 is kept alive by +30 only: 256 outputs of 1e3 each would carry layer 2 past its own -1e4)
    a1, a2 = force(d.lin1, even, keep=30.0), force(d.lin2, ~even)
    assert not (a1 & a2).any()
    run(d, base_inputs[:192].contiguous(), {1: a1, 2: a2}, order64, monkeypatch)


def test_dead_rows_are_never_read(base_inputs, order64, monkeypatch):
    """NaN in layer 2's weights of every feature that layer 1 leaves dead.  Feature 0 stays alive: Wk's row 512 of layer 1, which the pads
    name, is layer 2's row 0.  The finite check declines the compaction for this decoder (=1 is the full chain, which meets the NaN); =2 forces it."""
    d = decoder()
    alive = np.array([(j * 7) % 5 < 2 for j in range(512)])
    assert alive[0] and 0 < alive.sum() < 512 and alive.sum() % 16 != 0      # there are pads
    a = force(d.lin1, alive)
    net = R.Net.from_decoder(d)
    layers = [(W.copy(), b.copy()) for W, b in d.effective_layers()]
    layers[2][0][:, ~a] = np.nan
    dev = torch.device(DEV)
    poisoned = _DecoderHandle(layers, d.latent_size + 3, d._inject_table(), d.use_tanh, torch.cuda.current_device())
    h_ref = d.to(DEV).handle(dev).h
    x = base_inputs[:192].contiguous()
    # the guard holds: =1 is the full chain for this decoder, it meets the NaN in every output of layer 2 (which the ReLU then turns into
    # zeros) and gives another result than the unpoisoned decoder
    s, _ = forward(poisoned.h, x, 64, 1, monkeypatch)
    assert not torch.equal(s.view(torch.int32), forward(h_ref, x, 64, 0, monkeypatch)[0].view(torch.int32))
    compare(net, poisoned.h, x, {1: a}, order64, monkeypatch, h_ref=h_ref, compact=2)


def test_committed_fixture_ordered(base_inputs, monkeypatch):
    """the committed decoder on the 8^3 grid (8 tiles) through the ordered entry with the 4x4x4-block tile order"""
    d = decoder()
    net = R.Net.from_decoder(d)
    h = d.to(DEV).handle(torch.device(DEV)).h
    o = np.empty(D ** 3, np.int32)
    _lib.check(_lib.lib().sdfr_grid_tile_order(D, o.ctypes.data), "sdfr_grid_tile_order")
    o = torch.from_numpy(o).to(DEV)
    n = base_inputs.shape[0]
    s0, m0 = forward(h, base_inputs, n, 0, monkeypatch, o)
    s1, m1 = forward(h, base_inputs, n, 1, monkeypatch, o)
    assert torch.isfinite(s1).all()
    assert torch.equal(s0.view(torch.int32), s1.view(torch.int32)) and torch.equal(m0, m1)
    ratio = R.judge_forward(net, R.evaluate(net, base_inputs.cpu().numpy(), "f32"), s1.cpu().numpy(), "f32")
    assert ratio.max() <= 1, (int(ratio.argmax()), float(ratio.max()))
