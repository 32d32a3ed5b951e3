"""GPU tests of the KC epilogue (mlp_kernel.h: survivor vote from the mask words, stores placed by rank in the two survivor words;
csrc/kc_slots.h) with decoders whose survivor pattern is forced feature by feature: a bias of -1e4 kills a feature at every
point, +1e3 keeps it alive at every point.  SDFR_FWD_COMPACT=1 must give the sdf bits and mask words of the full chain (=0), through the
plain entry and through sdfr_mlp_forward_ordered, and the full chain's mask words of the shifted layer must show exactly the forced bits
(so that a bias edit that did not take hold cannot make the comparison empty)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import sdflabel_amd
from sdflabel_amd import _lib
from sdflabel_amd.fixtures import ASSET

pytestmark = pytest.mark.gpu
DEV = "cuda"
D = 8                                  # 512 rows = 8 tiles of 64


def chain_feature(w, c):
    """feature of wave w's chain position c = 2 q + g (register q, lane group g)"""
    q, g = c >> 1, c & 1
    return w * 64 + (q >> 4) * 32 + ((q >> 2) & 3) * 8 + 4 * g + (q & 3)


def low_counts(counts):
    return [[c for c in range(n)] for n in counts]


PATTERNS = {
    "counts_0_1_7_8_9_63_64": low_counts([0, 1, 7, 8, 9, 63, 64, 1]),
    "counts_64_63_9_8_7_1_0": low_counts([64, 63, 9, 8, 7, 1, 0, 9]),
    "single_survivor_per_wave": [[(9 * w + 4) % 64] for w in range(8)],
    "even_positions": [list(range(0, 64, 2))] * 8,
    "odd_positions": [list(range(1, 64, 2))] * 8,
    "all_dead": [[]] * 8,
    "all_alive": [list(range(64))] * 8,
    "mixed": [[c for c in range(64) if (c * 7 + w * 3) % 5 < 2] for w in range(8)],
}


def forced_decoder(layer, pattern):
    d, _ = sdflabel_amd.setup_dsdf(ASSET + ".pt", precision=torch.float32)
    lin = getattr(d, "lin%d" % layer)
    n_out = lin.bias.shape[0]
    alive = torch.zeros(512, dtype=torch.bool)
    for w, cs in enumerate(PATTERNS[pattern]):
        for c in cs:
            alive[chain_feature(w, c)] = True
    shift = torch.where(alive[:n_out], torch.tensor(1.0e3), torch.tensor(-1.0e4))
    with torch.no_grad():
        lin.bias.add_(shift.to(lin.bias.dtype))
    return d.to(DEV), alive[:n_out]


@pytest.fixture(scope="module")
def inputs():
    pts = sdflabel_amd.Grid3D(D, DEV).points.detach()
    lat = F.normalize(torch.tensor([[0.3, -0.5, 0.8]], device=DEV), p=2, dim=1)
    return torch.cat([lat.expand(pts.shape[0], -1), pts], 1).contiguous()


@pytest.fixture(scope="module")
def order():
    o = np.empty(D ** 3, np.int32)
    _lib.check(_lib.lib().sdfr_grid_tile_order(D, o.ctypes.data), "sdfr_grid_tile_order")
    return torch.from_numpy(o).to(DEV)


def forward(dec, inp, n, compact, monkeypatch, order=None):
    L = _lib.lib()
    h = dec.handle(torch.device(DEV)).h
    sdf = torch.full((n,), float("nan"), device=DEV)
    mw = torch.zeros(int(L.sdfr_decoder_mask_words(h, n)), dtype=torch.int32, device=DEV)
    monkeypatch.setenv("SDFR_FWD_COMPACT", "1" if compact else "0")
    if order is None:
        _lib.check(L.sdfr_mlp_forward(h, _lib.ptr(inp), n, _lib.ptr(sdf), _lib.ptr(mw), _lib.stream_ptr()), "sdfr_mlp_forward")
    else:
        _lib.check(L.sdfr_mlp_forward_ordered(h, _lib.ptr(inp), n, _lib.ptr(sdf), _lib.ptr(mw), _lib.ptr(order), order.shape[0],
                                              _lib.stream_ptr()), "sdfr_mlp_forward_ordered")
    torch.cuda.synchronize()
    return sdf, mw


def layer_bits(mw, n, layer):
    """[n][512] bool: the saved ReLU bits of one layer (mask layout v2: blocks of 128 rows, per layer 128 x 16 dwords; feature j at dword
    j >> 5, bit ((j >> 2) & 1) * 16 + ((j & 31) >> 3) * 4 + (j & 3))"""
    blocks = (n + 127) // 128
    n_layers = mw.numel() // (blocks * 128 * 16)
    words = mw.view(blocks, n_layers, 128, 16)[:, layer].reshape(blocks * 128, 16)[:n].cpu().numpy().astype(np.uint32)
    j = np.arange(512)
    sh = ((j >> 2) & 1) * 16 + ((j & 31) >> 3) * 4 + (j & 3)
    return ((words[:, j >> 5] >> sh[None, :].astype(np.uint32)) & 1).astype(bool)


CASES = [(1, p) for p in PATTERNS] + [(3, p) for p in PATTERNS] + [(6, "counts_0_1_7_8_9_63_64"), (6, "mixed")]


@pytest.mark.parametrize("layer,pattern", CASES)
def test_forced_survivor_patterns_bitwise(layer, pattern, inputs, order, monkeypatch):
    dec, alive = forced_decoder(layer, pattern)
    n = inputs.shape[0]
    s0, m0 = forward(dec, inputs, n, False, monkeypatch)
    bits = layer_bits(m0, n, layer)[:, :alive.shape[0]]
    assert (bits == alive.numpy()[None, :]).all()                      # the pattern took hold, at every row
    assert torch.isfinite(s0).all()
    for o in (None, order):
        s1, m1 = forward(dec, inputs, n, True, monkeypatch, o)
        assert torch.equal(s0.view(torch.int32), s1.view(torch.int32))
        assert torch.equal(m0, m1)
    for rows in (1, 63, 65):                                           # partial tiles
        r0, q0 = forward(dec, inputs, rows, False, monkeypatch)
        r1, q1 = forward(dec, inputs, rows, True, monkeypatch)
        assert torch.equal(r0.view(torch.int32), r1.view(torch.int32)) and torch.equal(q0, q1)
        assert torch.equal(r0.view(torch.int32), s0[:rows].view(torch.int32))
