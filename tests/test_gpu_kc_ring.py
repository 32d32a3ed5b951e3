"""GPU tests of the ring of the compacted product loop (mlp_kernel.h: gemm_kc_body of the 64-row kernels; csrc/kc_slots.h, sdfr_kc_ring_*;
DESIGN.md 3.1) at forced K-tile counts.  The loop's prologue names tiles 0 to 3, its gathers run two tiles ahead and a trip holds two tiles,
so the counts that matter are 2 (everything clamped), 4 (the k-list reads of the first trip reach the end), 6 (one trip past that), a
count of the form 4 n + 2 further out (10) and the full 64.  Layer 0's survivors are forced with the construction of
tests/test_gpu_kc_kmajor.py -- N features alive at the odd places of every 64-row tile only, every other feature of the layer dead -- which
sets layer 1's product to ceil(N / 16) * 2 k tiles; layer 1's are forced feature by feature through the bias as in
tests/test_gpu_kc_epilogue.py (M alive at every point), which sets layer 2's.  Three 64-row tiles; through the plain entry and through
sdfr_mlp_forward_ordered with a permutation of the 192 rows; SDFR_FWD_COMPACT=1 must give the sdf bits and the mask words of the full
chain (=0), and the full chain's masks must show exactly the forced patterns first."""
import pytest
import torch
import torch.nn.functional as F

import sdflabel_amd
from sdflabel_amd.fixtures import ASSET
from tests.test_gpu_kc_epilogue import DEV, chain_feature, forward, layer_bits
from tests.test_gpu_kc_kmajor import XCOL, coded

pytestmark = pytest.mark.gpu
N_ROWS = 192
ODD = list(range(1, 64, 2))
# (survivors forced in layer 0, in layer 1) -> k tiles of the products of layers 1 and 2: 2 (N / 16 rounded up, times two)
CASES = {
    "tiles_2_and_64": (9, 512),
    "tiles_2_and_4": (16, 17),
    "tiles_4_and_6": (17, 40),
    "tiles_6_and_10": (40, 70),
    "tiles_10_and_2": (70, 1),
    "tiles_64_and_6": (512, 33),
}


def features(n):
    """n features spread over the eight waves: wave p % 8, chain position p / 8"""
    return [chain_feature(p % 8, p // 8) for p in range(n)]


def set_unit_row(lin, j, col):
    """weight row j = 1 on input column col, zero elsewhere, bias 0: the feature is 1 where the column holds +1 and dead where it holds -1
    (a gain of 1 keeps layer 1's sums small against its forced biases)"""
    with torch.no_grad():
        if hasattr(lin, "weight_v"):
            lin.weight_v[j].zero_()
            lin.weight_v[j, col] = 1.0
            lin.weight_g[j] = 1.0
        else:
            lin.weight[j].zero_()
            lin.weight[j, col] = 1.0
        lin.bias[j] = 0.0


def tiles(n):
    return (n + 15) // 16 * 2


def forced_decoder(n0, n1):
    d, _ = sdflabel_amd.setup_dsdf(ASSET + ".pt", precision=torch.float32)
    assert d.lin0.bias.shape[0] == 512 and d.lin1.bias.shape[0] == 512
    js0, js1 = features(n0), features(n1)
    for j in js0:
        set_unit_row(d.lin0, j, XCOL)
    alive1 = torch.zeros(512, dtype=torch.bool)
    alive1[js1] = True
    dead0 = [j for j in range(512) if j not in set(js0)]
    with torch.no_grad():
        if dead0:
            d.lin0.bias[dead0] -= 1.0e4
        d.lin1.bias.add_(torch.where(alive1, torch.tensor(1.0e3), torch.tensor(-1.0e4)).to(d.lin1.bias.dtype))
    return d.to(DEV), js0, dead0, alive1


@pytest.fixture(scope="module")
def base_inputs():
    pts = sdflabel_amd.Grid3D(8, DEV).points.detach()[:N_ROWS]
    lat = F.normalize(torch.tensor([[0.3, -0.5, 0.8]], device=DEV), p=2, dim=1)
    return torch.cat([lat.expand(pts.shape[0], -1), pts], 1).contiguous()


@pytest.fixture(scope="module")
def permutation():
    return ((torch.arange(N_ROWS, dtype=torch.int64) * 37) % N_ROWS).to(torch.int32).to(DEV)      # 37 is coprime to 192


@pytest.mark.parametrize("case", list(CASES))
def test_forced_tile_counts_bitwise(case, base_inputs, permutation, monkeypatch):
    n0, n1 = CASES[case]
    assert (tiles(n0), tiles(n1)) == tuple(int(x) for x in case.split("_")[1::2])
    dec, js0, dead0, alive1 = forced_decoder(n0, n1)
    for o in (None, permutation):
        x, alive = coded(base_inputs, ODD, o)
        s0, m0 = forward(dec, x, N_ROWS, False, monkeypatch, o)
        bits0 = layer_bits(m0, N_ROWS, 0)
        assert (bits0[:, js0] == alive[:, None]).all() and not bits0[:, dead0].any()          # layer 0: N features, at the odd places only
        assert (layer_bits(m0, N_ROWS, 1) == alive1.numpy()[None, :]).all()                     # layer 1: M features, at every row
        assert torch.isfinite(s0).all()
        s1, m1 = forward(dec, x, N_ROWS, True, monkeypatch, o)
        assert torch.equal(s0.view(torch.int32), s1.view(torch.int32))
        assert torch.equal(m0, m1)
    x, _ = coded(base_inputs, ODD)
    r0, q0 = forward(dec, x, 65, False, monkeypatch)                                           # a partial second tile
    r1, q1 = forward(dec, x, 65, True, monkeypatch)
    assert torch.equal(r0.view(torch.int32), r1.view(torch.int32)) and torch.equal(q0, q1)
