"""GPU tests of the k-major image of the compacted operand (mlp_kernel.h: kc_store and gemm_kc_body of the 64-row kernels; csrc/kc_slots.h,
sdfr_kcm_*) with survivor patterns that differ from POINT TO POINT of a tile.  The forced-bias patterns of
tests/test_gpu_kc_epilogue.py keep a feature alive or dead at every point; an image that swapped the two point tiles of a row, or the two
lane-group rows of a k step, would pass them.  Here a feature of layer 0 is alive at chosen rows of every 64-row tile only: its weight row is
K on ONE input coordinate and zero elsewhere, its bias 0, and that coordinate (the x column, which a 64-row tile of the grid holds constant
anyway) carries +1 at the rows where the feature lives and -1 elsewhere -- a ReLU of an affine function of true grid coordinates could only
carve a half space, not a single row or alternating rows.  SDFR_FWD_COMPACT=1 must give the sdf bits and mask words of the full chain (=0)
through the plain entry and through sdfr_mlp_forward_ordered (there the coordinate is laid out by tile SLOT, so that the pattern is the same
inside the ordered tiles), and for 1, 63 and 65 rows.  The full chain's mask words of layer 0 must show exactly the forced pattern first."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import sdflabel_amd
from sdflabel_amd.fixtures import ASSET
from tests.test_gpu_kc_epilogue import D, DEV, chain_feature, forward, layer_bits, order  # noqa: F401  (order: fixture)

pytestmark = pytest.mark.gpu
K = 1.0e3
XCOL = 3                                 # inputs = latent (3) | x y z

ROWS = {
    "rows_0_31": list(range(32)),        # point tile 0 only
    "rows_32_63": list(range(32, 64)),   # point tile 1 only
    "row_0": [0], "row_31": [31], "row_32": [32], "row_63": [63],
    "even_rows": list(range(0, 64, 2)),
    "odd_rows": list(range(1, 64, 2)),
}
# forced features as (wave, chain position c = 2 q + g); `alone`: every other feature of these waves is dead at every point
FEATURES = {
    "lane_group_0": ([(w, c) for w in (0, 3, 7) for c in (0, 2, 30, 62)], ()),
    "lane_group_1": ([(w, c) for w in (0, 3, 7) for c in (1, 3, 31, 63)], ()),
    "one_survivor_in_the_wave": ([(2, 20), (5, 13)], (2, 5)),
}


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


def forced_decoder(features, kill_layer3=False):
    d, _ = sdflabel_amd.setup_dsdf(ASSET + ".pt", precision=torch.float32)
    forced, alone = FEATURES[features]
    js = [chain_feature(w, c) for w, c in forced]
    dead = [j for w in alone for j in range(w * 64, w * 64 + 64) if j not in js]
    assert d.lin0.bias.shape[0] == 512
    for j in js:
        set_row(d.lin0, j, XCOL)
    if dead:
        with torch.no_grad():
            d.lin0.bias[dead] -= 1.0e4
    dead3 = []
    if kill_layer3:
        # the layer whose epilogue re-injects the input columns behind its 506 features: few survivors in front of them
        n3 = d.lin3.bias.shape[0]
        assert d.latent_in == [4] and n3 == 512 - 6
        dead3 = [j for j in range(n3) if j % 7]
        with torch.no_grad():
            d.lin3.bias[dead3] -= 1.0e4
    return d.to(DEV), js, dead, dead3


@pytest.fixture(scope="module")
def base_inputs():
    pts = sdflabel_amd.Grid3D(D, DEV).points.detach()
    lat = F.normalize(torch.tensor([[0.3, -0.5, 0.8]], device=DEV), p=2, dim=1)
    return torch.cat([lat.expand(pts.shape[0], -1), pts], 1).contiguous()


def coded(base, rows, order=None):
    """the inputs with +1 / -1 in the x column: +1 where the row's place in its 64-row tile is in `rows`; the place is the row index under
    the plain entry and the slot index under the ordered one (slot j evaluates row order[j]).  Returns inputs and alive[row]."""
    n = base.shape[0]
    place = torch.zeros(64, dtype=torch.bool)
    place[rows] = True
    by_slot = place.repeat(n // 64).to(DEV)
    alive = by_slot
    if order is not None:
        alive = torch.zeros(n, dtype=torch.bool, device=DEV)
        alive[order.long()] = by_slot
    x = base.clone()
    x[:, XCOL] = torch.where(alive, torch.tensor(1.0, device=DEV), torch.tensor(-1.0, device=DEV))
    return x.contiguous(), alive.cpu().numpy()


def compare(dec, js, dead, dead3, base, rows, order, monkeypatch):
    n = base.shape[0]
    for o in (None, order):
        x, alive = coded(base, rows, o)
        s0, m0 = forward(dec, x, n, False, monkeypatch, o)
        bits = layer_bits(m0, n, 0)
        assert (bits[:, js] == alive[:, None]).all()                   # the pattern took hold: these rows and no others
        assert not bits[:, dead].any()
        if dead3:
            assert not layer_bits(m0, n, 3)[:, dead3].any()
        assert torch.isfinite(s0).all()
        s1, m1 = forward(dec, x, n, True, monkeypatch, o)
        assert torch.equal(s0.view(torch.int32), s1.view(torch.int32))
        assert torch.equal(m0, m1)
        if o is None:
            for part in (1, 63, 65):                                   # partial tiles
                r0, q0 = forward(dec, x, part, False, monkeypatch)
                r1, q1 = forward(dec, x, part, True, monkeypatch)
                assert torch.equal(r0.view(torch.int32), r1.view(torch.int32)) and torch.equal(q0, q1)
                assert torch.equal(r0.view(torch.int32), s0[:part].view(torch.int32))


@pytest.mark.parametrize("features", list(FEATURES))
@pytest.mark.parametrize("rows", list(ROWS))
def test_per_point_patterns_bitwise(rows, features, base_inputs, order, monkeypatch):
    dec, js, dead, dead3 = forced_decoder(features)
    compare(dec, js, dead, dead3, base_inputs, ROWS[rows], order, monkeypatch)


def test_per_point_values_at_the_re_injecting_layer(base_inputs, order, monkeypatch):
    """layer 3's epilogue appends the input columns -- the +1 / -1 column among them -- to its features: per-point values of both lane
    groups (features 506-511) that no ReLU has touched, behind a wave with few survivors"""
    dec, js, dead, dead3 = forced_decoder("lane_group_1", kill_layer3=True)
    compare(dec, js, dead, dead3, base_inputs, ROWS["odd_rows"], order, monkeypatch)
