"""GPU tests of the ordered exact-f32 grid forward (sdfr_mlp_forward_ordered; mlp_kernel.h ORDER): with the rows of a tile chosen
by sdfr_grid_tile_order -- 4x4x4 blocks of the grid instead of 64 consecutive rows -- every sdf value and every saved ReLU mask word of every
row of the launch must be bit for bit what the plain launch writes: per-tile K compaction on and off, with and without a mask buffer.  One BatchRenderer step and a captured BatchRefiner run must not depend on SDFR_FWD_ORDER, and an index outside the order's range
must cost its slot's row and nothing else.

Mask words are compared for the rows of the launch.  The mask buffer is padded to whole 128-row blocks; what a launch leaves in the padding
rows behind its last row (a partial tile writes the bits of mirrored rows up to the end of the tile) is nobody's and nothing reads it."""
import numpy as np
import pytest
import torch

import sdflabel_amd
from sdflabel_amd import _lib
from sdflabel_amd.fixtures import ASSET, ASSET_ELLIPSOID, K_for
from tests.test_gpu_kcompact import grid_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda"
LAT = [[0.3, -0.5, 0.8], [1.0, 0.2, -0.4]]


def _decoder(asset=ASSET):
    d, _ = sdflabel_amd.setup_dsdf(asset + ".pt", precision=torch.float32)
    return d.to(DEV)


@pytest.fixture(scope="module")
def dec():
    return _decoder()


def tile_order(D):
    o = np.empty(D ** 3, np.int32)
    _lib.check(_lib.lib().sdfr_grid_tile_order(D, o.ctypes.data), "sdfr_grid_tile_order")
    return torch.from_numpy(o)


def mask_rows(mw, n, n_layers=8, hp32=16):
    """the mask words of rows 0 .. n-1 (layout v2: [block of 128 rows][layer][row in block][HP / 32 dwords]) as [layer][row][dword]"""
    v = mw.view(-1, n_layers, 128, hp32).permute(1, 0, 2, 3).reshape(n_layers, -1, hp32)
    return v[:, :n]


def launch(dec, inputs, order, monkeypatch, compact=True, masks=True):
    """order None: the plain launch.  sdf starts as NaN and the mask words as zero, so a row never written shows."""
    L = _lib.lib()
    h = dec.handle(torch.device(DEV)).h
    n = inputs.shape[0]
    sdf = torch.full((n,), float("nan"), device=DEV)
    mw = torch.zeros(int(L.sdfr_decoder_mask_words(h, n)), dtype=torch.int32, device=DEV) if masks else None
    monkeypatch.setenv("SDFR_FWD_COMPACT", "1" if compact else "0")
    if order is None:
        _lib.check(L.sdfr_mlp_forward(h, _lib.ptr(inputs), n, _lib.ptr(sdf), _lib.ptr(mw), _lib.stream_ptr()), "sdfr_mlp_forward")
    else:
        _lib.check(L.sdfr_mlp_forward_ordered(h, _lib.ptr(inputs), n, _lib.ptr(sdf), _lib.ptr(mw), _lib.ptr(order), order.shape[0],
                                              _lib.stream_ptr()), "sdfr_mlp_forward_ordered")
    torch.cuda.synchronize()
    return sdf, (mask_rows(mw, n) if masks else None)


def assert_ordered_equals_plain(dec, inputs, order, monkeypatch):
    ref_s, ref_m = launch(dec, inputs, None, monkeypatch)               # the reference: one plain launch, shared by the four variants
    assert torch.isfinite(ref_s).all() and ref_m.shape[1] == inputs.shape[0]
    for compact in (True, False):
        for masks in (True, False):
            s, m = launch(dec, inputs, order, monkeypatch, compact, masks)
            assert torch.equal(ref_s.view(torch.int32), s.view(torch.int32)), (compact, masks)
            if masks:
                assert torch.equal(ref_m, m), (compact, masks)


@pytest.mark.parametrize("D,crops", [(4, 1), (5, 1), (6, 1), (8, 1), (5, 2)])
def test_small_grids_bitwise(dec, D, crops, monkeypatch):
    """D = 4: one tile; D = 5: 125 rows, clipped blocks and a partial last tile; D = 6: 216 rows; D = 8: eight whole blocks; two crops at
    D = 5: G is no multiple of the tile, and tiles span the crops"""
    inp = grid_inputs(LAT[:crops], density=D)
    assert inp.shape[0] == crops * D ** 3
    assert_ordered_equals_plain(dec, inp, tile_order(D).to(DEV), monkeypatch)


@pytest.mark.parametrize("asset", [ASSET, ASSET_ELLIPSOID])
def test_headline_grid_bitwise(asset, monkeypatch):
    inp = grid_inputs(LAT[:1], density=40)
    assert_ordered_equals_plain(_decoder(asset), inp, tile_order(40).to(DEV), monkeypatch)


def test_index_out_of_range_costs_its_own_row_only(dec, monkeypatch):
    """entries G and -1 planted in the order: the launch finishes, the two rows those slots should have named keep the prefill (NaN, zero mask
    words), every other row has the plain launch's bits"""
    D = 6
    inp = grid_inputs(LAT[:2], density=D)
    G = D ** 3
    order = tile_order(D)
    lost = [int(order[70]), int(order[215])]                         # (slot 215: the last one of a crop, in a partial tile of crop 0 / 1)
    order[70], order[215] = G, -1
    ref_s, ref_m = launch(dec, inp, None, monkeypatch)
    s, m = launch(dec, inp, order.to(DEV), monkeypatch)
    gone = torch.zeros(2 * G, dtype=torch.bool, device=DEV)
    for c in range(2):
        for r in lost:
            gone[c * G + r] = True
    assert torch.isnan(s[gone]).all() and int(gone.sum()) == 4
    assert torch.equal(s[~gone].view(torch.int32), ref_s[~gone].view(torch.int32))
    assert not m[:, gone].any() and torch.equal(m[:, ~gone], ref_m[:, ~gone])


def test_batch_renderer_step_does_not_depend_on_the_order(dec, monkeypatch):
    """one full fwd + bwd step at 64x64 pixels, grid 20 (8000 rows = 125 blocks): images, counts, xyzf, gradients, sdf and masks"""
    H = W = 64
    br = sdflabel_amd.BatchRenderer(dec, 20, K_for(H, W), (W, H), 1, device=DEV)
    assert br.fwd_order is not None and torch.equal(br.fwd_order.cpu(), tile_order(20))
    args = (torch.tensor([0.6], device=DEV), torch.tensor([[0.0, 0.0, 3.5]], device=DEV), torch.tensor([LAT[0]], device=DEV))
    res = []
    for on in ("0", "1"):
        monkeypatch.setenv("SDFR_FWD_ORDER", on)
        br.sdf.fill_(float("nan"))
        br.mask_ws.zero_()
        out = br.forward(*args)
        out = {k: v.clone() for k, v in out.items() if torch.is_tensor(v)}
        grads = [g.clone() for g in br.backward(g_color=torch.ones(1, 3, H, W, device=DEV), g_xyzf=torch.ones(1, br.cap, 3, device=DEV))]
        torch.cuda.synchronize()
        res.append((out, grads, br.sdf.clone(), mask_rows(br.mask_ws, 8000).clone()))
    (o0, g0, s0, m0), (o1, g1, s1, m1) = res
    assert int(o1["n"][0]) > 0 and o0.keys() == o1.keys()
    for k in o0:
        assert torch.equal(o0[k], o1[k]), k
    assert len(g0) == len(g1) and len(g0) > 0
    for a, b in zip(g0, g1):
        assert torch.equal(a, b)
    assert torch.isfinite(s1).all() and torch.equal(s0.view(torch.int32), s1.view(torch.int32)) and torch.equal(m0, m1)


def test_captured_refiner_does_not_depend_on_the_order(monkeypatch):
    """three iterations of a captured BatchRefiner (the switch is read when the launch is captured): parameters and losses, bit for bit"""
    from sdflabel_amd.fixtures import crop_params, synthetic_targets
    D, H, W, B = 20, 32, 32, 2
    K = K_for(H, W)
    nocs1, lidar = synthetic_targets(_decoder(), D, K, H, W, DEV)
    res = []
    for on in ("0", "1"):
        monkeypatch.setenv("SDFR_FWD_ORDER", on)
        rf = sdflabel_amd.BatchRefiner(_decoder(), D, K, (H, W), B, lidar_cap=4096, device=DEV)
        rf.set_crops(crop_params(list(range(B))), nocs1.expand(B, 3, H, W), [lidar] * B)
        rf.capture()
        rf.optimize(3)
        rows, l2, l3 = rf.results()
        res.append((rows, l2, l3, rf.br.sdf.clone(), rf.br.color.clone(), rf.br.xyzf.clone(), rf.grads.clone()))
    assert torch.isfinite(res[0][0]).all()
    for a, b in zip(*res):
        assert torch.equal(a, b) or torch.equal(torch.nan_to_num(a), torch.nan_to_num(b)) and torch.equal(torch.isnan(a), torch.isnan(b))
