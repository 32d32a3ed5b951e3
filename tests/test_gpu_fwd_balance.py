"""GPU tests of the grid forward whose launch order follows the last pass (sdfr_mlp_forward_balanced; csrc/tile_balance.h).
Whatever the state holds, every sdf value and every mask word is bit for bit what sdfr_mlp_forward_ordered writes on the static order; the
cost a launch reports for a chunk is the header's definition restated from that launch's OWN mask words (the K extent of the seven compacted
layers: features alive in some row of the tile plus the re-injected input columns, padded to 16); and the order of the next launch is the
stable descending sort of those costs applied to whole chunks of the static order.

Grids: D = 8 (8 full tiles), D = 9 (729 rows: clipped blocks, 11 full tiles and a partial one of 25 rows whose other slots read the crop's
row 0), D = 12 (27 tiles); both committed decoders."""
import warnings

import numpy as np
import pytest
import torch

import sdflabel_amd
from sdflabel_amd import _lib
from sdflabel_amd.fixtures import ASSET, ASSET_ELLIPSOID, K_for
from tests.test_gpu_fwd_order import _decoder, mask_rows, tile_order
from tests.test_gpu_kcompact import grid_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda"
LATS = [[0.3, -0.5, 0.8], [1.0, 0.2, -0.4], [-0.6, 0.7, 0.1]]
P = _lib.ptr


@pytest.fixture(scope="module")
def decs():
    return {ASSET: _decoder(ASSET), ASSET_ELLIPSOID: _decoder(ASSET_ELLIPSOID)}


class State:
    """the balance state of one order and views of its fields (csrc/tile_balance.h)"""

    def __init__(self, D):
        L = _lib.lib()
        self.G, self.T, self.full = D ** 3, (D ** 3 + 63) // 64, D ** 3 // 64
        self.fixed = tile_order(D)
        self.fixed_dev = self.fixed.to(DEV)
        nbytes = int(L.sdfr_mlp_balance_bytes(self.G))
        assert nbytes == 4 * (3 * self.T + 4 + 2 * self.G)
        self.buf = torch.full((nbytes // 4,), -7, dtype=torch.int32, device=DEV)
        _lib.check(L.sdfr_mlp_balance_init(P(self.buf), P(self.fixed_dev), self.G, _lib.stream_ptr()), "sdfr_mlp_balance_init")
        T, G = self.T, self.G
        self.cost, self.last, self.at = self.buf[:T], self.buf[T:2 * T], self.buf[2 * T:3 * T]
        self.ctl, self.order, self.kept = self.buf[3 * T:3 * T + 4], self.buf[3 * T + 4:3 * T + 4 + G], self.buf[3 * T + 4 + G:]


def run(dec, inputs, st=None, order=None):
    """one launch into NaN / zero prefilled outputs -> sdf bits, mask rows"""
    L = _lib.lib()
    h = dec.handle(torch.device(DEV)).h
    n = inputs.shape[0]
    sdf = torch.full((n,), float("nan"), device=DEV)
    mw = torch.zeros(int(L.sdfr_decoder_mask_words(h, n)), dtype=torch.int32, device=DEV)
    if st is not None:
        _lib.check(L.sdfr_mlp_forward_balanced(h, P(inputs), n, P(sdf), P(mw), P(st.buf), st.G, _lib.stream_ptr()), "sdfr_mlp_forward_balanced")
    else:
        _lib.check(L.sdfr_mlp_forward_ordered(h, P(inputs), n, P(sdf), P(mw), P(order), order.shape[0], _lib.stream_ptr()), "sdfr_mlp_forward_ordered")
    torch.cuda.synchronize()
    return sdf.view(torch.int32), mask_rows(mw, n)


_static = {}


def static_reference(decs, asset, D, lat):
    """sdfr_mlp_forward_ordered on the static order: computed once per case, shared, never written"""
    key = (asset, D, tuple(map(tuple, lat)))
    if key not in _static:
        s, m = run(decs[asset], grid_inputs(lat, density=D), order=tile_order(D).to(DEV))
        assert torch.isfinite(s.view(torch.float32)).all()
        _static[key] = (s, m)
    return _static[key]


def expected_costs(dec, m, order_before, at_before, st, crops=1):
    """the header's cost from the launch's own mask words m [layer][row][16]: per tile and compacted layer l = 0 .. 6 the features whose bit
    is set in some row of the tile, plus the input columns re-injected in front of layer l + 1, padded to 16; slots of a partial tile
    beyond the launch's rows read the crop's row 0.  Added to the word of the chunk at the tile's place, over the crops."""
    inj = [n for n, _ in dec._inject_table()]
    G, T = st.G, st.T
    mm = m.cpu().numpy().view(np.uint32)
    assert mm.shape[0] == 8 and len(inj) >= 8
    cost = np.zeros(T, np.int64)
    for c in range(crops):
        for p in range(T):
            rows = order_before[p * 64:(p + 1) * 64].astype(np.int64)
            if rows.shape[0] < 64:
                rows = np.concatenate([rows, [0]])
            k = 0
            for l in range(7):
                alive = int(sum(bin(int(w)).count("1") for w in np.bitwise_or.reduce(mm[l, c * G + rows], axis=0)))
                k += (alive + inj[l + 1] + 15) // 16 * 16
            cost[at_before[p]] += k
    return cost


def next_order(cost, st):
    rank_order = np.argsort(-cost[:st.full].astype(np.int64), kind="stable")
    fx = st.fixed.numpy()
    return np.concatenate([fx[c * 64:(c + 1) * 64] for c in rank_order] + [fx[st.full * 64:]]), np.concatenate([rank_order, np.arange(st.full, st.T)])


def check_state(st):
    """a permutation of the static order with whole chunks, the partial chunk last, at[] naming the chunk at each place; the kept copy intact"""
    o, at, fx = st.order.cpu().numpy(), st.at.cpu().numpy(), st.fixed.numpy()
    assert np.array_equal(st.kept.cpu().numpy(), fx) and np.array_equal(np.sort(at), np.arange(st.T))
    for p in range(st.T):
        assert np.array_equal(o[p * 64:(p + 1) * 64], fx[at[p] * 64:(at[p] + 1) * 64]), p
    assert at[st.T - 1] == st.T - 1 or st.T == st.full
    assert not st.cost.any() and not st.ctl.any()


@pytest.mark.parametrize("D", [8, 9, 12])
@pytest.mark.parametrize("asset", [ASSET, ASSET_ELLIPSOID])
def test_three_launches_bits_costs_and_next_order(decs, asset, D):
    """1, 2, 3: three consecutive balanced launches with three latents"""
    dec, st = decs[asset], State(D)
    assert torch.equal(st.order.cpu(), st.fixed) and torch.equal(st.kept.cpu(), st.fixed) and not st.cost.any() and not st.last.any()
    assert torch.equal(st.at.cpu(), torch.arange(st.T, dtype=torch.int32))
    moved = 0
    for i, lat in enumerate(LATS):
        ref_s, ref_m = static_reference(decs, asset, D, [lat])
        order_before, at_before = st.order.cpu().numpy(), st.at.cpu().numpy()
        s, m = run(dec, grid_inputs([lat], density=D), st)
        assert torch.equal(s, ref_s) and torch.equal(m, ref_m), i
        want = expected_costs(dec, m, order_before, at_before, st)
        got = st.last.cpu().numpy()
        print("%s D = %d launch %d: costs %d .. %d" % (asset.rsplit("/", 1)[-1], D, i, got.min(), got.max()))
        assert np.array_equal(got, want), (i, got, want)
        assert want.min() >= 7 * 16 and want.max() <= 7 * 512 and not (want % 16).any()
        o, at = next_order(got, st)
        assert np.array_equal(st.order.cpu().numpy(), o) and np.array_equal(st.at.cpu().numpy(), at), i
        check_state(st)
        moved += int((at != np.arange(st.T)).sum())
    assert moved > 0                                            # the costs differ between tiles: the order did move


def test_state_of_one_decoder_used_with_the_other(decs):
    """4"""
    D, st = 12, State(12)
    run(decs[ASSET], grid_inputs([LATS[0]], density=D), st)
    assert not torch.equal(st.order.cpu(), st.fixed)
    ref_s, ref_m = static_reference(decs, ASSET_ELLIPSOID, D, [LATS[1]])
    s, m = run(decs[ASSET_ELLIPSOID], grid_inputs([LATS[1]], density=D), st)
    assert torch.equal(s, ref_s) and torch.equal(m, ref_m)
    check_state(st)


@pytest.mark.parametrize("D", [9, 12])
def test_overwritten_cost_words(decs, D):
    """5: random integers in the cost words between launches, twice: the same bits, a valid permutation, the sort of what the words held"""
    st = State(D)
    g = torch.Generator().manual_seed(D)
    inp = grid_inputs([LATS[2]], density=D)
    ref_s, ref_m = static_reference(decs, ASSET, D, [LATS[2]])
    for _ in range(2):
        junk = torch.randint(-2 ** 31, 2 ** 31 - 1, (st.T,), generator=g, dtype=torch.int64).to(torch.int32)
        st.cost.copy_(junk.to(DEV))
        order_before, at_before = st.order.cpu().numpy(), st.at.cpu().numpy()
        s, m = run(decs[ASSET], inp, st)
        assert torch.equal(s, ref_s) and torch.equal(m, ref_m)
        check_state(st)
        want = (junk.numpy().astype(np.int64) + expected_costs(decs[ASSET], m, order_before, at_before, st)).astype(np.int32)    # (wraps)
        assert np.array_equal(st.last.cpu().numpy(), want)
        assert np.array_equal(st.order.cpu().numpy(), next_order(want, st)[0])


def test_two_crops_sum_their_costs(decs):
    """6: n = 2 order_rows"""
    D, st = 8, State(8)
    inp = grid_inputs(LATS[:2], density=D)
    ref_s, ref_m = static_reference(decs, ASSET, D, LATS[:2])
    for _ in range(2):                                          # (the second launch runs a moved order)
        order_before, at_before = st.order.cpu().numpy(), st.at.cpu().numpy()
        s, m = run(decs[ASSET], inp, st)
        assert torch.equal(s, ref_s) and torch.equal(m, ref_m)
        want = expected_costs(decs[ASSET], m, order_before, at_before, st, crops=2)
        assert np.array_equal(st.last.cpu().numpy(), want) and want.min() >= 2 * 7 * 16
        check_state(st)


def _step(br, args, H, W):
    out = br.forward(*args)
    out = {k: v.clone() for k, v in out.items() if torch.is_tensor(v)}
    grads = [g.clone() for g in br.backward(g_color=torch.ones(1, 3, H, W, device=DEV), g_xyzf=torch.ones(1, br.cap, 3, device=DEV))]
    return out, grads


def count_syncs(fn):
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            out = fn()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    return sum("synchroniz" in str(x.message).lower() for x in w), out


def test_renderer_switch_graph_replay_and_host_syncs(decs, monkeypatch):
    """7, 8: a BatchRenderer step at 64x64 pixels, grid 20 (125 tiles).  SDFR_FWD_BALANCE=0 leaves the state alone and gives the same
    outputs; the balanced step, captured on one stream and replayed three times, gives the eager bits each time while the order keeps
    following the costs; a step synchronises with the host as often as the static one."""
    H = W = 64
    dec = decs[ASSET]
    br = sdflabel_amd.BatchRenderer(dec, 20, K_for(H, W), (W, H), 1, device=DEV)
    T = 125
    args = (torch.tensor([0.6], device=DEV), torch.tensor([[0.0, 0.0, 3.5]], device=DEV), torch.tensor([LATS[0]], device=DEV))
    at = lambda: br.fwd_balance[2 * T:3 * T].cpu()
    ident = torch.arange(T, dtype=torch.int32)
    assert br.fwd_balance.shape[0] == 3 * T + 4 + 2 * 8000 and torch.equal(at(), ident)
    monkeypatch.setenv("SDFR_FWD_BALANCE", "0")
    syncs0, (o0, g0) = count_syncs(lambda: _step(br, args, H, W))
    s0, m0 = br.sdf.clone(), mask_rows(br.mask_ws, 8000).clone()
    assert torch.equal(at(), ident)                              # the static order ran, nothing was ranked
    monkeypatch.setenv("SDFR_FWD_BALANCE", "1")
    br.sdf.fill_(float("nan"))
    br.mask_ws.zero_()
    syncs1, (o1, g1) = count_syncs(lambda: _step(br, args, H, W))
    torch.cuda.synchronize()
    assert not torch.equal(at(), ident) and syncs1 == syncs0
    assert torch.equal(s0.view(torch.int32), br.sdf.view(torch.int32)) and torch.equal(m0, mask_rows(br.mask_ws, 8000))
    assert o0.keys() == o1.keys() and all(torch.equal(o0[k], o1[k]) for k in o0) and all(torch.equal(a, b) for a, b in zip(g0, g1))
    # capture on one stream, replay three times
    ones3, onesx = torch.ones(1, 3, H, W, device=DEV), torch.ones(1, br.cap, 3, device=DEV)
    replay = br.capture(lambda out: dict(g_color=ones3, g_xyzf=onesx))
    for _ in range(3):
        br.sdf.fill_(float("nan"))
        br.mask_ws.zero_()
        for g in (br.g_yaw, br.g_trans, br.g_latent):
            g.fill_(float("nan"))
        replay()
        torch.cuda.synchronize()
        assert torch.equal(s0.view(torch.int32), br.sdf.view(torch.int32)) and torch.equal(m0, mask_rows(br.mask_ws, 8000))
        assert all(torch.equal(a, b) for a, b in zip(g0, (br.g_yaw, br.g_trans, br.g_latent)))
        assert torch.equal(o0["color"], br.color) and torch.equal(o0["xyzf"], br.xyzf) and torch.equal(o0["n"], br.cnt)
        assert torch.equal(torch.sort(at()).values, ident) and not br.fwd_balance[:T].any() and not br.fwd_balance[3 * T:3 * T + 4].any()


def test_argument_checks_come_before_any_device_call():
    """9"""
    import ctypes
    L = _lib.lib()
    fake = ctypes.create_string_buffer(64)
    p = ctypes.addressof(fake)
    cases = [((None, p, 64, p, None, p, 64, None), b"NULL"), ((p, None, 64, p, None, p, 64, None), b"NULL"),
             ((p, p, 64, None, None, p, 64, None), b"NULL"), ((p, p, 64, p, None, None, 64, None), b"NULL"),
             ((p, p, 64, p, None, p, 0, None), b"order_rows=0"), ((p, p, 64, p, None, p, -5, None), b"order_rows=-5"),
             ((p, p, 100, p, None, p, 64, None), b"not a multiple"), ((p, p, -64, p, None, p, 64, None), b"out of range")]
    for args, msg in cases:
        assert L.sdfr_mlp_forward_balanced(*args) == -1, args
        assert msg in L.sdfr_last_error(), (msg, L.sdfr_last_error())
    assert L.sdfr_mlp_balance_init(None, p, 64, None) == -1 and b"NULL" in L.sdfr_last_error()
    assert L.sdfr_mlp_balance_init(p, p, 0, None) == -1 and b"order_rows=0" in L.sdfr_last_error()
