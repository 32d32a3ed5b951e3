"""GPU tests of the band selection and the tile ranking in one launch (sdfr_band_select_rank, sdfr_mlp_forward_balanced_deferred;
csrc/band_rank.hip).

Selection: idx, cnt, slot and the sticky flag are integers -- compared as whole sentinel-filled, guarded arrays with what sdfr_band_select_ex
writes AND with the reference of tests/_surface_ref.py.  Ranking: order, at and last against the ranking launch of sdfr_mlp_forward_balanced at
equal cost words, and against the rule restated with a stable sort; the costs and the control word are zero afterwards.  The renderer: every
output and gradient of two steps bit for bit between the default and SDFR_BAND_FUSED=0 SDFR_JAC_STAGE=0, and the same launch order for the next step."""
import numpy as np
import pytest
import torch

import sdflabel_amd
from sdflabel_amd import _lib
from sdflabel_amd.fixtures import ASSET, K_for
from tests import _surface_ref as R
from tests.test_gpu_fwd_balance import LATS, State, _step, check_state, next_order
from tests.test_gpu_fwd_order import _decoder
from tests.test_gpu_kcompact import grid_inputs
from tests.test_gpu_surface_ref import Guarded, T, _band_call, _band_check, _band_sdf, call, same

pytestmark = pytest.mark.gpu
DEV = "cuda"
F, I = np.float32, np.int32
THR = 0.03
P = _lib.ptr


def _rank_call(sdf_t, G, B, extra, skip, cap, prev, bit, slot=True, state=None, order_rows=0):
    """sdfr_band_select_rank on guarded device copies of `prev`; returns the arrays after the call"""
    d = dict(idx=Guarded(prev["idx"], -9), cnt=Guarded(prev["cnt"], -9), slot=Guarded(prev["slot"], -9) if slot else None,
             over=Guarded(prev["over"], 64))
    te = None if extra is None else T(extra)
    ts = None if skip is None else T(np.asarray(skip, I))
    call("sdfr_band_select_rank", P(sdf_t), G, B, THR, P(te), P(ts), d["idx"].p, cap, d["cnt"].p, d["slot"].p if slot else None, d["over"].p, bit,
         P(state), order_rows)
    return {k: (v.get() if v is not None else None) for k, v in d.items()}


@pytest.mark.parametrize("G", [1, 63, 64, 255, 256, 257, 1023, 1025, 4097, 70000])
def test_selection_equals_band_select_ex(G):
    """B = 1, 2, 3 (odd G: the crops behind the first start off a 16-byte boundary, so their counts take the scalar head and tail); densities
    0 (an empty band), 5 % with +-thr, +-0, +-inf, NaN and the neighbours of thr, 1 (every row); per-crop thr_extra with a crop it empties;
    cap below / at / above the count; skip flags 0 1 0 and none; slot NULL.  1025 and 4097 rows: a last block of one row; 70 000 rows: 69
    blocks per crop."""
    rng = np.random.default_rng(1000 + G)
    for B in (1, 2, 3):
        for dens in (0.0, 0.05, 1.0):
            sdf = _band_sdf(rng, B, G, dens, dens == 0.05)
            sdf_prev = _band_sdf(rng, B, G, 0.3, False)
            extra = np.array([[0.0, -0.04, 0.004][b % 3] for b in range(B)], F)
            skip = np.array([b % 3 == 1 for b in range(B)], I)
            with np.errstate(invalid="ignore"):
                tot = int((np.abs(sdf) < F(F(THR) + extra[:, None])).sum(1).max())
            sdf_t = T(sdf)
            for cap in sorted({max(1, tot - 1), max(1, tot), G}):
                sent = dict(idx=np.full((B, cap), -7, I), cnt=np.full(B, -7, I), slot=np.full((B, G), -7, I), over=np.full(B, 8, I))
                prev = R.band_ref(sdf_prev, THR, None, None, sent, cap, 1)
                for ex, sk, bit in ((None, None, 1), (extra, None, 4), (extra, skip, 2)):
                    tag = "G %d B %d density %g cap %d bit %d" % (G, B, dens, cap, bit)
                    ref = R.band_ref(sdf, THR, ex, sk, prev, cap, bit)
                    old = _band_call("ex", sdf_t, G, B, ex, sk, cap, prev, bit)
                    got = _rank_call(sdf_t, G, B, ex, sk, cap, prev, bit)
                    _band_check(tag + " against sdfr_band_select_ex", got, old)
                    _band_check(tag + " against the reference", got, ref)
            ref = R.band_ref(sdf, THR, extra, skip, prev, cap, 2)
            got = _rank_call(sdf_t, G, B, extra, skip, cap, prev, 2, slot=False)
            _band_check("G %d B %d slot NULL" % (G, B), got, ref)


def test_truncation_flag_stays_after_a_selection_that_fits():
    G, B, cap = 3000, 2, 40
    rng = np.random.default_rng(3)
    dense, thin = _band_sdf(rng, B, G, 0.5, False), _band_sdf(rng, B, G, 0.005, False)
    thin[1] = dense[1]                                            # crop 1 overflows both times, crop 0 only the first time
    state = dict(idx=np.full((B, cap), -7, I), cnt=np.full(B, -7, I), slot=np.full((B, G), -7, I), over=np.zeros(B, I))
    a = _rank_call(T(dense), G, B, None, None, cap, state, 1)
    assert (a["cnt"] > cap).all() and (a["over"] == 1).all()
    b = _rank_call(T(thin), G, B, None, None, cap, a, 2)
    assert b["cnt"][0] <= cap < b["cnt"][1] and b["over"].tolist() == [1, 3]
    _band_check("second selection", b, R.band_ref(thin, THR, None, None, a, cap, 2))


def test_no_rows_and_no_crops():
    """G = 0 zeroes every count (as sdfr_band_select_ex does); B = 0 writes nothing"""
    cnt = torch.full((5,), -7, dtype=torch.int32, device=DEV)
    one = torch.zeros(4, device=DEV)
    call("sdfr_band_select_rank", P(one), 0, 3, THR, None, None, P(cnt), 4, P(cnt[1:]), None, None, 0, None, 0)
    assert cnt.tolist() == [-7, 0, 0, 0, -7]
    call("sdfr_band_select_rank", P(one), 4, 0, THR, None, None, P(cnt), 4, P(cnt[1:]), None, None, 0, None, 0)
    assert cnt.tolist() == [-7, 0, 0, 0, -7]


# ---- the ranking half -----------------------------------------------------------------------------------------------------------------------------

class RawState:
    """a balance state of any order_rows (csrc/tile_balance.h) around a random static order, with the views of tests.test_gpu_fwd_balance.State"""

    def __init__(self, order_rows, seed):
        L = _lib.lib()
        self.G, self.T, self.full = order_rows, (order_rows + 63) // 64, order_rows // 64
        self.fixed = torch.randperm(order_rows, generator=torch.Generator().manual_seed(seed)).to(torch.int32)
        self.buf = torch.full((int(L.sdfr_mlp_balance_bytes(order_rows)) // 4,), -7, dtype=torch.int32, device=DEV)
        _lib.check(L.sdfr_mlp_balance_init(P(self.buf), P(self.fixed.to(DEV)), order_rows, _lib.stream_ptr()), "sdfr_mlp_balance_init")
        torch.cuda.synchronize()
        T_, G = self.T, self.G
        self.cost, self.last, self.at = self.buf[:T_], self.buf[T_:2 * T_], self.buf[2 * T_:3 * T_]
        self.ctl, self.order, self.kept = self.buf[3 * T_:3 * T_ + 4], self.buf[3 * T_ + 4:3 * T_ + 4 + G], self.buf[3 * T_ + 4 + G:]


def _crafted(T_, kind, rng):
    if kind == "zero":
        return np.zeros(T_, I)
    if kind == "ties":                                            # three values only, one of them negative: the static index decides
        return rng.choice(np.array([-16, 112, 3584], I), T_)
    if kind == "ascending":                                       # the full chunks end up reversed
        return (np.arange(T_) * 16).astype(I)
    return rng.integers(-2 ** 31, 2 ** 31 - 1, T_).astype(I)


@pytest.mark.parametrize("order_rows", [64, 729, 1331, 1728, 64000])
def test_ranking_alone_on_crafted_costs(order_rows):
    """B = 0: the launch is the ranking alone, on exactly the words the test wrote.  T = 1; 12 with a partial chunk of 25; 21 (not a multiple
    of 4) with a partial chunk of 51; 27 without; 1000.  Each state is ranked four times in a row: every call starts from the order the last left."""
    st = RawState(order_rows, order_rows)
    rng = np.random.default_rng(order_rows)
    none = torch.zeros(4, device=DEV)
    for kind in ("zero", "ties", "ascending", "random"):
        cost = _crafted(st.T, kind, rng)
        st.cost.copy_(torch.from_numpy(cost).to(DEV))
        call("sdfr_band_select_rank", P(none), 4, 0, THR, None, None, P(none), 4, P(none), None, None, 0, P(st.buf), order_rows)
        o, at = next_order(cost, st)
        assert np.array_equal(st.order.cpu().numpy(), o) and np.array_equal(st.at.cpu().numpy(), at), kind
        assert np.array_equal(st.last.cpu().numpy(), cost), kind
        check_state(st)
        if kind == "zero":
            assert torch.equal(st.order.cpu(), st.fixed)
        if kind == "ascending" and st.full > 1:
            assert at[0] == st.full - 1


def test_orders_beyond_the_ranked_size_are_left_alone():
    order_rows = 4097 * 64
    st = RawState(order_rows, 1)
    st.cost.copy_(torch.arange(st.T, dtype=torch.int32, device=DEV))
    before = st.buf.clone()
    none = torch.zeros(4, device=DEV)
    call("sdfr_band_select_rank", P(none), 4, 0, THR, None, None, P(none), 4, P(none), None, None, 0, P(st.buf), order_rows)
    assert torch.equal(st.buf, before)


@pytest.fixture(scope="module")
def dec():
    return _decoder(ASSET)


@pytest.mark.parametrize("D", [4, 9, 40])
def test_deferred_forward_and_rank_equal_the_balanced_forward(dec, D):
    """order_rows 64, 729 and 64 000: crafted words in the costs, then sdfr_mlp_forward_balanced on one state and
    sdfr_mlp_forward_balanced_deferred + sdfr_band_select_rank on another.  Two rounds (the second runs a moved order): equal sdf bits, and the
    whole states equal word for word -- order, at, last, zero costs, ctl 0.  The band of the same launch equals sdfr_band_select_ex's."""
    L = _lib.lib()
    h = dec.handle(torch.device(DEV)).h
    G = D ** 3
    a, b = State(D), State(D)
    rng = np.random.default_rng(D)
    cap = G
    for rnd, kind in enumerate(("ties", "random")):
        inp = grid_inputs([LATS[rnd]], density=D)
        cost = torch.from_numpy(_crafted(a.T, kind, rng)).to(DEV)
        a.cost.copy_(cost)
        b.cost.copy_(cost)
        sa, sb = torch.full((G,), float("nan"), device=DEV), torch.full((G,), float("nan"), device=DEV)
        call("sdfr_mlp_forward_balanced", h, P(inp), G, P(sa), None, P(a.buf), G)
        call("sdfr_mlp_forward_balanced_deferred", h, P(inp), G, P(sb), None, P(b.buf), G)
        assert torch.equal(sa.view(torch.int32), sb.view(torch.int32)) and torch.isfinite(sa).all()
        assert b.cost.cpu().numpy().astype(np.int64).sum() != cost.cpu().numpy().astype(np.int64).sum()      # the tiles did add their costs
        sent = dict(idx=np.full((1, cap), -7, I), cnt=np.full(1, -7, I), slot=np.full((1, G), -7, I), over=np.zeros(1, I))
        old = _band_call("ex", sa, G, 1, None, None, cap, sent, 1)
        got = _rank_call(sb, G, 1, None, None, cap, sent, 1, state=b.buf, order_rows=G)
        _band_check("D %d round %d" % (D, rnd), got, old)
        assert torch.equal(a.buf, b.buf), (D, rnd)
        check_state(b)
        assert np.array_equal(b.order.cpu().numpy(), next_order(b.last.cpu().numpy(), b)[0])


@pytest.mark.parametrize("D", [8, 12])
def test_renderer_steps_equal_the_separate_launches(dec, D, monkeypatch):
    """BatchRenderer, one 64x64 crop: two forward and backward steps with SDFR_BAND_FUSED=0 SDFR_JAC_STAGE=0 and two with the default on a second renderer --
    every output and gradient bit for bit, and the same state of the launch order (so the next step launches the same order)."""
    H = W = 64
    res = {}
    for fused in ("0", "1"):
        monkeypatch.setenv("SDFR_BAND_FUSED", fused)
        monkeypatch.setenv("SDFR_JAC_STAGE", fused)                 # (the Jacobian's stage switched with it: the old path whole)
        br = sdflabel_amd.BatchRenderer(dec, D, K_for(H, W), (W, H), 1, device=DEV)
        steps = []
        for s in range(2):
            args = (torch.tensor([0.6 + 0.1 * s], device=DEV), torch.tensor([[0.0, 0.0, 3.5]], device=DEV), torch.tensor([LATS[s]], device=DEV))
            steps.append(_step(br, args, H, W))
        torch.cuda.synchronize()
        res[fused] = (steps, br.fwd_balance.clone(), br.sdf.clone(), br.J.clone(), br.idx.clone())
    (s0, st0, sdf0, J0, idx0), (s1, st1, sdf1, J1, idx1) = res["0"], res["1"]
    for (o0, g0), (o1, g1) in zip(s0, s1):
        assert o0.keys() == o1.keys() and all(same(o0[k].cpu().numpy(), o1[k].cpu().numpy()) for k in o0)
        assert len(g0) == len(g1) and all(same(x.cpu().numpy(), y.cpu().numpy()) for x, y in zip(g0, g1))
    assert int(s1[-1][0]["n"][0]) > 0
    T_ = (D ** 3 + 63) // 64
    assert torch.equal(st0, st1) and st1[T_:2 * T_].all() and not st1[:T_].any()      # ranked from the second step's costs, which are zeroed
    assert same(sdf0.cpu().numpy(), sdf1.cpu().numpy()) and same(J0.cpu().numpy(), J1.cpu().numpy()) and torch.equal(idx0, idx1)
