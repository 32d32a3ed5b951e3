"""The band-selection / candidate-reuse bookkeeping kernels (csrc/surface.hip) and the parameter glue with the fused backward tail
(csrc/params.hip) against the references of tests/_surface_ref.py, through the C ABI.

Selection, candidate, guard and audit outputs are integers or float32 results of one rounding: compared BIT FOR BIT, every output array
sentinel-filled before the call and compared as a whole (so a write beyond cnt / cap / the documented padding fails), with a guard row in
front of and behind every array.  Float results are judged per element against c * eps32 * mass, c = half the number of roundings on the
longest path, counted in a comment beside each call.  Figures of one run: profiles/surface_tests_notes.md (`pytest -s`, lines SURFTEST)."""
import math

import numpy as np
import pytest
import torch

from sdflabel_amd import _lib
from tests import _loss_ref as LR
from tests import _splat_ref as SR
from tests import _surface_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
F = np.float32
I = np.int32
THR = 0.03
EPS32 = SR.EPS32


_alive = []


def T(a):
    """device copy; kept alive until the end of the next call() (a temporary handed over as `P(T(x))` must outlive the launch that reads it)"""
    t = torch.as_tensor(np.ascontiguousarray(a), device=DEV)
    _alive.append(t)
    return t


def N(t):
    return t.detach().cpu().numpy()


P = _lib.ptr


def call(name, *args):
    _lib.check(getattr(_lib.lib(), name)(*args, _lib.stream_ptr()), name)
    torch.cuda.synchronize()
    del _alive[:]


def same(a, b):
    """equal bits (a NaN equals a NaN)"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    nan = np.isnan(a)
    return bool(np.array_equal(nan, np.isnan(b)) and np.array_equal(a.view(np.uint32)[~nan], b.view(np.uint32)[~nan]))


class Guarded:
    """a device array of B rows with one sentinel row in front and one behind; get() returns the B rows after checking the two"""

    def __init__(self, a, fill):
        a = np.ascontiguousarray(a)
        full = np.empty((a.shape[0] + 2,) + a.shape[1:], a.dtype)
        full[...] = fill
        full[1:-1] = a
        self.guard = full[0].copy()
        self.full = T(full)
        self.t = self.full[1:-1]

    @property
    def p(self):
        return self.t.data_ptr()

    def get(self):
        f = N(self.full)
        assert same(f[0], self.guard) and same(f[-1], self.guard), "a guard row was written"
        return f[1:-1]


def judge(what, got, ref, mass, c):
    """every element within c eps32 mass of the reference; returns the largest error in those units"""
    mass = np.atleast_1d(np.asarray(mass, np.float64))
    got = np.asarray(got, np.float64).reshape(mass.shape)
    ref = np.asarray(ref, np.float64).reshape(mass.shape)
    assert np.isfinite(got).all(), what
    u = SR.unit_error(got, ref, mass, 1.0)
    worst = float(u.max()) if u.size else 0.0
    i = np.unravel_index(int(u.argmax()), u.shape) if u.size else ()
    print("SURFTEST %s: max error %.3g units (bound %.3g)" % (what, worst, c))
    assert worst <= c, "%s: element %s is %.3g units of eps32 mass from the reference (bound %.3g): got %r, reference %r, mass %r" % (
        what, i, worst, c, got[i], ref[i], mass[i])
    return worst


# ---- band selection ---------------------------------------------------------------------------------------------------------------------------

def _band_sdf(rng, B, G, dens, specials):
    inside = rng.uniform(-0.99, 0.99, (B, G)) * THR
    outside = np.where(rng.random((B, G)) < 0.5, -1.0, 1.0) * rng.uniform(1.01 * THR, 1.0, (B, G))
    sdf = np.where(rng.random((B, G)) < dens, inside, outside).astype(F)
    if specials and G >= 16:
        t = F(THR)
        below = np.nextafter(t, F(0))
        vals = np.array([t, -t, 0.0, -0.0, np.inf, -np.inf, np.nan, below, -below, np.nextafter(t, F(1))], F)
        for b in range(B):
            sdf[b, rng.choice(G, vals.size, replace=False)] = vals
    return sdf


def _band_call(entry, sdf_t, G, B, extra, skip, cap, prev, bit, slot=True):
    """one entry point on device copies of `prev` (guarded); returns the arrays after the call"""
    d = dict(idx=Guarded(prev["idx"], -9), cnt=Guarded(prev["cnt"], -9), slot=Guarded(prev["slot"], -9) if slot else None,
             over=Guarded(prev["over"], 64))
    scratch = torch.full((B * ((G + 255) // 256) + 1,), -3, dtype=torch.int32, device=DEV)
    te = None if extra is None else T(extra)
    ts = None if skip is None else T(np.asarray(skip, I))
    sl = d["slot"].p if slot else None
    if entry == "select":
        call("sdfr_band_select", P(sdf_t), G, B, THR, d["idx"].p, cap, d["cnt"].p, sl, P(scratch))
    elif entry == "margin":
        call("sdfr_band_select_margin", P(sdf_t), G, B, THR, P(te), d["idx"].p, cap, d["cnt"].p, sl, P(scratch))
    elif entry == "skip":
        call("sdfr_band_select_skip", P(sdf_t), G, B, THR, P(te), P(ts), d["idx"].p, cap, d["cnt"].p, sl, P(scratch))
    else:
        call("sdfr_band_select_ex", P(sdf_t), G, B, THR, P(te), P(ts), d["idx"].p, cap, d["cnt"].p, sl, P(scratch), d["over"].p, bit)
    assert int(scratch[-1]) == -3
    return {k: (v.get() if v is not None else None) for k, v in d.items()}


def _band_check(tag, got, ref):
    for k in ("idx", "cnt", "slot", "over"):
        if ref[k] is not None and got[k] is not None:
            assert same(got[k], ref[k]), "%s: %s differs at %s" % (tag, k, np.argwhere(got[k] != ref[k])[:4].tolist())


BAND_G = [1, 255, 256, 257, 1023, 1024, 1025, 2049, 3072, 65536, 65537, 70000]


@pytest.mark.parametrize("G", BAND_G)
def test_band_selection_every_entry_point(G):
    """sdfr_band_select, _margin, _skip and _ex (one workgroup per crop: skip flags and B <= 8; two kernels: B = 9 or no skip flags) against
    band_ref: idx, cnt, slot and the flag as whole arrays on top of a different previous selection, densities 0 / 5 % / 1 (the 5 % grids hold
    +-thr, +-0, +-inf, NaN and the neighbours of thr), per-crop thr_extra with a crop it empties, cap below / at / above the count, skip
    pattern 0 1 0.  G > 1024 takes further rounds of the one-workgroup form; 70 000 rows are 274 blocks, so blocks 257 and later take the second
    trip of the two-kernel form's offset sum (65 537 rows, 257 blocks, are one short of it: block 256 sums exactly 256 counts)."""
    rng = np.random.default_rng(G)
    ncase = 0
    for B in ((1, 2, 9) if G <= 3072 else (1, 2)):
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
                zero = np.zeros(B, I)
                res = {}
                for entry, ex, sk, bit in (("select", None, None, 0), ("margin", extra, None, 0), ("skip", extra, skip, 0),
                                           ("ex_skip", extra, skip, 2), ("ex_noskip", extra, None, 4), ("ex_zeroskip", extra, zero, 4)):
                    ref = R.band_ref(sdf, THR, ex, sk, prev, cap, bit)
                    if not entry.startswith("ex"):
                        ref["over"] = prev["over"]
                    got = _band_call(entry, sdf_t, G, B, ex, sk, cap, prev, bit)
                    _band_check("%s G %d B %d density %g cap %d" % (entry, G, B, dens, cap), got, ref)
                    res[entry] = got
                    ncase += 1
                # the two dispatch paths of _ex at equal inputs (B <= 8: one workgroup per crop against two kernels)
                for k in ("idx", "cnt", "slot", "over"):
                    assert same(res["ex_noskip"][k], res["ex_zeroskip"][k]), k
                assert (res["ex_noskip"]["cnt"] > cap).any() == (cap < tot)
            # slot == NULL
            ref = R.band_ref(sdf, THR, extra, skip, prev, cap, 2)
            got = _band_call("ex", sdf_t, G, B, extra, skip, cap, prev, 2, slot=False)
            _band_check("no slot", got, ref)
    print("SURFTEST band G %d: %d calls compared" % (G, ncase))


def test_band_flag_is_sticky_and_keeps_the_other_bit():
    rng = np.random.default_rng(5)
    for B, G in ((2, 3000), (9, 700)):
        sdf = _band_sdf(rng, B, G, 0.3, False)
        few = sdf.copy(); few[:, 5:] = 1.0
        cap = 40
        st = dict(idx=np.full((B, cap), -7, I), cnt=np.full(B, -7, I), slot=np.full((B, G), -7, I), over=np.full(B, 4, I))
        zero = np.zeros(B, I)
        for data, bit in ((sdf, 1), (few, 1), (sdf, 2), (few, 2)):
            ref = R.band_ref(data, THR, None, zero, st, cap, bit)
            got = _band_call("ex", T(data), G, B, None, zero, cap, st, bit)
            _band_check("sticky", got, ref)
            st = got
        assert (st["over"] == 7).all() and (st["cnt"] <= 5).all()


def test_band_in_the_first_or_the_last_block_only():
    """the whole band in the last 256-row block (every other block contributes 0 to its offset) and in the first (every later block's offset is
    the whole count), at G = 70 000: 274 blocks, so the offset sum takes its second trip"""
    G, B, cap = 70000, 2, 300
    sdf = np.full((B, G), 0.5, F)
    sdf[0, G - 100:] = 0.01
    sdf[1, :256] = -0.01
    st = dict(idx=np.full((B, cap), -7, I), cnt=np.full(B, -7, I), slot=np.full((B, G), -7, I), over=np.zeros(B, I))
    ref = R.band_ref(sdf, THR, None, None, st, cap, 1)
    assert ref["cnt"].tolist() == [100, 256]
    _band_check("two kernels", _band_call("select", T(sdf), G, B, None, None, cap, st, 0), dict(ref, over=st["over"]))
    _band_check("one workgroup", _band_call("ex", T(sdf), G, B, None, np.zeros(B, I), cap, st, 1), ref)
    sdf[1, 256:300] = 0.0                        # 300 rows against cap 300, then 301
    sdf[0, :] = 0.5; sdf[0, 69887] = 0.0; sdf[0, 69888] = 0.0       # one row on either side of the last block's first row
    ref = R.band_ref(sdf, THR, None, None, st, cap, 1)
    assert ref["cnt"].tolist() == [2, 300] and not ref["over"].any()
    _band_check("two kernels", _band_call("ex", T(sdf), G, B, None, None, cap, st, 1), ref)
    sdf[1, 65536] = 0.0
    ref = R.band_ref(sdf, THR, None, None, st, cap, 1)
    assert ref["cnt"].tolist() == [2, 301] and ref["over"].tolist() == [0, 1] and ref["slot"][1, 65536] == -1
    _band_check("two kernels", _band_call("ex", T(sdf), G, B, None, None, cap, st, 1), ref)
    _band_check("one workgroup", _band_call("ex", T(sdf), G, B, None, np.zeros(B, I), cap, st, 1), ref)


# ---- candidate chain --------------------------------------------------------------------------------------------------------------------------

def _candidates(rng, B, G, stride):
    return np.stack([np.sort(rng.choice(G, stride, replace=False)) for _ in range(B)]).astype(I)


def test_candidate_band_against_the_reference_and_the_three_launches():
    """sdfr_candidate_band with 0, 1, 1023, 1024, 1025 and 2500 candidates (round boundaries of its 1024-row walk), more candidates than the
    stride (flag 2, clamped) and a band above cap (flag 1): grid values, idx, pos, cnt and the flag; equal to sdfr_scatter_values +
    sdfr_band_select + sdfr_candidate_band_map on the same data"""
    rng = np.random.default_rng(11)
    ns = [0, 1, 1023, 1024, 1025, 2500, 3000]
    B, G, stride, cap = len(ns), 4000, 2560, 600
    ccnt = np.array(ns, I)
    cidx = _candidates(rng, B, G, stride)
    csdf = (rng.uniform(-2, 2, (B, stride)) * THR).astype(F)
    csdf[1, 0] = 0.01
    csdf[5, [3, 1023, 1024, 2047, 2048, 2499]] = np.array([np.nan, np.inf, THR, -0.0, np.nextafter(F(THR), F(0)), 0.0], F)
    grid = rng.uniform(0.2, 0.3, (B, G)).astype(F)
    prev = dict(idx=np.full((B, cap), -7, I), pos=np.full((B, cap), -7, I), cnt=np.full(B, -7, I), over=np.array([4, 0, 0, 4, 0, 0, 4], I))
    rgrid, ref = R.candidate_band_ref(grid, csdf, cidx, stride, ccnt, THR, cap, prev)
    assert (ref["over"] & 1).tolist() == [0, 0, 0, 0, 0, 1, 1] and (ref["over"] & 2).tolist() == [0] * 6 + [2] and ref["cnt"][2] > 400
    d = {k: Guarded(v, -9) for k, v in prev.items()}
    tg = Guarded(grid, 77.0)
    tcs, tci, tcc = T(csdf), T(cidx), T(ccnt)
    call("sdfr_candidate_band", tg.p, P(tcs), P(tci), G, B, stride, P(tcc), THR, d["idx"].p, cap, d["cnt"].p, d["pos"].p, d["over"].p)
    assert same(tg.get(), rgrid)
    for k in prev:
        assert same(d[k].get(), ref[k]), k
    # the three launches it replaces
    tg2 = Guarded(grid, 77.0)
    call("sdfr_scatter_values", tg2.p, P(tcs), P(tci), G, B, stride, P(tcc))
    assert same(tg2.get(), R.scatter_values_ref(grid, csdf, cidx, stride, ccnt)) and same(tg2.get(), rgrid)
    b_idx, b_cnt = Guarded(prev["idx"], -9), Guarded(prev["cnt"], -9)
    scratch = torch.zeros((B * 16,), dtype=torch.int32, device=DEV)
    call("sdfr_band_select", tg2.p, G, B, THR, b_idx.p, cap, b_cnt.p, None, P(scratch))
    cslot = np.full((B, G), -1, I)
    for b in range(B):
        n = min(ns[b], stride); cslot[b, cidx[b, :n]] = np.arange(n)
    b_pos = Guarded(prev["pos"], -9)
    vio = Guarded(np.zeros((B, 2), I), -9)
    call("sdfr_candidate_band_map", b_idx.p, cap, b_cnt.p, P(T(cslot)), G, B, stride, b_pos.p, vio.p)
    assert same(b_idx.get(), ref["idx"]) and same(b_cnt.get(), ref["cnt"]) and same(b_pos.get(), ref["pos"]) and not vio.get().any()


def test_candidate_rows_pads_whole_tiles_with_grid_row_0():
    rng = np.random.default_rng(12)
    stride = 256
    ns = [0, 1, 127, 128, 129, stride, stride + 50]
    B, G, NI = len(ns), 700, 6
    inputs = rng.standard_normal((B, G, NI)).astype(F)
    cidx = _candidates(rng, B, G, stride)
    prev = np.full((B, stride, NI), -7, F)
    rows = Guarded(prev, -9.0)
    call("sdfr_candidate_rows", P(T(inputs)), G, NI, B, P(T(cidx)), stride, P(T(np.array(ns, I))), rows.p)
    ref = R.candidate_rows_ref(inputs, cidx, stride, np.array(ns, I), prev)
    assert (ref[2, 127] == inputs[2, 0]).all() and (ref[2, 128] == -7).all() and (ref[4, 255] == inputs[4, 0]).all() and (ref[0] == -7).all()
    assert same(rows.get(), ref)


def test_candidate_band_map_counts_a_non_candidate():
    rng = np.random.default_rng(13)
    B, G, cap, stride = 2, 900, 300, 512
    cidx = _candidates(rng, B, G, stride)
    cslot = np.full((B, G), -1, I)
    for b in range(B):
        cslot[b, cidx[b]] = np.arange(stride)
    idx = np.stack([np.sort(rng.choice(cidx[b], cap, replace=False)) for b in range(B)]).astype(I)
    cnt = np.array([257, 400], I)                                       # (400 > cap: clamped)
    stranger = np.setdiff1d(np.arange(G), cidx[1])[7]
    idx[1, 299] = stranger                                              # one band row that is no candidate ...
    cslot[0, idx[0, 256]] = stride                                      # ... and one whose slot lies beyond the stride
    prev = np.full((B, cap), -7, I)
    for with_vio in (True, False):
        pos = Guarded(prev, -9); vio = Guarded(np.array([[3, 5], [0, 1]], I), -9)
        call("sdfr_candidate_band_map", P(T(idx)), cap, P(T(cnt)), P(T(cslot)), G, B, stride, pos.p, vio.p if with_vio else None)
        rpos, rvio = R.candidate_band_map_ref(idx, cap, cnt, cslot, stride, prev, np.array([[3, 5], [0, 1]], I))
        assert rvio.tolist() == [[3, 6], [0, 2]] and rpos[1, 299] == 0 and rpos[0, 256] == 0 and (rpos[0, 257:] == -7).all()
        assert same(pos.get(), rpos) and same(vio.get(), rvio if with_vio else np.array([[3, 5], [0, 1]], I))


def test_gather_and_scatter_rows():
    """sdfr_gather_rows (ncol 6, negative and too-large slots, cnt > cap), sdfr_scatter_values (cnt > cap), sdfr_gather_rows3,
    sdfr_scatter_add_rows3 and sdfr_sdf_input_grad with its miss counter"""
    rng = np.random.default_rng(14)
    B, G, cap, src_cap, ncol = 3, 1000, 300, 200, 6
    idx = np.stack([np.sort(rng.choice(G, cap, replace=False)) for _ in range(B)]).astype(I)
    cnt = np.array([0, 257, 999], I)
    slot = rng.integers(-3, src_cap + 3, (B, G)).astype(I)
    src = rng.standard_normal((B, src_cap, ncol)).astype(F)
    prev = np.full((B, cap, ncol), -7, F)
    out = Guarded(prev, -9.0)
    call("sdfr_gather_rows", out.p, P(T(src)), ncol, P(T(idx)), P(T(slot)), G, B, cap, src_cap, P(T(cnt)))
    ref = R.gather_rows_ref(src, idx, slot, cap, cnt, prev)
    assert (ref[0] == -7).all() and (ref[1, 257:] == -7).all() and (ref[2] != -7).all() and (ref[2] == 0).all(1).sum() > 3
    assert same(out.get(), ref)
    # scatter_values
    dst = rng.standard_normal((B, G)).astype(F); vals = rng.standard_normal((B, cap)).astype(F); vals[2, 5] = np.nan
    tg = Guarded(dst, 77.0)
    call("sdfr_scatter_values", tg.p, P(T(vals)), P(T(idx)), G, B, cap, P(T(cnt)))
    assert same(tg.get(), R.scatter_values_ref(dst, vals, idx, cap, cnt))
    # rows3: a selection inside one array of cap rows
    sel = np.stack([rng.permutation(cap) for _ in range(B)]).astype(I)
    n3 = np.array([0, 257, 300], I)
    src3 = rng.standard_normal((B, cap, 3)).astype(F)
    o3 = Guarded(np.full((B, cap, 3), -7, F), -9.0)
    call("sdfr_gather_rows3", o3.p, P(T(src3)), P(T(sel)), B, cap, P(T(n3)))
    assert same(o3.get(), R.gather_rows3_ref(src3, sel, n3))
    d3 = rng.standard_normal((B, cap, 3)).astype(F)
    a3 = Guarded(d3, -9.0)
    call("sdfr_scatter_add_rows3", a3.p, P(T(src3)), P(T(sel)), B, cap, P(T(n3)))
    assert same(a3.get(), R.scatter_add_rows3_ref(d3, src3, sel, n3))
    # sdf_input_grad: slots of a real selection (-1 outside), gradients also on rows outside it
    sl = np.full((B, G), -1, I)
    for b in range(B):
        sl[b, idx[b]] = np.arange(cap)
    gs = np.where(rng.random((B, G)) < 0.4, rng.standard_normal((B, G)), 0.0).astype(F)
    J = rng.standard_normal((B, cap, ncol)).astype(F)
    gi = Guarded(np.full((B, G, ncol), -7, F), -9.0)
    miss = torch.full((3,), -5, dtype=torch.int32, device=DEV)
    call("sdfr_sdf_input_grad", P(T(gs)), P(T(sl)), P(T(J)), ncol, G, B, cap, gi.p, miss[1:].data_ptr())
    rgi, rmiss = R.sdf_input_grad_ref(gs, sl, J)
    assert rmiss > 100 and N(miss).tolist() == [-5, rmiss, -5]
    assert same(gi.get(), rgi)
    call("sdfr_sdf_input_grad", P(T(gs)), P(T(sl)), P(T(J)), ncol, G, B, cap, gi.p, None)
    assert same(gi.get(), rgi)


# ---- guard, plan, audit -----------------------------------------------------------------------------------------------------------------------

def _guard_case(rng, ns, G, cap, regimes):
    """crops with ns[b] candidates, small deviations everywhere and the largest one, DEV_MAX, at the candidate the last wave of the last
    stride reads; margin chosen per regime"""
    B = len(ns)
    grid = rng.uniform(-0.05, 0.05, (B, G)).astype(F)
    idx = np.stack([np.sort(rng.choice(G, cap, replace=False)) for _ in range(B)]).astype(I)
    exact = np.zeros((B, cap), F)
    margin = np.zeros(B, F)
    for b in range(B):
        exact[b] = grid[b, idx[b]] + rng.uniform(-1e-4, 1e-4, cap).astype(F)
        n = min(ns[b], cap)
        if n:
            at = n - 1 if n < 1024 else (n - 1) // 1024 * 1024 - 1          # thread 1023 (wave 15) where the crop has 1024 or more
            exact[b, at] = grid[b, idx[b, at]] + F(0.004)
        margin[b] = {"quiet": 0.02, "soft": 0.006, "hard": 0.003, "equal": 0.004}[regimes[b]]
    return grid, idx, exact, margin


@pytest.mark.parametrize("entry", ["sdfr_prefilter_guard", "sdfr_prefilter_guard2"])
def test_prefilter_guard_state_machine(entry):
    """0, 1, 1025 and 2500 candidates, the largest deviation read by the last wave, in each regime (dev <= margin / 2, between, >= margin);
    cnt > cap; an infinite exact value; with guard2 a reused crop is patched and not judged.  Grid values, max_dev, margin and violations bit for bit."""
    rng = np.random.default_rng(21)
    ns = [0, 1, 1025, 2500] * 3 + [2500, 3000]
    regimes = ["quiet"] * 4 + ["soft"] * 4 + ["hard"] * 4 + ["hard", "soft"]
    B, G, cap = len(ns), 5000, 2560
    grid, idx, exact, margin = _guard_case(rng, ns, G, cap, regimes)
    exact[9, 0] = np.inf                                                # an infinite exact value: dev = inf, hard, the margin becomes inf
    cnt = np.array(ns, I)
    reused = None
    if entry.endswith("2"):
        reused = np.zeros(B, I); reused[[2, 12]] = 1
    md0 = np.full(B, -1.0, F); v0 = rng.integers(0, 5, (B, 2)).astype(I)
    rg, rm, rd, rv = R.guard_ref(grid, exact, idx, cap, cnt, margin, md0, v0, reused)
    judged = np.ones(B, bool) if reused is None else reused == 0
    assert ((rv - v0)[4:8][judged[4:8]][1:] == [1, 0]).all() and ((rv - v0)[8:12][1:] == [1, 1]).all() and not (rv - v0)[:5].any()
    assert (rd[1] > 0) and (rm[5:8][judged[5:8]] > margin[5:8][judged[5:8]]).all() and np.isinf(rd[9]) and np.isinf(rm[9])
    tg, tm, td, tv = Guarded(grid, 77.0), Guarded(margin, -9.0), Guarded(md0, -9.0), Guarded(v0, -9)
    args = (tg.p, P(T(exact)), P(T(idx)), G, B, cap, P(T(cnt)), tm.p, td.p, tv.p)
    if reused is not None:
        args += (P(T(reused)),)
    call(entry, *args)
    assert same(tg.get(), rg), "patched grid"
    assert same(td.get(), rd), ("max_dev", td.get(), rd)
    assert same(tm.get(), rm), ("margin", tm.get(), rm)
    assert same(tv.get(), rv), ("violations", tv.get(), rv)


@pytest.mark.parametrize("where", ["first", "last_wave", "second_round"])
def test_prefilter_guard_counts_a_nan_exact_value(where):
    """A candidate whose exact value is NaN: as the kernel documents, the crop counts a soft and a hard violation and its margin does not
    shrink (it stays: no finite deviation to grow it by); the row is patched like every other.
    On the parent commit this failed: the three fmaxf stages (per thread, across the wave, across the waves) each returned their non-NaN
    operand, so max_dev was the finite maximum of the other rows and nothing was counted."""
    rng = np.random.default_rng(22)
    ns = [2500, 2500]
    B, G, cap = 2, 5000, 2560
    grid, idx, exact, margin = _guard_case(rng, ns, G, cap, ["quiet", "quiet"])
    exact[1, {"first": 0, "last_wave": 1023, "second_round": 1500}[where]] = np.nan
    cnt = np.array(ns, I)
    md0 = np.full(B, -1.0, F); v0 = np.zeros((B, 2), I)
    rg, rm, rd, rv = R.guard_ref(grid, exact, idx, cap, cnt, margin, md0, v0)
    assert rv.tolist() == [[0, 0], [1, 1]] and np.isnan(rd[1]) and rm[1] == margin[1]
    tg, tm, td, tv = Guarded(grid, 77.0), Guarded(margin, -9.0), Guarded(md0, -9.0), Guarded(v0, -9)
    call("sdfr_prefilter_guard", tg.p, P(T(exact)), P(T(idx)), G, B, cap, P(T(cnt)), tm.p, td.p, tv.p)
    assert same(tg.get(), rg)
    assert same(tv.get(), rv), ("violations", tv.get().tolist())
    assert same(td.get(), rd) and same(tm.get(), rm)


def _params_forward(yaw, trans, latent, grid, with_inputs=True):
    B, L = latent.shape
    G = grid.shape[0]
    inputs = Guarded(np.full((B, G, L + 3), -7, F), -9.0)
    pose = Guarded(np.full((B, 16), -7, F), -9.0); latnorm = Guarded(np.full(B, -7, F), -9.0)
    call("sdfr_params_forward", P(T(yaw)), P(T(trans)), P(T(latent)), L, P(T(grid)), G, B, inputs.p if with_inputs else None, pose.p, latnorm.p)
    return inputs.get(), pose.get(), latnorm.get()


@pytest.mark.parametrize("L", [3, 9])
def test_plan_kernels_against_the_state_machine(L):
    """sdfr_prefilter_plan on the rows sdfr_params_forward wrote and sdfr_params_plan on the parameters: the same decisions and state as
    plan_ref on every crop, and params_plan's pose / latnorm / inputs are params_forward's bits.  Every state is decisive: both inequalities
    hold or fail by 1e-3 relative or more."""
    rng = np.random.default_rng(30 + L)
    max_reuse, lip, G = 4, 2.5, 257
    m = 0.04
    #        age           latent move (units of margin / 4 / lip)   max_dev (units of margin / 2)
    states = [(0, 0.0, 0.5), (1, 0.0, 0.5), (4, 0.0, 0.5), (5, 0.0, 0.5), (2, 0.5, 0.5), (2, 0.99, 0.99), (2, 1.01, 0.5), (2, 30.0, 0.5),
              (2, 0.5, 1.01), (2, 0.5, 3.0), (3, 0.0, 0.0), (-1, 0.0, 0.5), (4, 0.9, 0.9), (1, 2.0, 2.0)]
    B = len(states)
    yaw = rng.uniform(-3, 3, B).astype(F); trans = rng.standard_normal((B, 3)).astype(F); latent = rng.standard_normal((B, L)).astype(F)
    grid = rng.uniform(-1, 1, (G, 3)).astype(F)
    inputs, pose, latnorm = _params_forward(yaw, trans, latent, grid)
    z = inputs[:, 0, :L].copy()
    margin = np.full(B, m, F)
    age = np.array([s[0] for s in states], I)
    lat_ref = z.copy()
    lat_ref[:, 0] += np.array([s[1] * 0.25 * m / lip for s in states], F)
    max_dev = np.array([s[2] * 0.5 * m for s in states], F)
    nf0 = np.arange(B).astype(I)
    reuse, rl, ra, rn, dec = R.plan_ref(z, lip, margin, max_dev, lat_ref, age, max_reuse, nf0)
    assert (dec >= 1e-3).all(), dec
    assert reuse.tolist() == [0, 1, 1, 0, 1, 1, 0, 0, 0, 0, 1, 0, 1, 0]
    for fused in (False, True):
        tl, ta, tr, tn = Guarded(lat_ref, -9.0), Guarded(age, -9), Guarded(np.full(B, -7, I), -9), Guarded(nf0, -9)
        if fused:
            ti = Guarded(np.full((B, G, L + 3), -7, F), -9.0); tp = Guarded(np.full((B, 16), -7, F), -9.0); tnrm = Guarded(np.full(B, -7, F), -9.0)
            call("sdfr_params_plan", P(T(yaw)), P(T(trans)), P(T(latent)), L, P(T(grid)), G, B, ti.p, tp.p, tnrm.p, lip, P(T(margin)), P(T(max_dev)),
                 tl.p, ta.p, max_reuse, tr.p, tn.p)
            assert same(ti.get(), inputs) and same(tp.get(), pose) and same(tnrm.get(), latnorm)
        else:
            call("sdfr_prefilter_plan", P(T(inputs)), G, L + 3, L, B, lip, P(T(margin)), P(T(max_dev)), tl.p, ta.p, max_reuse, tr.p, tn.p)
        assert same(tr.get(), reuse) and same(ta.get(), ra) and same(tn.get(), rn) and same(tl.get(), rl), fused
    # n_full == NULL
    tl, ta, tr = Guarded(lat_ref, -9.0), Guarded(age, -9), Guarded(np.full(B, -7, I), -9)
    call("sdfr_prefilter_plan", P(T(inputs)), G, L + 3, L, B, lip, P(T(margin)), P(T(max_dev)), tl.p, ta.p, max_reuse, tr.p, None)
    assert same(tr.get(), reuse) and same(ta.get(), ra) and same(tl.get(), rl)


@pytest.mark.parametrize("stride", [1, 7, 16])
@pytest.mark.parametrize("G", [100, 4097])
def test_audit_select_and_check_over_a_full_rotation(G, stride):
    """`stride` consecutive phases: every non-candidate row is selected exactly once and no candidate; n_audit, the copied input rows and the
    phase counter per step; one planted band row and one NaN among the exact values count one hard violation each for their crop; audit_dev is
    the largest |grid - exact| of the crop that is not reused; a cap_rows below the slice writes nothing beyond it"""
    rng = np.random.default_rng(G + stride)
    B, NI = 2, 4
    cslot = np.where(rng.random((B, G)) < 0.3, 5, -1).astype(I)
    inputs = rng.standard_normal((B, G, NI)).astype(F)
    sdf_grid = rng.uniform(0.1, 0.3, (B, G)).astype(F)
    exact_of = (sdf_grid + rng.uniform(-0.01, 0.01, (B, G)).astype(F)).reshape(-1)
    free = [np.nonzero(cslot[b] < 0)[0] for b in range(B)]
    exact_of[0 * G + free[0][len(free[0]) // 2]] = np.nan
    exact_of[1 * G + free[1][-1]] = 0.02
    reused = np.array([0, 1], I)
    cap_rows = B * G
    phase0 = 5
    phase = torch.full((3,), -5, dtype=torch.int32, device=DEV); phase[1] = phase0
    dev = np.zeros(B, F); vio = np.zeros((B, 2), I)
    t_dev, t_vio = Guarded(dev, -9.0), Guarded(vio, -9)
    t_in, t_cs, t_grid, t_re = T(inputs), T(cslot), T(sdf_grid), T(reused)
    seen = []
    for step in range(stride):
        rows = torch.full((cap_rows + 1, NI), -7.0, device=DEV); src = torch.full((cap_rows + 1,), -7, dtype=torch.int32, device=DEV)
        n_audit = torch.full((3,), -5, dtype=torch.int32, device=DEV)
        call("sdfr_prefilter_audit_select", P(t_in), P(t_cs), G, NI, B, stride, phase[1:].data_ptr(), P(rows), P(src), n_audit[1:].data_ptr(), cap_rows)
        want, n = R.audit_select_ref(cslot, stride, phase0 + step)
        assert N(n_audit).tolist() == [-5, n, -5]
        s = N(src)
        order = np.argsort(s[:n])
        assert np.array_equal(s[:n][order], want) and (s[n:] == -7).all()
        assert same(N(rows)[:n], inputs.reshape(-1, NI)[s[:n]]) and (N(rows)[n:] == -7).all()
        seen.append(want)
        ex = np.zeros(cap_rows, F); ex[:n] = exact_of[s[:n]]
        call("sdfr_prefilter_audit_check", P(t_grid), P(T(ex)), P(src), n_audit[1:].data_ptr(), cap_rows, G, B, THR, P(t_re), t_dev.p, t_vio.p,
             phase[1:].data_ptr())
        dev, vio, ph = R.audit_check_ref(sdf_grid, ex, s, n, cap_rows, G, THR, reused, dev, vio, phase0 + step)
        assert N(phase).tolist() == [-5, ph, -5]
        assert same(t_dev.get(), dev) and same(t_vio.get(), vio), (step, t_vio.get().tolist(), vio.tolist())
    seen = np.concatenate(seen)
    assert np.array_equal(np.sort(seen), np.nonzero(cslot.reshape(-1) < 0)[0]), "not every non-candidate row exactly once"
    assert vio.tolist() == [[0, 1], [0, 1]] and dev[0] > 0 and dev[1] == 0
    # a workspace smaller than the slice: the count is the full one, nothing beyond cap_rows is written, the check reads cap_rows rows
    small = 5
    rows = torch.full((small + 1, NI), -7.0, device=DEV); src = torch.full((small + 1,), -7, dtype=torch.int32, device=DEV)
    n_audit = torch.zeros((1,), dtype=torch.int32, device=DEV)
    call("sdfr_prefilter_audit_select", P(t_in), P(t_cs), G, NI, B, stride, phase[1:].data_ptr(), P(rows), P(src), P(n_audit), small)
    want, n = R.audit_select_ref(cslot, stride, phase0 + stride)
    s = N(src)
    assert int(n_audit) == n and n > small and s[small] == -7 and (N(rows)[small] == -7).all()
    assert np.isin(s[:small], want).all() and np.unique(s[:small]).size == small
    assert same(N(rows)[:small], inputs.reshape(-1, NI)[s[:small]])
    ex = np.full(small, 0.5, F); ex[2] = 0.0
    v2 = Guarded(np.zeros((B, 2), I), -9); d2 = Guarded(np.zeros(B, F), -9.0)
    call("sdfr_prefilter_audit_check", P(t_grid), P(T(ex)), P(src), P(n_audit), small, G, B, THR, None, d2.p, v2.p, phase[1:].data_ptr())
    rd, rv, _ = R.audit_check_ref(sdf_grid, ex, s, n, small, G, THR, None, np.zeros(B, F), np.zeros((B, 2), I), 0)
    assert rv.sum() == 1 and same(v2.get(), rv) and same(d2.get(), rd)


# ---- parameters -------------------------------------------------------------------------------------------------------------------------------

# cosf / sinf of the device library against float64 cos / sin of the float32 yaw, in eps32 (mass 1): measured once over the sweep below
# (profiles/surface_tests_notes.md), twice that allowed because the sweep is finite, and never more than 4 eps32
TRIG_MEASURED = 0.5441
TRIG_BOUND = min(2 * TRIG_MEASURED, 4.0)


def _yaw_sweep(n):
    y = np.linspace(-2 * np.pi, 2 * np.pi, n).astype(F)
    y[:7] = np.array([0.0, -0.0, np.pi / 2, -np.pi / 2, np.pi, -np.pi, 2 * np.pi], F)
    return y


def _check_pose_bits(pose, trans):
    u = pose.view(np.uint32)
    bits = lambda v: np.array(v, F).view(np.uint32)
    for k, v in ((1, 0.0), (4, -0.0), (5, -1.0), (6, -0.0), (9, 0.0), (12, 0.0), (13, 0.0), (14, 0.0), (15, 1.0)):
        assert (u[:, k] == bits(v)).all(), "P[%d]" % k
    assert same(pose[:, 0], pose[:, 10]) and same(pose[:, 2], -pose[:, 8])
    assert same(pose[:, [3, 7, 11]], trans)


def test_params_forward_yaw_sweep():
    """4001 yaws over [-2 pi, 2 pi] with 0, -0, +-pi/2, +-pi, 2 pi in one launch: the constant entries of the pose by their bits (signed zeros
    included), P[0] == P[10], P[2] == -P[8], the translation column, and cos / sin against float64"""
    B = 4001
    rng = np.random.default_rng(40)
    yaw = _yaw_sweep(B); trans = rng.standard_normal((B, 3)).astype(F); latent = rng.standard_normal((B, 1)).astype(F)
    _, pose, latnorm = _params_forward(yaw, trans, latent, np.zeros((1, 3), F), with_inputs=False)
    _check_pose_bits(pose, trans)
    judge("params_forward latnorm sweep", latnorm, np.abs(latent[:, 0].astype(np.float64)), np.abs(latent[:, 0]), 0.75)     # (as below, L = 1)
    ec = np.abs(pose[:, 0].astype(np.float64) - np.cos(yaw.astype(np.float64))).max() / EPS32
    es = np.abs(pose[:, 2].astype(np.float64) - np.sin(yaw.astype(np.float64))).max() / EPS32
    print("SURFTEST trig sweep: cosf %.4g eps32, sinf %.4g eps32 (allowed %.3g)" % (ec, es, TRIG_BOUND))
    assert pose[0, 0] == 1 and pose[0, 2] == 0 and pose[1, 0] == 1
    assert max(ec, es) <= TRIG_BOUND


@pytest.mark.parametrize("L", [1, 3, 8, 9, 256])
def test_params_forward_rows_norm_and_pose(L):
    """G in {1, 256, 257} x B in {1, 3}: latnorm and the normalised latent columns against float64, the grid columns and the pose's exact
    entries by their bits, a zero latent (latnorm 1e-12f, zero rows), and inputs == NULL (64 threads: pose and norm the same bits, the input
    array untouched)"""
    rng = np.random.default_rng(41 + L)
    for G in (1, 256, 257):
        for B in (1, 3):
            yaw = rng.uniform(-2 * np.pi, 2 * np.pi, B).astype(F); trans = rng.standard_normal((B, 3)).astype(F)
            latent = rng.standard_normal((B, L)).astype(F)
            if B == 3:
                latent[1] = 0.0
            grid = rng.uniform(-1, 1, (G, 3)).astype(F)
            inputs, pose, latnorm = _params_forward(yaw, trans, latent, grid)
            rn, rrows, rpose = R.params_forward_ref(yaw, trans, latent)
            _check_pose_bits(pose, trans)
            judge("params_forward cos/sin", pose[:, [0, 2]], rpose[:, 0, [0, 2]], np.ones((B, 2)), TRIG_BOUND)
            # the sum of L squares: one rounding per product and per addition, relative to a partial sum below the total -> L roundings of the
            # sum, halved by the root, plus the root's own: (L / 2 + 1) roundings = (L / 4 + 1 / 2) eps32; the quotient adds one more
            judge("params_forward latnorm L %d" % L, latnorm, rn, rn, 0.25 * L + 0.5)
            assert same(inputs[:, :, L:], np.broadcast_to(grid[None], (B, G, 3)))
            assert same(inputs[:, :, :L], np.broadcast_to(inputs[:, :1, :L], (B, G, L))), "the latent columns differ between rows"
            judge("params_forward rows L %d" % L, inputs[:, 0, :L], rrows, np.abs(rrows), 0.25 * L + 1.0)
            if B == 3:
                assert latnorm[1] == F(1e-12) and not inputs[1, :, :L].any()
            i2, p2, n2 = _params_forward(yaw, trans, latent, grid, with_inputs=False)
            assert same(p2, pose) and same(n2, latnorm) and (i2 == -7).all()


@pytest.mark.parametrize("L", [1, 3, 8, 9, 256])
def test_params_backward_against_float64(L):
    """B in {1, 64, 65} (the second 64-thread block): g_yaw, g_trans and g_latent against params_backward_ref on the kernel's own cos, sin and
    latnorm; one crop with a zero latent"""
    rng = np.random.default_rng(50 + L)
    for B in (1, 64, 65):
        yaw = rng.uniform(-2 * np.pi, 2 * np.pi, B).astype(F); trans = rng.standard_normal((B, 3)).astype(F)
        latent = rng.standard_normal((B, L)).astype(F)
        if B > 1:
            latent[B - 1] = 0.0
        _, pose, latnorm = _params_forward(yaw, trans, latent, np.zeros((1, 3), F), with_inputs=False)
        g_pose = rng.standard_normal((B, 16)).astype(F); g_latn = rng.standard_normal((B, L)).astype(F)
        if B > 1:
            g_latn[B - 1] *= F(1e-14)                                   # (finite over latnorm = 1e-12)
        gy, gt, gl = Guarded(np.full(B, -7, F), -9.0), Guarded(np.full((B, 3), -7, F), -9.0), Guarded(np.full((B, L), -7, F), -9.0)
        call("sdfr_params_backward", P(T(yaw)), P(T(latent)), L, P(T(latnorm)), P(T(g_pose)), P(T(g_latn)), B, gy.p, gt.p, gl.p)
        ry, rt, rl, m = R.params_backward_ref(pose[:, 0], pose[:, 2], latent, latnorm, g_pose, g_latn)
        judge("params_backward g_yaw", gy.get(), ry, m["g_yaw"], 3.5)              # four products, three additions
        assert same(gt.get(), g_pose[:, [3, 7, 11]])
        # z = latent / latnorm (1), z g (1), the dot's L - 1 additions, z * dot (1), the difference (1), the quotient (1): L + 4, and z once more
        judge("params_backward g_latent L %d B %d" % (L, B), gl.get(), rl, m["g_latent"], 0.5 * (L + 5))


def _latent_contract(gs, ms, Jl):
    Jl = np.asarray(Jl, F).astype(np.float64)
    return (gs[:, None] * Jl).sum(0), (ms[:, None] * np.abs(Jl)).sum(0)


@pytest.mark.parametrize("nocs", [False, True])
@pytest.mark.parametrize("L", [3, 8, 9, 17])
def test_surface_latent_grad_against_float64(L, nocs):
    """count in {0, 1, 1024, 1025, 3000}: up to three strides of the 1024 threads, and with L 9 and 17 a second and third chunk of 8 columns"""
    for counts in ((0, 3000), (1, 1025), (1024, 2)):
        _latent_grad_case(np.random.default_rng(60 + L + counts[0]), counts, L, nocs)


def _latent_grad_case(rng, counts, L, nocs):
    B, cap, NI = len(counts), 3000, L + 3
    g_pts = rng.standard_normal((B, cap, 3)).astype(F); g_nocs = rng.standard_normal((B, cap, 3)).astype(F) if nocs else None
    nh = rng.standard_normal((B, cap, 3)); nh = (nh / np.linalg.norm(nh, axis=2, keepdims=True)).astype(F)
    J = rng.standard_normal((B, cap, NI)).astype(F)
    out = Guarded(np.full((B, L), -7, F), -9.0)
    call("sdfr_surface_latent_grad", P(T(g_pts)), P(T(g_nocs)) if nocs else None, P(T(nh)), P(T(J)), NI, L, B, cap, P(T(np.array(counts, I))), out.p)
    got = out.get()
    for b, c in enumerate(counts):
        gs, _, ms = SR.surface_project_bwd_ref(nh[b, :c], g_pts[b, :c], None if g_nocs is None else g_nocs[b, :c])
        gl, ml = _latent_contract(gs, ms, J[b, :c, :L])
        # g_sdf: the sum with g_nocs / 2 (1), three products and two additions (5); its product with J (1); then per thread ceil(c / 1024)
        # additions, 6 across the wave, 16 across the waves
        judge("latent_grad L %d count %d" % (L, c), got[b], gl, ml, 0.5 * (7 + math.ceil(c / 1024) + 6 + 16))
        if c == 0:
            assert not got[b].any()


TAIL_PAIRS = [(0, 6200), (1, 3073), (1023, 3072), (1024, 3071)]
TAIL_CONFIGS = [  # xyzf, J, L, output_nocs, absent
    (True, True, 3, 1, None), (True, True, 8, 6, "pc"), (True, True, 1, 2, "nc"), (True, True, 3, 5, "col"),
    (False, True, 8, 1, None), (False, True, 1, 5, "pc"), (False, True, 3, 2, "col"),
    (True, False, 3, 2, None), (True, False, 8, 5, "nc"),
    (False, False, 8, 6, None), (False, False, 1, 1, "nc")]


def _tail_inputs(rng, B, cap, counts, L, NI, xyzf):
    f = lambda *s: rng.standard_normal(s).astype(F)
    d = dict(points=rng.uniform(-1, 1, (B, cap, 3)).astype(F), g_pc=f(B, cap, 3), g_nc=f(B, cap, 3), g_col=f(B, cap, 3), J=f(B, cap, NI))
    nh = rng.standard_normal((B, cap, 3)); d["normals"] = (nh / np.linalg.norm(nh, axis=2, keepdims=True)).astype(F)
    d["yaw"] = rng.uniform(-3, 3, B).astype(F); d["trans"] = f(B, 3); d["latent"] = f(B, L)
    fslot = np.full((B, cap), -1, I)
    for b, c in enumerate(counts):                                     # about half the rows front-facing (back-facing rows: slot -1)
        front = np.nonzero(rng.random(c) < 0.5)[0]
        fslot[b, front] = np.arange(front.size)
    d["fslot"] = fslot
    d["g_xyzf"] = f(B, cap, 3)
    _, d["pose"], d["latnorm"] = _params_forward(d["yaw"], d["trans"], d["latent"], np.zeros((1, 3), F), with_inputs=False)
    return d


def _tail_bounds(c, L, xyzf):
    n = math.ceil(c / 1024)
    c_pts = 3.5                     # a = g_pc + g_xyzf (1), three products and two additions (5), the colour's term (1): 7 roundings
    c_pose = 0.5 * (n + 6 + 16 + 4)  # a (1), two products and their sum (3), then n additions per thread, 6 across the wave, 16 across the waves
    c_latn = c_pts + 2.5 + 0.5 + 0.5 * (n + 6 + 16)     # g_points, its contraction with the normal (5), the product with J (1), the sums
    return dict(g_points=c_pts, g_pose=c_pose, g_latn=c_latn, g_yaw=c_pose + 3.5, g_trans=c_pose, g_latent=c_latn + 0.5 * (L + 5))


def _tail_check(tag, d, b, c, L, mode, absent, xyzf, lat, got, gx_rows):
    """crop b of a launch against tail_ref; got: g_points (or None), g_pose, g_latn, g_yaw, g_trans, g_latent as numpy"""
    pick = lambda k: None if absent == k else d["g_" + k][b, :c]
    r = R.tail_ref(d["pose"][b], d["points"][b, :c], d["normals"][b, :c], pick("pc"), pick("nc"), pick("col"), mode,
                   gx_rows if xyzf else None, d["fslot"][b, :c] if xyzf else None, d["J"][b, :c, :L] if lat else None, d["latent"][b], d["latnorm"][b])
    bd = _tail_bounds(c, L, xyzf)
    worst = {}
    if got["g_points"] is not None:
        worst["g_points"] = judge(tag + " g_points", got["g_points"][b, :c], r["g_points"], r["mass_g_points"], bd["g_points"])
        assert (got["g_points"][b, c:] == -7).all()
    gp = got["g_pose"][b].reshape(4, 4)
    worst["g_pose"] = judge(tag + " g_pose", gp[:3], r["g_pose"], r["mass_g_pose"], bd["g_pose"])
    assert not gp[3].any()
    worst["g_yaw"] = judge(tag + " g_yaw", got["g_yaw"][b], r["g_yaw"], r["mass_g_yaw"], bd["g_yaw"])
    worst["g_trans"] = judge(tag + " g_trans", got["g_trans"][b], r["g_trans"], r["mass_g_trans"], bd["g_trans"])
    if lat:
        worst["g_latn"] = judge(tag + " g_latn", got["g_latn"][b], r["g_latn"], r["mass_g_latn"], bd["g_latn"])
        worst["g_latent"] = judge(tag + " g_latent", got["g_latent"][b], r["g_latent"], r["mass_g_latent"], bd["g_latent"])
    else:
        assert not got["g_latn"][b].any() and not got["g_latent"][b].any()
    return r


@pytest.mark.parametrize("cfg", TAIL_CONFIGS, ids=lambda c: "xyzf%d-J%d-L%d-mode%d-no_%s" % c)
def test_pose_latent_backward_against_the_composed_reference(cfg):
    """sdfr_pose_latent_backward, two crops per launch with different counts, count in {0, 1, 1023, 1024, 3071, 3072, 3073, 6200} of cap 6400
    (3072 surfels per trip of the unrolled loop: 3073 and 6200 take the second and third): every g_points row, the 12 pose sums, the zero
    fourth row, g_latn, g_yaw, g_trans, g_latent"""
    xyzf, lat, L, mode, absent = cfg
    rng = np.random.default_rng(70 + L + mode)
    B, cap, NI = 2, 6400, L + 2
    for counts in TAIL_PAIRS:
        d = _tail_inputs(rng, B, cap, counts, L, NI, xyzf)
        t = {k: T(v) for k, v in d.items()}
        opt = lambda k: None if absent == k else P(t["g_" + k])
        o = dict(g_points=Guarded(np.full((B, cap, 3), -7, F), -9.0), g_pose=Guarded(np.full((B, 16), -7, F), -9.0),
                 g_latn=Guarded(np.full((B, L), -7, F), -9.0), g_yaw=Guarded(np.full(B, -7, F), -9.0), g_trans=Guarded(np.full((B, 3), -7, F), -9.0),
                 g_latent=Guarded(np.full((B, L), -7, F), -9.0))
        call("sdfr_pose_latent_backward", P(t["pose"]), P(t["points"]), P(t["normals"]), opt("pc"), opt("nc"), opt("col"), B, cap,
             P(T(np.array(counts, I))), mode, P(t["g_xyzf"]) if xyzf else None, P(t["fslot"]) if xyzf else None, P(t["J"]) if lat else None, NI, L,
             P(t["yaw"]), P(t["latent"]), P(t["latnorm"]), o["g_points"].p, o["g_pose"].p, o["g_latn"].p, o["g_yaw"].p, o["g_trans"].p, o["g_latent"].p)
        got = {k: v.get() for k, v in o.items()}
        for b, c in enumerate(counts):
            _tail_check("tail %s count %d" % (cfg, c), d, b, c, L, mode, absent, xyzf, lat, got, d["g_xyzf"][b])


@pytest.mark.parametrize("lat", [True, False])
def test_pose_latent_solver_against_the_references_and_the_separate_launches(lat):
    """sdfr_pose_latent_solver on three crops (2000, 5000 and 3500 surfels: below and above one 3072-surfel trip; the third is skipped by
    npairs = -1): gradients against the composed reference with the factor kscale[2 b + 1] on the g_xyzf rows, parameters / Adam state /
    total / stepped against solver_ref fed with the reference gradients, and everything bit-equal to sdfr_pose_latent_backward on the
    products + sdfr_solver_step"""
    rng = np.random.default_rng(90)
    B, cap, L, mode = 3, 6400, 3, 5
    NI = L + 2
    counts = (2000, 5000, 3500)
    d = _tail_inputs(rng, B, cap, counts, L, NI, True)
    kscale = rng.uniform(0.2, 2.0, (B, 2)).astype(F)
    lrA, lrS, lrL = 0.01, 0.01, 3e-5
    w2, w3 = 0.7, 1.3
    loss2d = rng.uniform(0.1, 1.0, B).astype(F); loss3d = rng.uniform(0.1, 1.0, B).astype(F)
    npairs = np.array([40, 7, -1], I)
    params = np.concatenate([d["yaw"], d["trans"].reshape(-1), np.full(B, 2.0, F), d["latent"].reshape(-1)]).astype(F)
    grads0 = np.full(params.size, -7, F); g_scale = rng.standard_normal(B).astype(F); grads0[4 * B:5 * B] = g_scale
    t = {k: T(v) for k, v in d.items()}
    tcnt, tks = T(np.array(counts, I)), T(kscale)

    def state():
        return dict(params=Guarded(params[None], -9.0), grads=Guarded(grads0[None], -9.0), m=Guarded(np.zeros((B, 4), F), -9.0), v=Guarded(np.zeros((B, 4), F), -9.0),
                    t=Guarded(np.zeros(B, I), -9), total=Guarded(np.full(B, -7, F), -9.0), stepped=Guarded(np.full(B, -7, I), -9),
                    g_pose=Guarded(np.full((B, 16), -7, F), -9.0), g_latn=Guarded(np.full((B, L), -7, F), -9.0))

    a = state()
    call("sdfr_pose_latent_solver", P(t["pose"]), P(t["points"]), P(t["normals"]), P(t["g_pc"]), P(t["g_nc"]), P(t["g_col"]), B, cap, P(tcnt), mode,
         P(t["g_xyzf"]), P(t["fslot"]), P(tks), P(t["J"]) if lat else None, NI, L, P(t["yaw"]), P(t["latent"]), P(t["latnorm"]), a["g_pose"].p, a["g_latn"].p,
         a["params"].p, a["grads"].p, P(T(loss2d)), P(T(loss3d)), P(T(npairs)), w2, w3, a["m"].p, a["v"].p, a["t"].p, lrA, lrS, lrL, a["total"].p,
         a["stepped"].p)
    A = {k: v.get() for k, v in a.items()}
    # the launches it replaces: the float32 products first (one rounding, as the kernel forms them on load)
    gx_scaled = (t["g_xyzf"] * tks[:, 1].view(B, 1, 1)).contiguous()
    s = state()
    gbase = s["grads"].t.view(-1)
    call("sdfr_pose_latent_backward", P(t["pose"]), P(t["points"]), P(t["normals"]), P(t["g_pc"]), P(t["g_nc"]), P(t["g_col"]), B, cap, P(tcnt), mode,
         P(gx_scaled), P(t["fslot"]), P(t["J"]) if lat else None, NI, L, P(t["yaw"]), P(t["latent"]), P(t["latnorm"]), None, s["g_pose"].p, s["g_latn"].p,
         gbase.data_ptr(), gbase[B:].data_ptr(), gbase[5 * B:].data_ptr())
    call("sdfr_solver_step", s["params"].p, s["grads"].p, L, P(T(loss2d)), P(T(loss3d)), P(T(npairs)), w2, w3, s["m"].p, s["v"].p, s["t"].p, lrA, lrS, lrL, B,
         s["total"].p, s["stepped"].p)
    S = {k: v.get() for k, v in s.items()}
    for k in A:
        assert same(A[k], S[k]), k
    # against the references
    g = A["grads"][0]
    got = dict(g_points=None, g_pose=A["g_pose"], g_latn=A["g_latn"], g_yaw=g[:B], g_trans=g[B:4 * B].reshape(B, 3), g_latent=g[5 * B:].reshape(B, L))
    assert same(g[4 * B:5 * B], g_scale)
    gref = np.zeros(params.size); dg = np.zeros(params.size)            # the reference gradients and the bound on the kernel's distance from them
    gref[4 * B:5 * B] = g_scale
    gxs = N(gx_scaled)
    for b, c in enumerate(counts):
        r = _tail_check("solver tail J%d count %d" % (lat, c), d, b, c, L, mode, None, True, lat, got, gxs[b])
        bd = _tail_bounds(c, L, True)
        gref[b] = r["g_yaw"]; dg[b] = bd["g_yaw"] * EPS32 * r["mass_g_yaw"]
        gref[B + 3 * b:B + 3 * b + 3] = r["g_trans"]; dg[B + 3 * b:B + 3 * b + 3] = bd["g_trans"] * EPS32 * r["mass_g_trans"]
        gref[5 * B + b * L:5 * B + (b + 1) * L] = r["g_latent"]; dg[5 * B + b * L:5 * B + (b + 1) * L] = bd["g_latent"] * EPS32 * r["mass_g_latent"]
    f32 = lambda x: float(F(x))
    pr = params.astype(np.float64); mr, vr, tr = np.zeros((B, 4)), np.zeros((B, 4)), np.zeros(B, np.int64)
    tot, stepped = LR.solver_ref(pr, gref, L, loss2d, loss3d, npairs, w2, w3, mr, vr, tr, f32(lrA), f32(lrS), f32(lrL))
    assert stepped.tolist() == [1, 1, 0] and same(A["stepped"], stepped) and same(A["total"], tot.astype(F)) and same(A["t"], tr.astype(I))
    p = A["params"][0]
    crop = np.concatenate([np.arange(B), np.repeat(np.arange(B), 3), np.arange(B), np.repeat(np.arange(B), L)])
    assert same(p[crop == 2], params[crop == 2]) and not A["m"][2].any() and not A["v"][2].any()
    # the bounds of tests/test_gpu_losses.py for one step (Adam: lr * 1e-5 + 8 ulp; SGD: 2 ulp; m, v: 1e-5 relative), widened by what the
    # gradient's own bound dg moves the step: the first Adam step is lr g / (|g| + 1e-8), whose derivative is at most lr / (|g| + 1e-8);
    # SGD moves by lr dg; m = 0.1 g by 0.1 dg; v = 0.001 g^2 by 0.001 (2 |g| + dg) dg
    ulp = np.spacing(np.maximum(np.abs(pr), np.abs(p)).astype(F)).astype(np.float64)
    lr = np.where(np.arange(params.size) < 5 * B, lrS, lrL)
    tol = np.where(np.arange(params.size) < 4 * B, lrA * 1e-5 + 8 * ulp + lrA * dg / (np.abs(gref) + 1e-8), 2 * ulp + lr * dg)
    err = np.abs(p - pr)
    print("SURFTEST solver J%d: parameter error / bound %.3g" % (lat, float((err / tol).max())))
    assert (err <= tol).all(), (err / tol).max()
    g4 = np.stack([np.concatenate([gref[b:b + 1], gref[B + 3 * b:B + 3 * b + 3]]) for b in range(B)])
    d4 = np.stack([np.concatenate([dg[b:b + 1], dg[B + 3 * b:B + 3 * b + 3]]) for b in range(B)])
    assert (np.abs(A["m"] - mr) <= 1e-5 * np.abs(mr) + 1e-30 + 0.1 * d4).all()
    assert (np.abs(A["v"] - vr) <= 1e-5 * np.abs(vr) + 1e-30 + 0.001 * (2 * np.abs(g4) + d4) * d4).all()
