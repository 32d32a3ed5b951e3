"""The sphere tracer's kernels (csrc/trace.hip) one entry point at a time against the float64 restatement of tests/_trace_ref.py, through the
C ABI: set-up (dense, ragged, cone starts), the step rule, one speculative pass of the looping kernel, whole marches on a hand-built slab
decoder, the cone phase, hit list, polish and images, pixel-order points, and the backward in both derivative semantics.

Every output array is sentinel-filled with a guard in front of and behind it and compared as a whole.  Integers, copied values and floats the
reference proves exact are compared BIT FOR BIT; every other float against the error bound the reference carries for it (tests/_trace_ref.py:
u per rounding on the value's path, handed on to first order); decisions on the rays whose comparison is further from its threshold than
that bound (`decided`; tests/test_trace_refs_cpu.py caps the others at 2 % per case).  Lists filled by ballot appends are compared as sets
keyed by pixel, their slots a bijection onto [0, count).  Figures of one run: profiles/trace_tests_notes.md (`pytest -s`, lines TRACETEST)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from sdflabel_amd import _lib
from tests import _trace_cases as C
from tests import _trace_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
F = np.float32
I = np.int32
SENT_F = F(-777.25)
SENT_I = I(-77)
PAD = 64

_alive = []


def T(a):
    t = torch.as_tensor(np.ascontiguousarray(a), device=DEV)
    _alive.append(t)
    return t


def Z(z):
    """the latent rows on the device (L = 0: a word to point at -- the entry points refuse NULL)"""
    return _lib.ptr(T(z if z.size else np.zeros(1, F)))


def call(name, *args):
    rc = getattr(_lib.lib(), name)(*args, _lib.stream_ptr())
    torch.cuda.synchronize()
    _lib.check(rc, name)


def same(a, b):
    """equal bits (a NaN equals a NaN; -0 differs from +0)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    nan = np.isnan(a)
    return bool(np.array_equal(nan, np.isnan(b)) and np.array_equal(a.view(np.uint32)[~nan], b.view(np.uint32)[~nan]))


class Out:
    """a device array between two guards of PAD sentinels; starts as `init` or all sentinel; get() checks the guards"""

    def __init__(self, shape, dtype, init=None):
        self.shape = (shape,) if isinstance(shape, int) else tuple(shape)
        self.sent = SENT_F if dtype == F else SENT_I
        n = int(np.prod(self.shape))
        full = np.full(n + 2 * PAD, self.sent, dtype)
        if init is not None:
            full[PAD:PAD + n] = np.asarray(init, dtype).reshape(-1)
        self.n = n
        self.full = torch.as_tensor(full, device=DEV)

    @property
    def p(self):
        return self.full.data_ptr() + PAD * 4

    def get(self):
        f = self.full.cpu().numpy()
        assert (f[:PAD] == self.sent).all() and (f[PAD + self.n:] == self.sent).all(), "a guard was written"
        return f[PAD:PAD + self.n].reshape(self.shape)


def take(rays, k):
    return dict(o=[c[k] for c in rays["o"]], d=[c[k] for c in rays["d"]], r=[c[k] for c in rays["r"]], dn=rays["dn"][k])


def worst_unit(what, got, ref, sel=None):
    """largest |got - ref| in units of the reference's own bound over the selected elements; asserts <= 1"""
    u = R.unit(got, ref)
    if sel is not None:
        u = u[sel]
    w = float(np.nanmax(u)) if u.size else 0.0
    assert not np.isnan(u).any() and w <= 1.0, "%s: %.3g bounds from the reference at element %s" % (what, w, np.argmax(u))
    return w


def valid(W, H, PS):
    return W > 0 and H > 0 and W * H <= PS


def extents(sizes, PS, cone_cap=1):
    wh = T(np.asarray(sizes, I).reshape(-1, 2))
    ext = _lib.Extents(wh.data_ptr(), PS, cone_cap)
    _alive.append(ext)
    return ctypes.addressof(ext)


# ---- sdfr_trace_setup2 / _r -------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _setup_ref(name, W, H, block, seed):
    Pm, Ki = C.POSES[name]
    cone = C.cone_starts(W, H, block, C.BOUND, C.NEAR, Pm, Ki, seed) if block else None
    return R.setup_crop(Pm, Ki, W, H, C.BOUND, C.NEAR, cone, block), cone


def _setup_case(tag, names, sizes, PS, L, block, ragged):
    B = len(names)
    Pm, Ki = C.batch(names)
    z = C.latn(B, L)
    n = B * PS
    refs = [(_setup_ref(nm, W, H, block, b) if valid(W, H, PS) else (None, None)) for b, (nm, (W, H)) in enumerate(zip(names, sizes))]
    ncap = 1
    cone_t = None
    if block:
        ncap = max(((W + block - 1) // block) * ((H + block - 1) // block) for W, H in sizes if valid(W, H, PS)) + (3 if ragged else 0)
        cone = np.full((B, ncap), 9.0, F)
        for b, (_, cn) in enumerate(refs):
            if cn is not None:
                cone[b, :cn.size] = cn
        cone_t = T(cone)
    o = dict(counters=Out(32, I), pix=Out(n, I), lam=Out((n, 4), F), far=Out(n, F), inputs=Out((n, L + 3), F), hl=Out(n, F), hs=Out(n, F))
    tail = (C.BOUND, C.NEAR, o["counters"].p, o["pix"].p, o["lam"].p, o["far"].p, o["inputs"].p, _lib.ptr(cone_t), block, o["hl"].p, o["hs"].p)
    if ragged:
        call("sdfr_trace_setup_r", _lib.ptr(T(Pm)), _lib.ptr(T(Ki)), Z(z), L, B, extents(sizes, PS, ncap), *tail)
    else:
        call("sdfr_trace_setup2", _lib.ptr(T(Pm)), _lib.ptr(T(Ki)), Z(z), L, B, sizes[0][0], sizes[0][1], *tail)
    g = {k: v.get() for k, v in o.items()}
    del _alive[:]
    cnt = g["counters"]
    nl = int(cnt[0])
    assert 0 <= nl <= n and not cnt[1:].any(), "%s: counters %s" % (tag, cnt[:8])
    assert same(g["hl"], np.zeros(n, F)) and same(g["hs"], np.zeros(n, F)), tag + ": hit records not zeroed over the whole slot"
    pix = g["pix"][:nl].astype(np.int64)
    assert np.unique(pix).size == nl, tag + ": a pixel is listed twice"
    assert (g["pix"][nl:] == SENT_I).all() and (g["lam"][nl:] == SENT_F).all() and (g["inputs"][nl:] == SENT_F).all(), tag + ": rows beyond the count"
    assert ((pix >= 0) & (pix < n)).all()
    worst = dict(far=0.0, l0=0.0, x=0.0)
    und = tot = 0
    for b, (W, H) in enumerate(sizes):
        far_b = g["far"][b * PS:(b + 1) * PS]
        mine = np.nonzero(pix // PS == b)[0]
        if not valid(W, H, PS):
            assert same(far_b, np.zeros(PS, F)) and mine.size == 0, tag + ": a crop outside the contract lists or writes something"
            continue
        ref = refs[b][0]
        npx = W * H
        assert same(far_b[npx:], np.zeros(PS - npx, F)), tag + ": far on the slack pixels"
        loc = pix[mine] - b * PS
        assert (loc < npx).all(), tag + ": a slack pixel is listed"
        listed = np.zeros(npx, bool)
        listed[loc] = True
        dec = ref["ratio"] > 1
        und += int((~dec).sum()); tot += npx
        bad = np.nonzero((listed != ref["active"]) & dec)[0]
        assert bad.size == 0, "%s crop %d: the active set differs on decided pixels %s" % (tag, b, bad[:6])
        assert (far_b[:npx][~listed] == 0).all(), tag + ": far of an inactive ray"
        worst["far"] = max(worst["far"], worst_unit(tag + " far", far_b[:npx], ref["l1"], listed))
        st = g["lam"][mine]
        assert same(st[:, 1:], np.tile(np.array([0, 1, 0], F), (mine.size, 1))), tag + ": state"
        worst["l0"] = max(worst["l0"], worst_unit(tag + " l0", st[:, 0], ref["l0"][loc]))
        rows = g["inputs"][mine]
        assert same(rows[:, :L], np.tile(z[b], (mine.size, 1))), tag + ": latent of a row"
        pt = R.point(take(ref["rays"], loc), st[:, 0].astype(np.float64))          # 10 roundings: ray 6, slab (its l0 is taken from the device), 2 here
        for j in range(3):
            worst["x"] = max(worst["x"], worst_unit(tag + " x", rows[:, L + j], pt[j]))
    assert und <= 0.02 * tot
    print("TRACETEST setup %s: %d listed, %d of %d undecided, worst far %.3g l0 %.3g point %.3g bounds" % (tag, nl, und, tot, worst["far"], worst["l0"], worst["x"]))


@pytest.mark.parametrize("names", C.SETUP_BATCHES)
def test_setup_dense_every_pixel(names):
    """37 x 29, B = 3: far (0 when inactive), the zeroed hit records, the active set on decided rays, state (l0, 0, 1, 0), the input row,
    counters[0] with all others 0; a direction component that is exactly 0 with the origin inside / outside / on the slab, a camera inside the
    cube, a cube behind the camera"""
    _setup_case("dense " + "/".join(names), names, [(C.W0, C.H0)] * 3, C.W0 * C.H0, C.L3, 0, False)
    _setup_case("dense L=0 " + "/".join(names), names, [(C.W0, C.H0)] * 3, C.W0 * C.H0, 0, 0, False)


@pytest.mark.parametrize("block", [2, 4, 8])
def test_setup_with_cone_starts(block):
    """crafted cone starts (-1, below the entry, between entry and exit, beyond the exit) for blocks 2, 4, 8 -- 37 x 29 clips the last blocks"""
    for names in C.SETUP_BATCHES:
        _setup_case("cone %d %s" % (block, names[0]), names, [(C.W0, C.H0)] * 3, C.W0 * C.H0, C.L3, block, False)
    _setup_case("cone %d ragged" % block, C.SETUP_BATCHES[0], C.SIZES_R + [C.BAD_SIZES[0]], C.PS_R, C.L3, block, True)


@pytest.mark.parametrize("bad", C.BAD_SIZES)
def test_setup_ragged_and_a_crop_outside_the_contract(bad):
    """pix_stride 1280 with (37, 29), (40, 32) and a crop outside the contract at each position: it lists nothing and its slot holds zeros"""
    for pos in range(3):
        sizes = list(C.SIZES_R)
        sizes.insert(pos, bad)
        _setup_case("ragged %s at %d" % (bad, pos), ("generic", "axis_in", "inside"), sizes, C.PS_R, C.L3, 0, True)


# ---- sdfr_trace_step --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,step", [(1, 0), (63, 1), (64, 2), (65, 0), (256, 1), (257, 2), (1000, 0)])
def test_step_rule_on_crafted_states(n, step):
    """sdf is an input here, so hit / NaN / clamp decisions are exact: v = +-0, |v| one ulp either side of eps, NaN, +-inf, negative v, rho = 0,
    the ratio at both clamps, lam' equal to far (a miss) and one ulp below it on rays whose arithmetic is exact, far a safe distance either side"""
    case = C.step_case(n, 100 + n)
    ref = C.step_ref(case)
    assert (ref["ratio"] > 1).all()
    PS, L, B = C.W0 * C.H0, C.L3, 2
    cap = n + 300
    z = C.latn(B, L, 3)
    cnt0 = np.full(32, 41, I)
    cnt0[step % 3], cnt0[(step + 1) % 3], cnt0[(step + 2) % 3] = n, 5, 99
    o = dict(counters=Out(32, I, cnt0), pix=Out(cap, I), lam=Out((cap, 4), F), inputs=Out((cap, L + 3), F), hl=Out(B * PS, F), hs=Out(B * PS, F))
    pin, lin = np.full(cap, SENT_I, I), np.full((cap, 4), SENT_F, F)
    pin[:n], lin[:n] = case["pix"], case["st"]
    sdf = np.full(cap, SENT_F, F)
    sdf[:n] = case["v"]
    call("sdfr_trace_step", _lib.ptr(T(np.stack(C.STEP_POSES))), _lib.ptr(T(np.stack(C.STEP_KINV))), _lib.ptr(T(z)), L, C.W0, C.H0, C.EPS,
         _lib.ptr(T(sdf)), o["counters"].p, step, cap, _lib.ptr(T(pin)), _lib.ptr(T(lin)), o["pix"].p, o["lam"].p, _lib.ptr(T(case["far"])),
         o["inputs"].p, o["hl"].p, o["hs"].p)
    g = {k: v.get() for k, v in o.items()}
    del _alive[:]
    keep = np.nonzero(ref["what"] == 0)[0]
    hit = np.nonzero(ref["what"] == 1)[0]
    want = cnt0.copy()
    want[(step + 1) % 3], want[(step + 2) % 3] = 5 + keep.size, 0                  # n_next accumulates, n_zero is cleared
    assert same(g["counters"], want), g["counters"][:4]
    hl, hs = np.full(B * PS, SENT_F, F), np.full(B * PS, SENT_F, F)
    hl[case["pix"][hit]], hs[case["pix"][hit]] = case["st"][hit, 0], case["v"][hit]
    assert same(g["hl"], hl) and same(g["hs"], hs), "hit records: written only at hits, lam and value copied"
    lo, hi = 5, 5 + keep.size
    for k in ("pix", "lam", "inputs"):
        rest = np.concatenate([g[k][:lo], g[k][hi:]])
        assert (rest == (SENT_I if k == "pix" else SENT_F)).all(), k + " outside the appended range"
    slot_of = {int(p): lo + i for i, p in enumerate(g["pix"][lo:hi])}
    assert len(slot_of) == keep.size and set(slot_of) == set(int(p) for p in case["pix"][keep]), "survivors as a set"
    sl = np.array([slot_of[int(p)] for p in case["pix"][keep]], np.int64)
    st = g["lam"][sl]
    assert same(st[:, 1], ref["rho"][keep]) and same(st[:, 2], ref["q"][keep]) and same(st[:, 3], case["st"][keep, 3]), "rho, q (one division) and the spare word"
    fin = np.isfinite(ref["lam"].v[keep])
    assert same(st[~fin, 0], ref["lam"].v[keep][~fin].astype(F))
    w = worst_unit("lam'", st[fin, 0], ref["lam"][keep[fin]])                        # |d| (9 roundings), v / |d|, the sum
    rows = g["inputs"][sl]
    assert same(rows[:, :L], z[ref["b"][keep]])
    pt = R.point(take(ref["rays"], keep[fin]), st[fin, 0].astype(np.float64))
    wx = max(worst_unit("x", rows[fin, L + j], pt[j]) for j in range(3)) if fin.any() else 0.0
    assert not np.isfinite(rows[~fin, L:]).any()
    print("TRACETEST step n %d: %d hits, %d survivors, worst lam' %.3g point %.3g bounds" % (n, hit.size, keep.size, w, wx))


# ---- sdfr_trace_hits / _r ---------------------------------------------------------------------------------------------------------------------

def _hits_case(tag, sizes, PS, L, ragged, seed):
    B = len(sizes)
    names = ["generic", "axis_in", "inside"][:B]
    Pm, Ki = C.batch(names)
    z = C.latn(B, L, seed)
    hl = C.hit_record(sizes, PS, seed)
    n = B * PS
    o = dict(n_hits=Out(1, I, [0]), slot=Out(n, I), idx=Out(n, I), rows=Out((n, L + 3), F))
    tail = (_lib.ptr(T(hl)), o["n_hits"].p, o["slot"].p, o["idx"].p, o["rows"].p)
    if ragged:
        call("sdfr_trace_hits_r", _lib.ptr(T(Pm)), _lib.ptr(T(Ki)), Z(z), L, B, extents(sizes, PS), *tail)
    else:
        call("sdfr_trace_hits", _lib.ptr(T(Pm)), _lib.ptr(T(Ki)), Z(z), L, B, sizes[0][0], sizes[0][1], *tail)
    g = {k: v.get() for k, v in o.items()}
    del _alive[:]
    hit = np.stack([R.hits_crop(hl[b], W, H, PS) if valid(W, H, PS) else np.zeros(PS, bool) for b, (W, H) in enumerate(sizes)])
    cnt = int(hit.sum())
    assert int(g["n_hits"][0]) == cnt
    slot = g["slot"].reshape(B, PS)
    assert (slot[~hit] == -1).all(), tag + ": hit_slot of a pixel without a hit (slack pixels hold positive values)"
    assert same(np.sort(slot[hit]), np.arange(cnt, dtype=I)), tag + ": the slots are no bijection onto [0, count)"
    assert same(g["idx"][:cnt], np.arange(cnt, dtype=I)) and (g["idx"][cnt:] == SENT_I).all() and (g["rows"][cnt:] == SENT_F).all()
    w = 0.0
    for b, (W, H) in enumerate(sizes):
        px = np.nonzero(hit[b])[0]
        if px.size == 0:
            continue
        rows = g["rows"][slot[b, px]]
        assert same(rows[:, :L], np.tile(z[b], (px.size, 1)))
        pt = R.point(R.ray(Pm[b], Ki[b], (px % W).astype(np.float64), (px // W).astype(np.float64)), hl[b, px].astype(np.float64))
        w = max([w] + [worst_unit(tag + " row", rows[:, L + j], pt[j]) for j in range(3)])          # ray 6 roundings + 2
    print("TRACETEST hits %s: %d hits, worst point %.3g bounds" % (tag, cnt, w))


def test_hit_list_dense_and_ragged():
    """a crafted hit_lam (positive, +-0, negative, NaN; positive on the slack pixels of the ragged slots): hit_slot a bijection or -1, idx the
    identity, the rows at their slots, the count"""
    _hits_case("dense", [(C.W0, C.H0)] * 3, C.W0 * C.H0, C.L3, False, 7)
    _hits_case("dense L=0", [(C.W0, C.H0)] * 2, C.W0 * C.H0, 0, False, 8)
    for bad in C.BAD_SIZES:
        _hits_case("ragged %s" % (bad,), [C.SIZES_R[0], bad, C.SIZES_R[1]], C.PS_R, C.L3, True, 9)


# ---- sdfr_trace_composite / _r ----------------------------------------------------------------------------------------------------------------

def _composite_call(case, ragged, with_lam_s=True):
    B, PS, L = case["B"], case["PS"], case["L"]
    o = dict(color=Out((B, 3, PS), F), mask=Out((B, PS), F), depth=Out((B, PS), F), normals=Out((B, 3, PS), F), lam_s=Out((B, PS), F))
    tail = (_lib.ptr(T(case["hit_lam"])), _lib.ptr(T(case["hit_slot"])), _lib.ptr(T(case["J"])), _lib.ptr(T(case["f0"])), o["color"].p, o["mask"].p,
            o["depth"].p, o["normals"].p, o["lam_s"].p if with_lam_s else None)
    if ragged:
        call("sdfr_trace_composite_r", _lib.ptr(T(case["pose"])), _lib.ptr(T(case["Kinv"])), L, B, extents(case["sizes"], PS), *tail)
    else:
        call("sdfr_trace_composite", _lib.ptr(T(case["pose"])), _lib.ptr(T(case["Kinv"])), L, B, case["sizes"][0][0], case["sizes"][0][1], *tail)
    g = {k: v.get() for k, v in o.items()}
    del _alive[:]
    return g


def _composite_case(tag, sizes, PS, ragged, seed):
    case = C.render_case(sizes, PS, C.L3, seed)
    g = _composite_call(case, ragged)
    und = tot = 0
    w = dict(color=0.0, normals=0.0, depth=0.0, lam_s=0.0)
    zero = {k: v.copy() for k, v in g.items()}
    for b, cr in enumerate(case["crops"]):
        if cr is None:
            continue
        px, pol = cr["px"], cr["pol"]
        img = R.images(case["pose"][b], cr["rays"], pol)
        dec = pol["ratio"] > 1
        und += int((~dec).sum()); tot += px.size
        assert (g["mask"][b, px] == 1).all()
        for c in range(3):
            w["color"] = max(w["color"], worst_unit(tag + " colour", g["color"][b, c, px], img["color"][c], dec))      # point 10 roundings, polish 12, 2 here
            w["normals"] = max(w["normals"], worst_unit(tag + " normals", g["normals"][b, c, px], img["normals"][c]))  # |g| 4, division 2, rotation 3, 2 here
            zero["color"][b, c, px] = 0; zero["normals"][b, c, px] = 0
        w["depth"] = max(w["depth"], worst_unit(tag + " depth", g["depth"][b, px], img["depth"], dec))
        w["lam_s"] = max(w["lam_s"], worst_unit(tag + " lam_s", g["lam_s"][b, px], pol["lam_s"], dec))
        for k in ("mask", "depth", "lam_s"):
            zero[k][b, px] = 0
        for kind in range(C.GATE_KINDS):
            assert (dec & (cr["kinds"] == kind)).sum() >= 8, "gate kind %d is not populated" % kind
    for k, v in zero.items():
        assert same(v, np.zeros_like(v)), tag + ": %s is not +0 on a miss or a slack pixel" % k
    assert und <= 0.02 * tot
    g2 = _composite_call(case, ragged, with_lam_s=False)
    for k in ("color", "mask", "depth", "normals"):
        assert same(g[k], g2[k]), k + " with lam_s = NULL"
    assert (g2["lam_s"] == SENT_F).all()
    print("TRACETEST composite %s: %d hits, %d undecided gates, worst colour %.3g normals %.3g depth %.3g lam_s %.3g bounds" % (
        tag, tot, und, w["color"], w["normals"], w["depth"], w["lam_s"]))


def test_polish_and_images_every_pixel():
    """J and f0 are crafted: the gate |g . d| > 0.1 |g| |d| clearly on (both signs) and clearly off, g . d = 0, g = 0; all four images and lam_s
    on every pixel, +0 on misses and slack pixels; lam_s = NULL"""
    _composite_case("dense", [(C.W0, C.H0)] * 3, C.W0 * C.H0, False, 21)
    _composite_case("ragged", [C.SIZES_R[0], C.BAD_SIZES[1], C.SIZES_R[1]], C.PS_R, True, 22)


# ---- sdfr_trace_points / _r -------------------------------------------------------------------------------------------------------------------

def _points_case(tag, sizes, PS, ragged, seed, ecap, densities):
    B = len(sizes)
    rng = np.random.default_rng(seed)
    Ki = np.stack([C.KINV_GEN, C.KINV_AXIS, C.KINV_WIDE][:B])
    hit = np.zeros((B, PS), bool)
    for b, (W, H) in enumerate(sizes):
        if valid(W, H, PS):
            hit[b, :W * H] = rng.random(W * H) < densities[b]
    slot, _ = C.slots_of(hit.reshape(-1), seed)
    slot = slot.reshape(B, PS)
    slot[~hit] = np.where(rng.random((~hit).sum()) < 0.5, -1, -5)                  # any negative value is "no hit"
    lam_s = rng.uniform(1.5, 3.5, (B, PS)).astype(F)
    o = dict(xyzf=Out((B, ecap, 3), F), ecnt=Out(B, I), pt=Out((B, PS), I))
    tail = (_lib.ptr(T(slot)), _lib.ptr(T(lam_s)), o["xyzf"].p, ecap, o["ecnt"].p, o["pt"].p)
    if ragged:
        call("sdfr_trace_points_r", _lib.ptr(T(Ki)), B, extents(sizes, PS), *tail)
    else:
        call("sdfr_trace_points", _lib.ptr(T(Ki)), B, sizes[0][0], sizes[0][1], *tail)
    g = {k: v.get() for k, v in o.items()}
    del _alive[:]
    w = 0.0
    for b, (W, H) in enumerate(sizes):
        if not valid(W, H, PS):
            assert g["ecnt"][b] == 0 and (g["xyzf"][b] == SENT_F).all() and (g["pt"][b] == SENT_I).all()
            continue
        npx = W * H
        x, y = R.pixels(W, H)
        rays = dict(r=[(R.Ap(float(Ki[b, 3 * i])) * R.Ap(x) + R.Ap(float(Ki[b, 3 * i + 1])) * R.Ap(y)) + R.Ap(float(Ki[b, 3 * i + 2])) for i in range(3)])
        pt, cnt, keep, xyz = R.points_crop(hit[b, :npx], lam_s[b, :npx], rays, ecap)
        assert int(g["ecnt"][b]) == cnt, tag + ": ecnt is the TRUE count"
        assert same(g["pt"][b, :npx], pt), tag + ": pt_slot in pixel order, -1 beyond ecap"
        assert (g["pt"][b, npx:] == SENT_I).all(), tag + ": pt_slot of a slack pixel was written (the kernel leaves those words alone)"
        k = min(cnt, ecap)
        assert (g["xyzf"][b, k:] == SENT_F).all(), tag + ": rows beyond min(count, ecap)"
        for j in range(3):
            w = max(w, worst_unit(tag + " xyz", g["xyzf"][b, :k, j], xyz[j]))      # the pixel ray's 3 roundings and the product
    print("TRACETEST points %s: counts %s against ecap %d, worst %.3g bounds" % (tag, g["ecnt"].tolist(), ecap, w))


def test_points_in_pixel_order():
    """pt_slot and ecnt as exact integers; hits above ecap are dropped (guards intact, ecnt the true count); a 40 x 32 crop takes two trips of
    the kernel's loop; a crop without hits; ragged with a crop outside the contract"""
    _points_case("dense over ecap", [(C.W0, C.H0)] * 3, C.W0 * C.H0, False, 31, 300, (0.5, 0.0, 0.2))
    _points_case("dense two trips", [(40, 32)] * 2, 1280, False, 32, 1280, (0.7, 1.0))
    _points_case("dense at ecap", [(40, 32)] * 2, 1280, False, 33, 1280 // 2, (0.5, 1.0))
    for bad in C.BAD_SIZES:
        _points_case("ragged %s" % (bad,), [C.SIZES_R[0], bad, C.SIZES_R[1]], C.PS_R, True, 34, 700, (0.6, 0.5, 0.9))


# ---- sdfr_trace_refine_backward / _r, sdfr_trace_backward -------------------------------------------------------------------------------------

def _pt_slots(case, ecap, seed):
    """pt_slot as sdfr_trace_points leaves it (pixel order, -1 beyond ecap) -- plus, on a few hits, a row >= ecap: ignored by the backward"""
    B, PS = case["B"], case["PS"]
    pt = np.full((B, PS), -1, I)
    for b in range(B):
        pt[b], _, _, _ = R.points_crop(case["hit"][b], np.zeros(PS), dict(r=[R.Ap(np.zeros(PS))] * 3), ecap)
        h = np.nonzero(case["hit"][b])[0]
        if h.size > 4:
            pt[b, h[::5]] = ecap + 3
    return pt


def _bwd_call(entry, case, up, use, surfel, ecap, pt, ragged=False, crops=None):
    """one backward call on the crops `crops` of the case (default all); returns g_pose (B, 16), g_latn (B, L)"""
    sel = list(range(case["B"])) if crops is None else crops
    B, PS, L = len(sel), case["PS"], case["L"]
    W, H = case["sizes"][0]
    lib = _lib.lib()
    nws = int(lib.sdfr_trace_backward_ws_floats(B, PS, 1) if ragged else lib.sdfr_trace_backward_ws_floats(B, W, H))
    o = dict(ws=Out(nws, F), g_pose=Out((B, 16), F), g_latn=Out((B, max(L, 1)), F))
    gr = [(_lib.ptr(T(up[k][sel])) if k in use else None) for k in ("g_color", "g_depth", "g_normals", "g_xyzf")]
    head = (_lib.ptr(T(case["pose"][sel])), _lib.ptr(T(case["Kinv"][sel])), L, B)
    mid = (_lib.ptr(T(case["hit_lam"][sel])), _lib.ptr(T(case["hit_slot"][sel])), _lib.ptr(T(case["J"])), _lib.ptr(T(case["f0"])))
    if entry == "sdfr_trace_backward":
        call(entry, *head, W, H, *mid, gr[0], gr[1], gr[2], o["ws"].p, o["g_pose"].p, o["g_latn"].p)
    else:
        ext = (extents([case["sizes"][b] for b in sel], PS),) if ragged else (W, H)
        call(entry, *head, *ext, *mid, *gr, _lib.ptr(T(pt[sel])) if pt is not None else None, ecap, int(surfel), o["ws"].p, o["g_pose"].p, o["g_latn"].p)
    g = {k: v.get() for k, v in o.items()}
    del _alive[:]
    return g["g_pose"], g["g_latn"][:, :L]


def _bwd_ref(case, up, use, surfel, ecap, pt, b):
    cr = case["crops"][b]
    L, PS = case["L"], case["PS"]
    if cr is None:
        return R.Ap(np.zeros(R.NV))
    px = cr["px"]
    g_pt = None
    if "g_xyzf" in use:
        ps = pt[b, px]
        ok = (ps >= 0) & (ps < ecap)
        g_pt = np.where(ok[:, None], up["g_xyzf"][b, np.clip(ps, 0, ecap - 1)], F(0))
    terms = R.backward_terms(case["pose"][b], cr["rays"], cr["pol"], cr["J"], L,
                             g_color=up["g_color"][b][:, px].T if "g_color" in use else None,
                             g_depth=up["g_depth"][b, px] if "g_depth" in use else None,
                             g_normals=up["g_normals"][b][:, px].T if "g_normals" in use else None, g_pt=g_pt, surfel=surfel)
    return R.backward_sum(terms, PS)


def _bwd_judge(tag, case, up, use, surfel, ecap, pt, g_pose, g_latn):
    w = 0.0
    for b in range(case["B"]):
        ref = _bwd_ref(case, up, use, surfel, ecap, pt, b)
        got = np.concatenate([g_pose[b].reshape(4, 4)[:3, :3].reshape(-1), g_pose[b].reshape(4, 4)[:3, 3], g_latn[b], np.zeros(8 - case["L"], F)])
        # per term the roundings the reference counts (up to 22 on the rotation entries) + (8 + 8 + trips) eps32 / 2 of the |terms| for the two trees
        w = max(w, worst_unit("%s crop %d" % (tag, b), got, ref))
        assert same(g_pose[b, 12:], np.zeros(4, F)), tag + ": g_pose[12..15]"
    return w


ALL = ("g_color", "g_depth", "g_normals", "g_xyzf")


@pytest.mark.parametrize("W,H,L", [(16, 16, 0), (16, 16, 3), (16, 16, 8), (17, 16, 3)])
def test_backward_both_semantics_and_every_gradient_absent(W, H, L):
    """one block partial per crop (16 x 16) and two (17 x 16); L = 0, 3, 8; image and surfel semantics; each of the four gradient inputs NULL in
    turn, all present, only one present: all 12 pose entries and the L latent entries against the float64 sums; sdfr_trace_backward is
    sdfr_trace_refine_backward with the NULL arguments; L = 9 is refused"""
    PS, ecap = W * H, 60
    case = C.render_case([(W, H)] * 3, PS, L, 40 + L + W, density=0.6)
    for cr in case["crops"]:
        assert (cr["pol"]["ratio"] > 1).all(), "an undecided gate: the sums would not be comparable"
    up = C.upstream(3, PS, ecap, 5)
    pt = _pt_slots(case, ecap, 6)
    uses = [ALL] + [tuple(k for k in ALL if k != drop) for drop in ALL] + [(k,) for k in ALL] + [()]
    w = 0.0
    for surfel in (False, True):
        for use in uses:
            gp, gl = _bwd_call("sdfr_trace_refine_backward", case, up, use, surfel, ecap, pt)
            w = max(w, _bwd_judge("%dx%d L %d surfel %d %s" % (W, H, L, surfel, "+".join(use)), case, up, use, surfel, ecap, pt, gp, gl))
    img = ("g_color", "g_depth", "g_normals")
    a = _bwd_call("sdfr_trace_backward", case, up, img, False, 0, None)
    b = _bwd_call("sdfr_trace_refine_backward", case, up, img, False, 0, None)
    assert same(a[0], b[0]) and same(a[1], b[1])
    d = torch.zeros(64, device=DEV)
    rc = _lib.lib().sdfr_trace_refine_backward(d.data_ptr(), d.data_ptr(), 9, 1, 4, 4, d.data_ptr(), d.data_ptr(), d.data_ptr(), d.data_ptr(), None, None,
                                               None, None, None, 0, 0, d.data_ptr(), d.data_ptr(), d.data_ptr(), _lib.stream_ptr())
    assert rc != 0, "L = 9 must be refused"
    print("TRACETEST backward %dx%d L %d: %d calls, worst %.3g bounds" % (W, H, L, 2 * len(uses), w))


def test_backward_many_block_partials():
    """a 260 x 256 crop: more than 256 block partials, so the second kernel's threads 0 .. 3 take a second trip"""
    W, H, L, ecap = 260, 256, C.L3, 9000
    case = C.render_case([(W, H)], W * H, L, 77, poses=["generic"], density=0.3)
    assert (case["crops"][0]["pol"]["ratio"] > 1).mean() == 1.0
    up = C.upstream(1, W * H, ecap, 8)
    pt = _pt_slots(case, ecap, 9)
    w = 0.0
    for surfel in (False, True):
        gp, gl = _bwd_call("sdfr_trace_refine_backward", case, up, ALL, surfel, ecap, pt)
        w = max(w, _bwd_judge("260x256 surfel %d" % surfel, case, up, ALL, surfel, ecap, pt, gp, gl))
    print("TRACETEST backward 260x256: %d hits, worst %.3g bounds" % (case["n_hits"], w))


def test_backward_is_batch_independent_and_ragged():
    """a crop's result is bit-equal alone and at each position of a batch of three; the ragged entry point (a crop outside the contract gives
    zeros) equals the dense one bit for bit on the crops they share"""
    W, H, L, ecap = 17, 16, C.L3, 100
    PS = W * H
    case = C.render_case([(W, H)] * 3, PS, L, 55, density=0.5)
    up = C.upstream(3, PS, ecap, 5)
    pt = _pt_slots(case, ecap, 6)
    for surfel in (False, True):
        gp, gl = _bwd_call("sdfr_trace_refine_backward", case, up, ALL, surfel, ecap, pt)
        for order in ([0], [1], [2], [2, 0, 1], [1, 2, 0]):
            gp1, gl1 = _bwd_call("sdfr_trace_refine_backward", case, up, ALL, surfel, ecap, pt, crops=order)
            assert same(gp1, gp[order]) and same(gl1, gl[order]), "crops %s" % order
        gpr, glr = _bwd_call("sdfr_trace_refine_backward_r", case, up, ALL, surfel, ecap, pt, ragged=True)
        assert same(gpr, gp) and same(glr, gl), "ragged at the dense size"
    # ragged with slack and a crop outside the contract
    sizes, PSr = [(16, 16), C.BAD_SIZES[0], (17, 16)], 300
    case = C.render_case(sizes, PSr, L, 56, density=0.5)
    up = C.upstream(3, PSr, ecap, 7)
    pt = _pt_slots(case, ecap, 8)
    w = 0.0
    for surfel in (False, True):
        gp, gl = _bwd_call("sdfr_trace_refine_backward_r", case, up, ALL, surfel, ecap, pt, ragged=True)
        assert same(gp[1], np.zeros(16, F)) and same(gl[1], np.zeros(L, F))
        w = max(w, _bwd_judge("ragged surfel %d" % surfel, case, up, ALL, surfel, ecap, pt, gp, gl))
    print("TRACETEST backward ragged: worst %.3g bounds" % w)


# ---- one speculative pass of the looping kernel (mlp_kernel.h MODE 4), observed through the hand-over -------------------------------------------

@pytest.fixture(scope="module")
def slab_handle():
    dec = C.SlabDecoder(1.0).torch_decoder().to(DEV)
    h = dec.handle(torch.device(DEV, torch.cuda.current_device()))
    assert h.hp == 512 and not h.has_ln, "the slab decoder must take the looping kernel"
    return dec, h


SPEC_N = {4: (1, 15, 16, 17, 1000), 8: (1, 7, 8, 9, 1000), 16: (1, 3, 4, 5, 1000), 32: (1, 2, 3, 1000, 2100)}      # 1, t_rt - 1, t_rt, t_rt + 1, 1000


def _spec_run(handle, case, half):
    K, n = case["K"], case["n"]
    B, PS, L = 3, C.W0 * C.H0, C.L3
    nmax = B * PS
    Pm, Ki = C.batch(C.SPEC_POSES)
    cnt0 = np.zeros(32, I)
    cnt0[0] = n
    pix0, lam0 = np.full(nmax, SENT_I, I), np.full((nmax, 4), SENT_F, F)
    pix0[:n], lam0[:n] = case["pix"], case["st"]
    o = dict(counters=Out(32, I, cnt0), pix2=Out(nmax, I), lam2=Out((nmax, 4), F), hl=Out(nmax, F), hs=Out(nmax, F))
    zi, zf = (lambda *s: torch.zeros(s, dtype=torch.int32, device=DEV)), (lambda *s: torch.zeros(s, dtype=torch.float32, device=DEV))
    scratch = [zi(nmax), zf(nmax, 4), zf(nmax, L + 3), zf(nmax), zf(int(_lib.lib().sdfr_trace_pool()), 64, L + 3)]
    _alive.extend(scratch)
    levels = np.ascontiguousarray(np.array([[0, K], [1, 2 * K]], I))
    call("sdfr_trace_march", handle.h, _lib.ptr(T(Pm)), _lib.ptr(T(Ki)), Z(C.latn(3, L, 5)), L, B, C.W0, C.H0, C.EPS, 2, 0, 0, levels.ctypes.data, 2,
         C.QMAX, C.SIGMA, half, o["counters"].p, _lib.ptr(T(pix0)), _lib.ptr(T(lam0)), _lib.ptr(scratch[0]), _lib.ptr(scratch[1]), o["pix2"].p,
         o["lam2"].p, _lib.ptr(T(case["far"])), _lib.ptr(scratch[2]), _lib.ptr(scratch[3]), _lib.ptr(scratch[4]), o["hl"].p, o["hs"].p)
    g = {k: v.get() for k, v in o.items()}
    del _alive[:]
    return g


def _spec_check(tag, case, g):
    K, n = case["K"], case["n"]
    ref = C.spec_ref(case)
    assert (ref["ratio"] > 1).all()
    pix = case["pix"].astype(np.int64)
    keep, hit0 = np.nonzero(ref["keep"])[0], np.nonzero(ref["hit"])[0]
    cnt = g["counters"]
    ns = int(cnt[7])
    assert ns == keep.size, "%s: %d survivors handed over, the reference keeps %d" % (tag, ns, keep.size)
    assert (g["pix2"][ns:] == SENT_I).all() and (g["lam2"][ns:] == SENT_F).all()
    slot_of = {int(p): i for i, p in enumerate(g["pix2"][:ns])}
    assert len(slot_of) == ns and set(slot_of) == set(int(p) for p in pix[keep]), tag + ": the survivors as a set"
    sl = np.array([slot_of[int(p)] for p in pix[keep]], np.int64)
    st = g["lam2"][sl] if ns else np.zeros((0, 4), F)
    # the state after one pass: positions (up to K - 1 increments of 4 roundings on |d|'s 9), the decoder's tolerance at the accepted sample
    # carried through v / |d| and |v| / rho'; q' bit for bit where a clamp holds it
    w = dict(lam=worst_unit(tag + " lam'", st[:, 0], ref["lam"][keep]), rho=worst_unit(tag + " rho'", st[:, 1], ref["rho"][keep]),
             q=worst_unit(tag + " q'", st[:, 2], ref["q"][keep]))
    assert same(st[:, 3], case["st"][keep, 3]), tag + ": the state's spare word"
    # stage 1: one pass of 2 K samples from the states the device handed over (its own float32 numbers: exact inputs of the reference)
    ref1 = C.spec_ref(case, st=st, pix=pix[keep], K=2 * K) if ns else None
    hl, hs = g["hl"], g["hs"]
    touched = np.zeros(hl.size, bool)
    touched[pix[hit0]] = True
    w["hit"] = max(worst_unit(tag + " hit lam", hl[pix[hit0]], ref["pj"][hit0]), worst_unit(tag + " hit sdf", hs[pix[hit0]], ref["vj"][hit0]))
    und1 = 0
    unresolved_lo = unresolved_hi = 0
    if ns:
        dec1 = ref1["ratio"] > 1
        und1 = int((~dec1).sum())
        p1 = pix[keep]
        got_hit = hl[p1] != SENT_F
        assert np.array_equal(got_hit[dec1], ref1["hit"][dec1]), tag + ": stage 1 hit set on decided rays"
        both = got_hit & ref1["hit"]
        w["hit1"] = max(worst_unit(tag + " stage 1 hit lam", hl[p1][both], ref1["pj"][both]), worst_unit(tag + " stage 1 hit sdf", hs[p1][both], ref1["vj"][both]))
        touched[p1[got_hit]] = True
        unresolved_lo, unresolved_hi = int((ref1["keep"] & dec1).sum()), int((ref1["keep"] & dec1).sum()) + und1
    assert (hl[~touched] == SENT_F).all() and (hs[~touched] == SENT_F).all() and (hs[touched] != SENT_F).all(), tag + ": hit records elsewhere"
    assert unresolved_lo <= int(cnt[3]) <= unresolved_hi, (tag, cnt[3], unresolved_lo, unresolved_hi)
    evals = int(np.asarray(cnt[4:6]).view(np.uint64)[0])
    assert evals == n * K + ns * 2 * K, "%s: %d evaluations, live rays x samples are %d" % (tag, evals, n * K + ns * 2 * K)
    assert cnt[0] == n and not cnt[1:3].any() and cnt[6] == 0 and not cnt[8:16].any() and not cnt[18:].any(), cnt
    return w, ns, hit0.size, und1


@pytest.mark.parametrize("half", [0, 1])
@pytest.mark.parametrize("K", [4, 8, 16, 32])
def test_one_speculative_pass_through_the_hand_over(slab_handle, K, half):
    """sdfr_trace_march with head_steps = 0, levels [(0, K), (1, 2 K)], steps = 2 on uploaded lists: stage 0 runs exactly one pass of K samples
    from the crafted states (every accepted-prefix length, hits at sample 0 and later, a prefix ended by v <= 0, exits, rho = 0, q at 0.5 and
    q_max); its hits land in hit_lam / hit_sdf, its survivors with their state after the pass in pix2 / lam2 (count counters[7]).  Stage 1 then
    takes one pass of 2 K samples (64 for K = 32) from those states: hits and counters[3].  n = 1, t_rt - 1, t_rt, t_rt + 1, 1000; K = 32 also
    with more rays than the tile pool holds (1024 tiles of 2), so that workgroups fetch a second tile.  counters[4..5] = live rays x samples."""
    dec, h = slab_handle
    assert 2100 > int(_lib.lib().sdfr_trace_pool()) * (64 // 32)
    for n in SPEC_N[K]:
        case = C.spec_case(K, n, "f16" if half else "f32", 1000 * K + n)
        tag = "spec K %d n %d %s" % (K, n, "f16" if half else "f32")
        w, ns, nh, und1 = _spec_check(tag, case, _spec_run(h, case, half))
        print("TRACETEST %s: %d hits, %d survivors, worst %s bounds; stage 1: %d undecided" % (
            tag, nh, ns, " ".join("%s %.3g" % kv for kv in w.items()), und1))


# ---- sdfr_trace_cone: one pass ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", [1, 4, 8])
@pytest.mark.parametrize("block", [2, 4, 8])
def test_cone_setup_and_one_pass(slab_handle, block, K):
    """cone_steps = 1 makes the state after one pass visible in `cone`: -1 for a block whose rays all miss the cube, the sample a cone stopped at
    (its rays take over there), -1 for a cone that advanced past the far side, else where the cone got to.  Blocks 2, 4, 8 on 37 x 29 (clipped
    blocks), spec_k 1, 4, 8, poses under which some blocks miss the cube and most cones start at a centre point outside it (evaluated clamped).
    Per cone: the outcome on decided cones, the start within its bound; counters[4..5] = kept cones x spec_k."""
    dec, h = slab_handle
    B, L, W, H = 3, C.L3, C.W0, C.H0
    ref = C.cone_ref(block, K)
    nblk = ((W + block - 1) // block) * ((H + block - 1) // block)
    n = B * nblk
    Pm, Ki = C.batch(C.CONE_POSES)
    o = dict(counters=Out(32, I), cone=Out((B, nblk), F), ids0=Out(n, I), st0=Out((n, 4), F), aux0=Out((n, 2), F), ids1=Out(n, I), st1=Out((n, 4), F),
             aux1=Out((n, 2), F), inputs=Out((n * K, L + 3), F), sdf=Out(n * K, F))
    call("sdfr_trace_cone", h.h, _lib.ptr(T(Pm)), _lib.ptr(T(Ki)), Z(C.latn(3, L, 5)), L, B, W, H, C.BOUND, C.NEAR, C.EPS, block, 1, K, C.SIGMA, 0,
         o["counters"].p, o["ids0"].p, o["st0"].p, o["aux0"].p, o["ids1"].p, o["st1"].p, o["aux1"].p, o["inputs"].p, o["sdf"].p, o["cone"].p)
    g = {k: v.get() for k, v in o.items()}
    del _alive[:]
    kept = und = 0
    w = 0.0
    kinds = np.zeros(3, int)
    for b, (cs, res) in enumerate(ref):
        cone = g["cone"][b]
        assert (cs["ratio"] > 1).all(), "a block's slab decisions"
        assert same(cone[~cs["keep"]], np.full(int((~cs["keep"]).sum()), -1, F)), "blocks whose rays all miss the cube"
        got = cone[res["sel"]]
        dec_ = res["ratio"] > 1
        und += int((~dec_).sum()); kept += dec_.size
        kinds += np.bincount(res["kind"][dec_], minlength=3)
        culled = res["kind"] == 1
        assert np.array_equal((got == -1)[dec_], culled[dec_]), "crop %d: culled or not on decided cones" % b
        # start: block entry 8 roundings, K - 1 increments of 3, the centre point 10 and the decoder's row tolerance through free / (|d_c| + delta)
        w = max(w, worst_unit("cone start crop %d" % b, got, res["start"], dec_ & ~culled))
        # the cone phase's reason to exist, against the analytic first hit of every pixel: no ray of a culled block hits, and no block's
        # rays start beyond the first point at which one of them could report a hit (by more than the two float bounds)
        first, hits = C.slab_first_hit(C.CONE_POSES[b])
        start_tol = np.where(np.isfinite(res["start"].e), res["start"].e, 0.0)
        for i, k in enumerate(res["sel"]):
            ys, xs = np.meshgrid(np.arange(cs["y0"][k], cs["y1"][k] + 1), np.arange(cs["x0"][k], cs["x1"][k] + 1), indexing="ij")
            px = (ys * W + xs).reshape(-1)
            px = px[hits[px]]
            if got[i] == -1:
                assert px.size == 0, "crop %d block %d is culled, its pixel %d hits" % (b, k, px[0])
            elif px.size:
                slack = got[i] - (first.v[px] + first.e[px] + start_tol[i])
                assert slack.max() <= 0, "crop %d block %d starts %.3g beyond the first hit of pixel %d" % (b, k, slack.max(), px[slack.argmax()])
    if K == 4:
        # the ragged entry point: bit-identical at the dense size; with spare cone slots and a crop outside the contract the valid crops keep
        # their bits and the other's slots are not written
        for sizes, cap in (([(W, H)] * 3, nblk), ([(W, H), C.BAD_SIZES[1], (W, H)], nblk + 5)):
            nr = B * cap
            r = dict(counters=Out(32, I), cone=Out((B, cap), F), ids0=Out(nr, I), st0=Out((nr, 4), F), aux0=Out((nr, 2), F), ids1=Out(nr, I),
                     st1=Out((nr, 4), F), aux1=Out((nr, 2), F), inputs=Out((nr * K, L + 3), F), sdf=Out(nr * K, F))
            call("sdfr_trace_cone_r", h.h, _lib.ptr(T(Pm)), _lib.ptr(T(Ki)), Z(C.latn(3, L, 5)), L, B, extents(sizes, W * H, cap), C.BOUND, C.NEAR,
                 C.EPS, block, 1, K, C.SIGMA, 0, r["counters"].p, r["ids0"].p, r["st0"].p, r["aux0"].p, r["ids1"].p, r["st1"].p, r["aux1"].p,
                 r["inputs"].p, r["sdf"].p, r["cone"].p)
            gr = r["cone"].get()
            for v in r.values():
                v.get()
            del _alive[:]
            for b, (Wb, Hb) in enumerate(sizes):
                if valid(Wb, Hb, W * H):
                    assert same(gr[b, :nblk], g["cone"][b]) and (gr[b, nblk:] == SENT_F).all(), "ragged crop %d" % b
                else:
                    assert (gr[b] == SENT_F).all(), "a crop outside the contract wrote cone slots"
    cnt = g["counters"]
    evals = int(np.asarray(cnt[4:6]).view(np.uint64)[0])
    n_keep = sum(int(cs["keep"].sum()) for cs, _ in ref)
    assert evals == n_keep * K, (evals, n_keep, K)
    assert und <= 0.02 * kept
    print("TRACETEST cone block %d spec_k %d: %d cones, %d undecided, stop / culled / marching %s, worst start %.3g bounds" % (block, K, kept, und, kinds.tolist(), w))


# ---- sdfr_trace_march / _r: whole marches on the slab decoder ---------------------------------------------------------------------------------------

MARCH_CALLS = [("plain", 0, 4096), ("plain", 32, 0), ("plain", 5, 1 << 30), ("two", 32, 0), ("five", 32, 0), ("two", 2, 4096)]


def _march_run(h, names, sizes, PS, sched, head_steps, tail_rows, ragged):
    B, L = len(names), C.L3
    n = B * PS
    Pm = np.stack([C.MARCH_POSES[nm][0] for nm in names]); Ki = np.stack([C.MARCH_POSES[nm][1] for nm in names])
    z = np.tile(C.latn(1, L, 5), (B, 1))
    levels = np.ascontiguousarray(np.asarray(C.SCHEDULES[sched], I).reshape(-1, 2))
    o = dict(counters=Out(32, I), hl=Out(n, F), hs=Out(n, F), far=Out(n, F))
    zi, zf = (lambda *s: torch.zeros(s, dtype=torch.int32, device=DEV)), (lambda *s: torch.zeros(s, dtype=torch.float32, device=DEV))
    pix, lam = [zi(n), zi(n), zi(n)], [zf(n, 4), zf(n, 4), zf(n, 4)]
    inputs, sdf, tail = zf(n, L + 3), zf(n), zf(int(_lib.lib().sdfr_trace_pool()), 64 if len(levels) else 16, L + 3)
    _alive.extend(pix + lam + [inputs, sdf, tail])
    tp, tk, tz = _lib.ptr(T(Pm)), _lib.ptr(T(Ki)), Z(z)
    where = (extents(sizes, PS),) if ragged else (sizes[0][0], sizes[0][1])
    call("sdfr_trace_setup_r" if ragged else "sdfr_trace_setup2", tp, tk, tz, L, B, *where, C.BOUND, C.NEAR, o["counters"].p, _lib.ptr(pix[0]),
         _lib.ptr(lam[0]), o["far"].p, _lib.ptr(inputs), None, 0, o["hl"].p, o["hs"].p)
    call("sdfr_trace_march_r" if ragged else "sdfr_trace_march", h.h, tp, tk, tz, L, B, *where, C.EPS, C.MSTEPS, head_steps, tail_rows,
         levels.ctypes.data if len(levels) else None, len(levels), C.QMAX, C.SIGMA, 0, o["counters"].p, _lib.ptr(pix[0]), _lib.ptr(lam[0]),
         _lib.ptr(pix[1]), _lib.ptr(lam[1]), _lib.ptr(pix[2]), _lib.ptr(lam[2]), o["far"].p, _lib.ptr(inputs), _lib.ptr(sdf), _lib.ptr(tail),
         o["hl"].p, o["hs"].p)
    g = {k: v.get() for k, v in o.items()}
    del _alive[:]
    return g


@functools.lru_cache(maxsize=None)
def _march_ref(name, sched, W, H):
    return C.march_ref(name, sched, "f32", W, H)


def _march_check(tag, g, names, sizes, PS, sched):
    dec = C.SlabDecoder(1.0, "f32")
    z = C.latn(1, C.L3, 5)[0]
    und = tot = evals = unres = slack = 0
    w = dict(lam=0.0, sdf=0.0)
    for b, (nm, (W, H)) in enumerate(zip(names, sizes)):
        su, m = _march_ref(nm, sched, W, H)
        hl, hs = g["hl"][b * PS:(b + 1) * PS], g["hs"][b * PS:(b + 1) * PS]
        off = np.ones(PS, bool)
        off[m["px"]] = False
        assert same(hl[off], np.zeros(int(off.sum()), F)) and same(hs[off], np.zeros(int(off.sum()), F)), tag + ": a hit record outside the reference's active rays"
        got = hl[m["px"]] > 0
        d = m["ratio"] > 1
        und += int((~d).sum()); tot += d.size
        bad = np.nonzero((got != m["hit"]) & d)[0]
        assert bad.size == 0, "%s crop %d: the hit set differs on %d decided rays, first pixel %d" % (tag, b, bad.size, m["px"][bad[0]])
        both = got & m["hit"] & d
        # hit_lam: C_ACC x the sum of the one-step bounds of the passes the ray took (set-up entry 8 roundings, per pass the positions' 4 (K - 1),
        # the decoder's row tolerance through v / |d|, the sum)
        w["lam"] = max(w["lam"], worst_unit(tag + " hit_lam", hl[m["px"]], m["hit_lam"], both))
        # hit_sdf: below eps, and the decoder at the DEVICE's hit point within its row bound (+ the point's 10 roundings through the slope)
        hp = m["px"][got]
        assert (np.abs(hs[hp]) < F(C.EPS)).all(), tag + ": |hit_sdf| < eps"
        rays = dict(o=[c[hp] for c in su["rays"]["o"]], d=[c[hp] for c in su["rays"]["d"]])
        v = dec.value(np.tile(z, (hp.size, 1)))(R.point(rays, hl[hp].astype(np.float64)))
        w["sdf"] = max(w["sdf"], worst_unit(tag + " hit_sdf", hs[hp], v))
        evals += m["evals"]; unres += int((m["unresolved"] & d).sum()); slack += int((~d).sum()) * m["max_evals"]
    assert und <= 0.02 * tot
    cnt = g["counters"]
    assert unres <= int(cnt[3]) <= unres + und, (tag, cnt[3], unres, und)
    ev = int(np.asarray(cnt[4:6]).view(np.uint64)[0])
    assert abs(ev - evals) <= slack, "%s: %d evaluations, the reference counts %d (undecided rays may differ by %d)" % (tag, ev, evals, slack)
    return w, und, tot, ev, evals


@pytest.mark.parametrize("sched,head_steps,tail_rows", MARCH_CALLS)
def test_whole_march_every_pixel(slab_handle, sched, head_steps, tail_rows):
    """every pixel of three 48 x 40 crops, steps = 32, float32: per-step launches only (32, 0), the looping kernel from pass 0 (0, 4096), a
    hand-over after 5 per-step passes (5, 1 << 30), [(4, 4), (6, 16)] and five levels up to 64 samples behind a per-step head, and a
    count-gated hand-over in front of the first level (2, 4096).  Hit set on decided rays, hit_lam within the accumulated bound, |hit_sdf| < eps
    and equal to the reference decoder at the device's hit point, unresolved, evaluations (exact unless a ray is undecided)."""
    dec, h = slab_handle
    sizes, PS = [(C.MW, C.MH)] * 3, C.MW * C.MH
    g = _march_run(h, C.MARCH_BATCH, sizes, PS, sched, head_steps, tail_rows, False)
    tag = "march %s head %d tail %d" % (sched, head_steps, tail_rows)
    w, und, tot, ev, evals = _march_check(tag, g, C.MARCH_BATCH, sizes, PS, sched)
    print("TRACETEST %s: %d rays, %d undecided, evaluations %d (reference %d), worst hit_lam %.3g hit_sdf %.3g bounds" % (tag, tot, und, ev, evals, w["lam"], w["sdf"]))


@pytest.mark.parametrize("sched", ["plain", "five"])
def test_whole_march_ragged(slab_handle, sched):
    """sdfr_trace_march_r: three crops of their own sizes in slots of 1920 pixels"""
    dec, h = slab_handle
    g = _march_run(h, C.MARCH_BATCH, C.MARCH_SIZES_R, 1920, sched, 32, 0, True)
    w, und, tot, ev, evals = _march_check("march_r " + sched, g, C.MARCH_BATCH, C.MARCH_SIZES_R, 1920, sched)
    print("TRACETEST march_r %s: %d rays, %d undecided, evaluations %d (reference %d), worst hit_lam %.3g hit_sdf %.3g bounds" % (sched, tot, und, ev, evals, w["lam"], w["sdf"]))


@pytest.mark.parametrize("block,K,steps", [(2, 1, 10), (4, 1, 10), (2, 4, 4), (4, 4, 4), (8, 8, 4), (8, 1, 10)])
def test_cone_march_of_several_passes_never_culls_or_passes_a_hit(slab_handle, block, K, steps):
    """cone_steps = 4 and 10: the state between passes (a_prev, q, the compacted lists) is not visible, its one reason to exist is: against the
    analytic surface of the slab, no ray of a culled block hits, and no block starts beyond the point where one of its rays meets the surface.
    The tolerance is ONE step's float error, not an accumulated one: a pass proves its advance from the position the cone actually stands at,
    whatever rounding brought it there, so only the last advance's own arithmetic can carry a start past the surface --
    (decoder row tolerance + 8 u (1 + far delta)) / (|d_c| + delta) + 2 u far, with |d_c| >= 1 (r_z = 1), plus the analytic hit's own bound.
    The 8 roundings of an advance a = (v - p delta) / (|d_c| + delta), each on a quantity of at most 1 + far delta (|v| <= 1): the centre
    point o + p d (2, carried into v by the slope <= 1), the value outside the cube sqrt(cd^2 + max(v, 0)^2) (2: the sum and the root; cd's own
    are second order), the product p delta, the difference, the sum |d_c| + delta, the quotient; the last sum p + a rounds a number <= far (2 u far
    covers it and the hand-over of the start to the ray)."""
    dec, h = slab_handle
    B, L, W, H = 3, C.L3, C.W0, C.H0
    nblk = ((W + block - 1) // block) * ((H + block - 1) // block)
    n = B * nblk
    Pm, Ki = C.batch(C.CONE_POSES)
    o = dict(counters=Out(32, I), cone=Out((B, nblk), F), ids0=Out(n, I), st0=Out((n, 4), F), aux0=Out((n, 2), F), ids1=Out(n, I), st1=Out((n, 4), F),
             aux1=Out((n, 2), F), inputs=Out((n * K, L + 3), F), sdf=Out(n * K, F))
    call("sdfr_trace_cone", h.h, _lib.ptr(T(Pm)), _lib.ptr(T(Ki)), Z(C.latn(3, L, 5)), L, B, W, H, C.BOUND, C.NEAR, C.EPS, block, steps, K, C.SIGMA, 0,
         o["counters"].p, o["ids0"].p, o["st0"].p, o["aux0"].p, o["ids1"].p, o["st1"].p, o["aux1"].p, o["inputs"].p, o["sdf"].p, o["cone"].p)
    g = {k: v.get() for k, v in o.items()}
    del _alive[:]
    sd = C.SlabDecoder(1.0, "f32")
    zz = np.linspace(-1, 1, 4001)
    rows = np.concatenate([np.tile(C.latn(1, L, 5), (zz.size, 1)), np.zeros((zz.size, 2)), zz[:, None]], 1)
    dec_tol = float(sd.tol(sd.D.evaluate(sd.net_small, rows, "f32")).max())
    culled = started = 0
    worst = -np.inf
    for b, nm in enumerate(C.CONE_POSES):
        cs = R.cone_setup(*C.POSES[nm], W, H, block, C.BOUND, C.NEAR)
        assert (cs["ratio"] > 1).all()
        cone = g["cone"][b]
        assert same(cone[~cs["keep"]], np.full(int((~cs["keep"]).sum()), -1, F))
        first, hits = C.slab_first_hit(nm, widen=False)
        far_b, delta = cs["far"].v, cs["delta"].v
        for k in np.nonzero(cs["keep"])[0]:
            ys, xs = np.meshgrid(np.arange(cs["y0"][k], cs["y1"][k] + 1), np.arange(cs["x0"][k], cs["x1"][k] + 1), indexing="ij")
            px = (ys * W + xs).reshape(-1)
            px = px[hits[px]]
            if cone[k] == -1:
                culled += 1
                assert px.size == 0, "crop %d block %d is culled, its pixel %d hits" % (b, k, px[0])
            else:
                started += 1
                assert cone[k] >= F(C.NEAR) and cone[k] <= far_b[k] * (1 + 1e-6), "a start outside the block's range"
                if px.size:
                    tol = dec_tol + 8 * R.U * (1 + far_b[k] * delta[k]) + 2 * R.U * far_b[k]
                    slack = float((cone[k] - (first.v[px] + first.e[px] + tol)).max())
                    worst = max(worst, slack)
                    assert slack <= 0, "crop %d block %d starts %.3g beyond the surface" % (b, k, slack)
    assert culled >= 1 and started >= 8
    print("TRACETEST cone block %d spec_k %d steps %d: %d culled, %d started, closest start %.3g before the surface" % (block, K, steps, culled, started, -worst))


# ---- the generic per-step path: a LayerNorm decoder -------------------------------------------------------------------------------------------------

def test_layernorm_march_on_the_generic_path():
    """A 12 x 12 float32 march (two crops, 32 passes) on the LayerNorm fixture, which takes sdfr_trace_march's per-step path.  No accumulated
    bound is needed: the march is rebuilt from the device's OWN states -- decoder forward on the active rows, then sdfr_trace_step -- and every
    link is judged on its own: the decoder values against _decoder_ref at the device's rows within the row tolerance, the step against
    R.advance (its sdf is an input, so hit and clamp decisions are exact; lam' < far on decided rays).  sdfr_trace_march(head_steps = steps,
    tail_rows = 0) must then equal that chain bit for bit: hit records, rotating counters, unresolved, and evaluations = the live rays of every
    pass."""
    import sdflabel_amd
    from sdflabel_amd.fixtures import ASSET_ELLIPSOID_LN
    from tests import _decoder_ref as D
    d, _ = sdflabel_amd.setup_dsdf(ASSET_ELLIPSOID_LN + ".pt", precision=torch.float32)
    d = d.to(DEV)
    h = d.handle(torch.device(DEV, torch.cuda.current_device()))
    assert h.has_ln, "the fixture must take the generic path"
    net = D.Net.from_decoder(d.cpu())
    B, W, H, L, steps = 2, 12, 12, d.latent_size, 32
    PS, n = W * H, 2 * W * H
    Pm = np.stack([C.pose(C.rot(0.6, 0.2), [0.05, -0.03, 3.5]), C.pose(C.rot(-0.8, -0.3), [-0.1, 0.05, 3.2])])
    Ki = np.stack([C.kinv(20.0, 5.5, 5.5), C.kinv(18.0, 6.0, 5.0)])
    z = C.latn(B, L, 9)
    rays_all = [R.ray(Pm[b], Ki[b], *R.pixels(W, H)) for b in range(B)]

    def rays_of(gp):
        b, p = gp // PS, gp % PS
        pick = lambda f: R.Ap(np.where(b == 0, f(rays_all[0]).v[p], f(rays_all[1]).v[p]), np.where(b == 0, f(rays_all[0]).e[p], f(rays_all[1]).e[p]))
        return dict(o=[pick(lambda r, j=j: r["o"][j]) for j in range(3)], d=[pick(lambda r, j=j: r["d"][j]) for j in range(3)], dn=pick(lambda r: r["dn"])), b

    def fresh():
        zi, zf = (lambda *s: torch.zeros(s, dtype=torch.int32, device=DEV)), (lambda *s: torch.zeros(s, dtype=torch.float32, device=DEV))
        s = dict(counters=zi(32), pix=[zi(n), zi(n), zi(n)], lam=[zf(n, 4), zf(n, 4), zf(n, 4)], far=zf(n), inputs=zf(n, L + 3), sdf=zf(n),
                 hl=torch.full((n,), float(SENT_F), device=DEV), hs=torch.full((n,), float(SENT_F), device=DEV),
                 tail=zf(int(_lib.lib().sdfr_trace_pool()), 16, L + 3), tp=T(Pm), tk=T(Ki), tz=T(z))
        _alive.append(s)
        P = _lib.ptr
        call("sdfr_trace_setup2", P(s["tp"]), P(s["tk"]), P(s["tz"]), L, B, W, H, C.BOUND, C.NEAR, P(s["counters"]), P(s["pix"][0]), P(s["lam"][0]),
             P(s["far"]), P(s["inputs"]), None, 0, P(s["hl"]), P(s["hs"]))
        return s

    P = _lib.ptr
    # ---- the chain, every link judged
    s = fresh()
    far = s["far"].cpu().numpy()
    live, w_dec, w_lam, und = [], 0.0, 0.0, 0
    for step in range(steps):
        a = step & 1
        cur = int(s["counters"][step % 3])
        live.append(cur)
        call("sdfr_mlp_forward_counted", h.h, P(s["inputs"]), n, s["counters"].data_ptr() + 4 * (step % 3), P(s["sdf"]), 0)
        pix_in, st_in = s["pix"][a][:cur].cpu().numpy().astype(np.int64), s["lam"][a][:cur].cpu().numpy()
        rows, v = s["inputs"][:cur].cpu().numpy(), s["sdf"][:cur].cpu().numpy()
        call("sdfr_trace_step", P(s["tp"]), P(s["tk"]), P(s["tz"]), L, W, H, C.EPS, P(s["sdf"]), P(s["counters"]), step, n, P(s["pix"][a]),
             P(s["lam"][a]), P(s["pix"][1 - a]), P(s["lam"][1 - a]), P(s["far"]), P(s["inputs"]), P(s["hl"]), P(s["hs"]))
        if cur == 0:
            continue
        r = D.evaluate(net, rows, "f32")
        w_dec = max(w_dec, float(D.judge_forward(net, r, v, "f32").max()))
        rays, bb = rays_of(pix_in)
        what, l2, rho, q, rt = R.advance(st_in, v, rays["dn"], C.EPS, far[pix_in])
        dec_ = rt > 1
        und += int((~dec_).sum())
        nxt = int(s["counters"][(step + 1) % 3])
        pix_out, st_out = s["pix"][1 - a][:nxt].cpu().numpy().astype(np.int64), s["lam"][1 - a][:nxt].cpu().numpy()
        rows_out = s["inputs"][:nxt].cpu().numpy()
        slot_of = {int(p): i for i, p in enumerate(pix_out)}
        assert len(slot_of) == nxt
        kept = np.array([int(p) in slot_of for p in pix_in])
        assert np.array_equal(kept[dec_], (what == 0)[dec_]), "pass %d: survivors on decided rays" % step
        k = np.nonzero(kept & (what == 0))[0]
        sl = np.array([slot_of[int(p)] for p in pix_in[k]], np.int64)
        if k.size:
            w_lam = max(w_lam, worst_unit("pass %d lam'" % step, st_out[sl, 0], l2[k]))          # |d| 9 roundings, v / |d|, the sum
            assert same(st_out[sl, 1], rho[k]) and same(st_out[sl, 2], q[k]), "pass %d: rho', q'" % step
            assert same(rows_out[sl, :L], z[bb[k]])
            pt = R.point(dict(o=[c[k] for c in rays["o"]], d=[c[k] for c in rays["d"]]), st_out[sl, 0].astype(np.float64))
            for j in range(3):
                worst_unit("pass %d point" % step, rows_out[sl, L + j], pt[j])
        hl_now, hs_now = s["hl"].cpu().numpy(), s["hs"].cpu().numpy()
        hits = pix_in[what == 1]
        assert same(hl_now[hits], st_in[what == 1, 0]) and same(hs_now[hits], v[what == 1]), "pass %d: hit records" % step
    assert w_dec <= 1.0, "decoder values at the device's rows: %.3g of the row tolerance" % w_dec
    chain = dict(hl=s["hl"].cpu().numpy(), hs=s["hs"].cpu().numpy(), counters=s["counters"].cpu().numpy())
    left = int(chain["counters"][steps % 3])
    nh = int((chain["hl"] > 0).sum())
    assert nh >= 8 and sum(live) > live[0] and live[0] >= 64
    assert (np.abs(chain["hs"][chain["hl"] > 0]) < F(C.EPS)).all()
    # ---- the march in one call: the same bits
    m = fresh()
    call("sdfr_trace_march", h.h, P(m["tp"]), P(m["tk"]), P(m["tz"]), L, B, W, H, C.EPS, steps, steps, 0, None, 0, 1.0, C.SIGMA, 0, P(m["counters"]),
         P(m["pix"][0]), P(m["lam"][0]), P(m["pix"][1]), P(m["lam"][1]), P(m["pix"][2]), P(m["lam"][2]), P(m["far"]), P(m["inputs"]), P(m["sdf"]),
         P(m["tail"]), P(m["hl"]), P(m["hs"]))
    got = dict(hl=m["hl"].cpu().numpy(), hs=m["hs"].cpu().numpy(), counters=m["counters"].cpu().numpy())
    del _alive[:]
    assert same(got["hl"], chain["hl"]) and same(got["hs"], chain["hs"]), "the march's hit records differ from the chain of its own steps"
    assert same(got["counters"][:3], chain["counters"][:3]) and int(got["counters"][3]) == left
    assert int(np.asarray(got["counters"][4:6]).view(np.uint64)[0]) == sum(live), "evaluations = the live rays of every pass"
    assert not got["counters"][6:].any()
    print("TRACETEST LayerNorm march 12x12: %d rays, live per pass %s, %d hits, %d unresolved, %d undecided exits, decoder %.3g of its tolerance, lam' %.3g bounds" % (
        live[0], live[:8], nh, left, und, w_dec, w_lam))
