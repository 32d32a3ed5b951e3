"""The loss and solver kernels (csrc/losses.hip, csrc/solver.h) through the C ABI against the float64 references of tests/_loss_ref.py, on every
path: the three template instantiations of the 2-D loss, plain / ragged / fused, one- and multi-tile 3-D searches, the tie rule, the edge
semantics, and the Adam / SGD step with its skip rules.

Acceptance rule of a gradient row: within 1e-5 absolute, on the normalised gradient, of the row of SOME member of that pixel's / point's
candidate set (every distinct value within 1e-5 of the float64 minimum).  tests/test_loss_refs_cpu.py bounds the rows with more than one
member at 1 % of each input and keeps every minimum away from the thresholds, on the references alone.  Loss: 1e-5 * max(1, diam); counts: exact.
Output buffers are pre-filled with 7.0: an unwritten element shows.  Each test prints its largest observed errors (pytest -s)."""
import numpy as np
import pytest
import torch

from sdflabel_amd import _lib
from tests import _loss_cases as C
from tests._loss_ref import loss_2d_ref, loss_3d_ref, match_rows, solver_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5


def T(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t.to(DEV) if dtype is None else t.to(DEV, dtype)


def N(t):
    return t.detach().cpu().numpy()


def filled(shape, dtype=torch.float32):
    return torch.full(shape, 7, dtype=dtype, device=DEV)


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


_REFS = {}


def ref_2d(key, rend, tgt, diam, thr):
    k = ("2d", key, diam, thr)
    if k not in _REFS:
        _REFS[k] = loss_2d_ref(rend, tgt, diam, thr)
    return _REFS[k]


def ref_3d(key, est, lid, scale, thr):
    k = ("3d", key, thr)
    if k not in _REFS:
        _REFS[k] = loss_3d_ref(est, lid, scale, thr)
    return _REFS[k]


# ---- calls ---------------------------------------------------------------------------------------------------------------------------------

def tiles16(H, W):
    return ((W + 15) // 16) * ((H + 15) // 16)


def call_2d(rend, tgt, diam, thr, weight=1.0):
    """rend, tgt (B, 3, H, W) -> loss (B,), g (B, 3, H, W), nvalid (B,)"""
    L = _lib.lib()
    B, _, H, W = rend.shape
    r, t = T(rend), T(tgt)
    loss, g, nv, scr = filled((B,)), filled((B, 3, H, W)), filled((B,), torch.int32), filled((3 * B * tiles16(H, W),))
    _lib.check(L.sdfr_loss_2d(_lib.ptr(r), _lib.ptr(t), B, H, W, diam, thr, weight, _lib.ptr(loss), _lib.ptr(g), _lib.ptr(nv), _lib.ptr(scr),
                              _lib.stream_ptr()), "sdfr_loss_2d")
    torch.cuda.synchronize()
    return N(loss), N(g), N(nv)


def slots_2d(crops, pst):
    """[(name, rend, target)] -> rend / target slots (B, 3, pst) and extents wh (B, 2) = (W_b, H_b)"""
    B = len(crops)
    rng = np.random.default_rng(99)
    r = rng.random((B, 3, pst)).astype(np.float32)                       # the rest of a slot holds anything
    t = rng.random((B, 3, pst)).astype(np.float32)
    wh = np.zeros((B, 2), np.int32)
    for b, (_, rr, tt) in enumerate(crops):
        H, W = rr.shape[1:]
        wh[b] = (W, H)
        n = min(H * W, pst)
        r[b, :, :n] = rr.reshape(3, -1)[:, :n]
        t[b, :, :n] = tt.reshape(3, -1)[:, :n]
    return r, t, wh


def call_2d_r(r, t, wh, pst, tcap, diam, thr, weight=1.0):
    L = _lib.lib()
    B = r.shape[0]
    rd, td, whd = T(r), T(t), T(wh)
    loss, g, nv, scr = filled((B,)), filled((B, 3, pst)), filled((B,), torch.int32), filled((3 * B * tcap,))
    _lib.check(L.sdfr_loss_2d_r(_lib.ptr(rd), _lib.ptr(td), B, _lib.ptr(whd), pst, tcap, diam, thr, weight, _lib.ptr(loss), _lib.ptr(g),
                                _lib.ptr(nv), _lib.ptr(scr), _lib.stream_ptr()), "sdfr_loss_2d_r")
    torch.cuda.synchronize()
    return N(loss), N(g), N(nv)


def pack_3d(crops, ecap, lcap):
    """[(name, est rows, lidar rows, ecnt, lcnt, scale)] -> padded arrays; the rows beyond a crop's own hold random points"""
    B = len(crops)
    rng = np.random.default_rng(98)
    est = rng.random((B, ecap, 3)).astype(np.float32)
    lid = rng.random((B, lcap, 3)).astype(np.float32)
    for b, (_, e, l, _, _, _) in enumerate(crops):
        est[b, :e.shape[0]] = e
        lid[b, :l.shape[0]] = l
    ecnt = np.array([c[3] for c in crops], np.int32)
    lcnt = np.array([c[4] for c in crops], np.int32)
    scale = np.array([c[5] for c in crops], np.float32)
    return est, ecnt, lid, lcnt, scale


def call_3d(est, ecnt, lid, lcnt, scale, thr, weight=1.0):
    L = _lib.lib()
    B, ecap, _ = est.shape
    lcap = lid.shape[1]
    e, ec, l, lc, s = T(est), T(ecnt), T(lid), T(lcnt), T(scale)
    loss, g, gs, npairs = filled((B,)), filled((B, ecap, 3)), filled((B,)), filled((B,), torch.int32)
    scr = filled((3 * B * ((ecap + 63) // 64),))
    _lib.check(L.sdfr_loss_3d(_lib.ptr(e), _lib.ptr(ec), ecap, _lib.ptr(l), _lib.ptr(lc), lcap, _lib.ptr(s), thr, weight, B, _lib.ptr(loss),
                              _lib.ptr(g), _lib.ptr(gs), _lib.ptr(npairs), _lib.ptr(scr), _lib.stream_ptr()), "sdfr_loss_3d")
    torch.cuda.synchronize()
    return N(loss), N(g), N(gs), N(npairs)


def call_fused(r, t, wh, pst, tcap, diam, thr2, w2, est, ecnt, lid, lcnt, scale, thr3, w3):
    """r, t: (B, 3, H, W) with wh None, or slots (B, 3, pst) with extents wh.  Returns the 2-D triple with g * kscale[:, 0] and the 3-D
    quadruple with g_est * kscale[:, 1] (the products the consumers form on load)."""
    L = _lib.lib()
    B, ecap, _ = est.shape
    lcap = lid.shape[1]
    if wh is None:
        H, W = r.shape[2:]
        nt, whd = tiles16(H, W), None
    else:
        H = W = 0
        nt, whd = tcap, T(wh)
    rd, td = T(r), T(t)
    e, ec, l, lc, s = T(est), T(ecnt), T(lid), T(lcnt), T(scale)
    loss2, g2, nv, scr2 = filled((B,)), filled(tuple(r.shape)), filled((B,), torch.int32), filled((3 * B * nt,))
    loss3, g3, gs, npairs = filled((B,)), filled((B, ecap, 3)), filled((B,)), filled((B,), torch.int32)
    scr3, ks = filled((3 * B * ((ecap + 63) // 64),)), filled((B, 2))
    _lib.check(L.sdfr_losses_fused(_lib.ptr(rd), _lib.ptr(td), B, H, W, _lib.ptr(whd), pst if wh is not None else 0, tcap if wh is not None else 0,
                                   diam, thr2, w2, _lib.ptr(loss2), _lib.ptr(g2), _lib.ptr(nv), _lib.ptr(scr2),
                                   _lib.ptr(e), _lib.ptr(ec), ecap, _lib.ptr(l), _lib.ptr(lc), lcap, _lib.ptr(s), thr3, w3, _lib.ptr(loss3),
                                   _lib.ptr(g3), _lib.ptr(gs), _lib.ptr(npairs), _lib.ptr(scr3), _lib.ptr(ks), _lib.stream_ptr()), "sdfr_losses_fused")
    torch.cuda.synchronize()
    g2n = g2 * ks[:, 0].reshape((B,) + (1,) * (g2.dim() - 1))
    g3n = g3 * ks[:, 1].reshape(B, 1, 1)
    return (N(loss2), N(g2n), N(nv)), (N(loss3), N(g3n), N(gs), N(npairs))


# ---- checks --------------------------------------------------------------------------------------------------------------------------------

def check_2d(name, ref, loss, g, nv, diam, weight=1.0):
    """one crop: loss scalar, g (3, H, W), nv scalar, against its reference.  Returns (loss error, gradient error, rows accepted through a
    candidate other than the reference's own)."""
    if np.isnan(ref.loss):
        assert np.isnan(loss), (name, float(loss), "expected NaN")
        lerr = 0.0
    else:
        lerr = abs(float(loss) - ref.loss)
        assert lerr <= TOL * max(1.0, diam), (name, float(loss), ref.loss)
    assert int(nv) == ref.nvalid, (name, int(nv), ref.nvalid)
    assert np.isfinite(g).all(), name
    err, pick = match_rows(g[:, ref.ys, ref.xs].T, [r * weight for r in ref.rows])
    gerr = float(err.max()) if err.size else 0.0
    assert gerr <= TOL, (name, "%d rendered pixel(s) beyond the tolerance, worst %.3g at (%d, %d)"
                         % ((err > TOL).sum(), gerr, ref.ys[err.argmax()], ref.xs[err.argmax()]))
    rest = g.copy()
    rest[:, ref.ys, ref.xs] = 0
    assert not rest.any(), (name, "gradient on an unrendered pixel (or an unwritten one)")
    return lerr, gerr, int((pick > 0).sum())


def check_3d(name, ref, ne, loss, g, gs, npairs, weight=1.0):
    """one crop: g (ecap, 3)"""
    assert int(npairs) == ref.npairs, (name, int(npairs), ref.npairs)
    lerr = abs(float(loss) - ref.loss)
    assert lerr <= TOL, (name, float(loss), ref.loss)
    assert not g[ne:].any(), (name, "rows beyond the count must be exactly 0")
    if ref.npairs < 0:
        assert not g.any() and float(gs) == 0.0, name
        return lerr, 0.0, 0
    err, pick = match_rows(g[:ne], [r * weight for r in ref.rows])
    gerr = float(err.max())
    assert gerr <= TOL, (name, "%d row(s) beyond the tolerance, worst %.3g at %d" % ((err > TOL).sum(), gerr, err.argmax()))
    gs_ref = weight * sum(x[p] for x, p in zip(ref.gs_rows, pick))
    assert abs(float(gs) - gs_ref) <= TOL * max(1.0, abs(gs_ref)), (name, float(gs), gs_ref)
    return lerr, gerr, int((pick > 0).sum())


def report(family, stats):
    stats = [s for s in stats if s is not None]
    print("\nLOSSTEST %s: cases %d, max |loss - ref| %.3g, max gradient error %.3g, rows through a non-first candidate %d"
          % (family, len(stats), max(s[0] for s in stats), max(s[1] for s in stats), sum(s[2] for s in stats)))


# ---- 2-D -----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", C.SHAPES + C.DENSE_SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("diam", C.DIAMS)
def test_loss_2d_single_crop(diam, shape):
    """one crop per call: tile-boundary, halo and empty-tile layouts (tests/_loss_cases.py image_2d) and the small dense crops, where no pixel
    of the image has weight 0 and the rendered colour's own norm is not a candidate."""
    H, W = shape
    rend, tgt = C.single_2d(H, W)
    stats = []
    for thr in C.THRESHOLDS_2D:
        ref = ref_2d(("single", H, W), rend, tgt, diam, thr)
        loss, g, nv = call_2d(rend[None], tgt[None], diam, thr)
        print("\n  %dx%d diam %g thr %g: loss %.7g ref %.7g nvalid %d" % (H, W, diam, thr, loss[0], ref.loss, nv[0]))
        stats.append(check_2d("%dx%d diam %g thr %g" % (H, W, diam, thr), ref, loss[0], g[0], nv[0], diam))
    report("2d single %dx%d diam %g" % (H, W, diam), stats)


@pytest.mark.parametrize("shape", C.BATCH_SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("diam", C.DIAMS)
def test_loss_2d_batch_of_distinct_crops(diam, shape):
    """B = 6 in one call: a normal crop, an all-zero rendering, only pixel (0, 0) rendered (the reference tests the SUM of the indices,
    optimizer.py:214: loss 0), every minimum above the threshold (NaN, nvalid 0), pixels with channel sum 0 (unrendered), the dense small crop.
    Each crop equals its own reference."""
    H, W = shape
    crops = C.batch_2d(H, W, diam)
    rend, tgt = np.stack([c[1] for c in crops]), np.stack([c[2] for c in crops])
    stats = []
    for thr in C.BATCH_THRESHOLDS:
        loss, g, nv = call_2d(rend, tgt, diam, thr)
        for b, (name, r, t) in enumerate(crops):
            ref = ref_2d(("batch", H, W, name), r, t, diam, thr)
            print("\n  batch %dx%d %s diam %g thr %g: loss %.7g ref %.7g nvalid %d" % (H, W, name, diam, thr, loss[b], ref.loss, nv[b]))
            stats.append(check_2d("%s diam %g thr %g" % (name, diam, thr), ref, loss[b], g[b], nv[b], diam))
            if name in ("zero", "origin"):
                assert float(loss[b]) == 0.0 and not g[b].any()
            if name == "far":
                assert np.isnan(loss[b]) and nv[b] == 0 and not g[b].any()
    report("2d batch %dx%d diam %g" % (H, W, diam), stats)


def _check_ragged(crops, pst, diam, thr, loss, g, nv, weight=1.0):
    stats = []
    for b, (name, r, t) in enumerate(crops):
        H, W = r.shape[1:]
        if H * W > pst:                                                  # outside the contract: an empty crop
            assert float(loss[b]) == 0.0 and int(nv[b]) == 0, (name, loss[b], nv[b])
            continue
        ref = ref_2d(("ragged", name), r, t, diam, thr)
        stats.append(check_2d("ragged %s diam %g thr %g" % (name, diam, thr), ref, loss[b], g[b, :, :H * W].reshape(3, H, W), nv[b], diam, weight))
    return stats


@pytest.mark.parametrize("diam", C.DIAMS)
def test_loss_2d_ragged_slots(diam):
    """sdfr_loss_2d_r: five crops of different extents in slots of one pix_stride (one 1 x 1, one larger than its slot: loss 0, nvalid 0).
    Pixels [0, W_b * H_b) of each channel slot are compared; the rest of a slot is not part of the contract."""
    crops = C.ragged_2d()
    pst, tcap = C.RAGGED_PIX_STRIDE, C.RAGGED_TILES_CAP
    r, t, wh = slots_2d(crops, pst)
    stats = []
    for thr in C.THRESHOLDS_2D:
        loss, g, nv = call_2d_r(r, t, wh, pst, tcap, diam, thr)
        stats += _check_ragged(crops, pst, diam, thr, loss, g, nv)
    report("2d ragged diam %g" % diam, stats)


# ---- 3-D -----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cloud", C.CLOUDS, ids=lambda c: "%dx%d" % c[:2])
def test_loss_3d_cloud(cloud):
    """one to four lidar tiles, capacities that are no multiples of 64, fewer lidar points than waves"""
    ne, nl, ecap, lcap, scale = cloud
    est, lid = C.cloud_3d(ne, nl, scale)
    ref = ref_3d(("cloud", ne, nl), est, lid, scale, C.THRESHOLD_3D)
    loss, g, gs, npairs = call_3d(*pack_3d([("c", est, lid, ne, nl, scale)], ecap, lcap), C.THRESHOLD_3D)
    print("\n  cloud %dx%d: loss %.7g ref %.7g npairs %d g_scale %.7g ref %.7g" % (ne, nl, loss[0], ref.loss, npairs[0], gs[0], ref.g_scale))
    report("3d cloud %dx%d" % (ne, nl), [check_3d("cloud %dx%d" % (ne, nl), ref, ne, loss[0], g[0], gs[0], npairs[0])])


def _check_batch_3d(crops, ecap, loss, g, gs, npairs, weight=1.0):
    stats = []
    for b, (name, e, l, ec, lc, scale) in enumerate(crops):
        ne = min(ec, ecap)
        ref = ref_3d(("batch", name), e[:ne], l[:lc], scale, C.THRESHOLD_3D)
        stats.append(check_3d("batch " + name, ref, ne, loss[b], g[b], gs[b], npairs[b], weight))
        if name in ("nolidar", "noest"):
            assert int(npairs[b]) == -1 and float(loss[b]) == 0.0 and not g[b].any()
    return stats


def test_loss_3d_batch_with_per_crop_counts():
    """B = 5 in one call: normal; no lidar point (npairs -1, loss 0, gradient 0); no estimated point (same); a count above the capacity
    (clamped); a single estimated point."""
    ecap, lcap = 1000, 1025
    crops = C.batch_3d(ecap, lcap)
    loss, g, gs, npairs = call_3d(*pack_3d(crops, ecap, lcap), C.THRESHOLD_3D)
    report("3d batch", _check_batch_3d(crops, ecap, loss, g, gs, npairs))


@pytest.mark.parametrize("scale", C.TIE_SCALES)
def test_loss_3d_ties_resolve_to_the_lowest_lidar_index(scale):
    """The project's own documented rule (csrc/losses.hip: "ties resolve to the lowest lidar index, as a sequential scan would"); the
    reference's KDTree leaves the winner of an exact tie unspecified.  Lidar: a 13^3 lattice in shuffled order (three tiles); estimated
    points: edge, face and cell midpoints, so 2, 4 or 8 lidar points are nearest at the same exact float32 squared distance, spread over
    waves and tiles (tests/test_loss_refs_cpu.py checks that they are).  The gradient row names the winner."""
    est, lidar, winner, tied = C.lattice_3d(scale)
    ne, nl = est.shape[0], lidar.shape[0]
    ecap, lcap = 3904, 2200
    loss, g, gs, npairs = call_3d(*pack_3d([("tie", est, lidar, ne, nl, scale)], ecap, lcap), C.TIE_THRESHOLD)
    assert int(npairs[0]) == ne
    fr = (lidar / np.float32(scale)).astype(np.float64)
    e = est.astype(np.float64)
    chosen = np.zeros(ne, np.int64)
    worst = 0.0
    for j in range(ne):
        d = fr[tied[j]] - e[j]
        rows = -d / np.sqrt((d * d).sum(1))[:, None] / ne
        err = np.abs(rows - g[0, j].astype(np.float64)).max(1)
        chosen[j] = tied[j][err.argmin()]
        worst = max(worst, err.min())
    assert worst <= TOL, worst
    wrong = np.nonzero(chosen != winner)[0]
    print("\nLOSSTEST 3d ties scale %g: %d points, %d resolved to another index than the lowest, row error %.3g" % (scale, ne, wrong.size, worst))
    assert wrong.size == 0, ("%d of %d ties not resolved to the lowest index, e.g. point %d: chose %d (tile, wave %s) over %d (%s)"
                             % (wrong.size, ne, wrong[0], chosen[wrong[0]], C.scan_slot(chosen[wrong[0]], nl), winner[wrong[0]],
                                C.scan_slot(winner[wrong[0]], nl)))
    dmin = np.array([np.sqrt(((fr[w] - e[j]) ** 2).sum()) for j, w in enumerate(winner)])
    assert abs(float(loss[0]) - dmin.mean()) <= TOL


# ---- fused ---------------------------------------------------------------------------------------------------------------------------------

def _same_bits(a, b, what):
    assert np.array_equal(bits(a), bits(b)), what + ": fused and separate calls differ in bits"


@pytest.mark.parametrize("ragged", [False, True], ids=["dense", "ragged"])
@pytest.mark.parametrize("diam", C.DIAMS)
def test_losses_fused_against_the_references_and_the_separate_calls(diam, ragged):
    """sdfr_losses_fused on the inputs of the batched 2-D and 3-D tests, with the loop's weights: g * kscale[b, 0] and g_est * kscale[b, 1]
    pass the reference checks, and loss, nvalid, npairs, g_scale and both products carry the bits of the separate calls."""
    w2, w3 = C.W2, C.W3
    stats2, stats3 = [], []
    if ragged:
        crops2 = C.ragged_2d()
        pst, tcap = C.RAGGED_PIX_STRIDE, C.RAGGED_TILES_CAP
        r, t, wh = slots_2d(crops2, pst)
        crops3 = C.batch_3d()
        thresholds = C.THRESHOLDS_2D
    else:
        H, W = 12, 12
        crops2 = C.batch_2d(H, W, diam)
        r, t, wh, pst, tcap = np.stack([c[1] for c in crops2]), np.stack([c[2] for c in crops2]), None, 0, 0
        e6, l6 = C.cloud_3d(1000, 1025, 1.1, 9)
        crops3 = C.batch_3d() + [("second", e6, l6, 1000, 1025, 1.1)]
        thresholds = C.BATCH_THRESHOLDS
    ecap, lcap = 1000, 1025
    p3 = pack_3d(crops3, ecap, lcap)
    sep3 = call_3d(*p3, C.THRESHOLD_3D, w3)
    for thr in thresholds:
        f2, f3 = call_fused(r, t, wh, pst, tcap, diam, thr, w2, *p3, C.THRESHOLD_3D, w3)
        sep2 = call_2d_r(r, t, wh, pst, tcap, diam, thr, w2) if ragged else call_2d(r, t, diam, thr, w2)
        if ragged:
            stats2 += _check_ragged(crops2, pst, diam, thr, *f2, weight=w2)
            for b, (name, rr, _) in enumerate(crops2):
                n = rr.shape[1] * rr.shape[2]
                if n <= pst:
                    _same_bits(f2[1][b, :, :n], sep2[1][b, :, :n], "g_rend of " + name)
        else:
            for b, (name, rr, tt) in enumerate(crops2):
                ref = ref_2d(("batch", H, W, name), rr, tt, diam, thr)
                stats2.append(check_2d("fused %s diam %g thr %g" % (name, diam, thr), ref, f2[0][b], f2[1][b], f2[2][b], diam, w2))
            _same_bits(f2[1], sep2[1], "g_rend")
        _same_bits(f2[0], sep2[0], "loss2d"); _same_bits(f2[2], sep2[2], "nvalid")
        stats3 += _check_batch_3d(crops3, ecap, *f3, weight=w3)
        for k, what in enumerate(("loss3d", "g_est", "g_scale", "npairs")):
            _same_bits(f3[k], sep3[k], what)
    report("fused 2d %s diam %g" % ("ragged" if ragged else "dense", diam), stats2)
    report("fused 3d %s diam %g" % ("ragged" if ragged else "dense", diam), stats3)


# ---- solver --------------------------------------------------------------------------------------------------------------------------------

def _torch_float32_deviation(B, L, p0, seq):
    """for the record only: torch.optim in float32 on the CPU against solver_ref -- what the reference's own arithmetic deviates by"""
    f = np.float32
    lrA, lrS, lrL = float(f(C.LR_ADAM)), float(f(C.LR_SCALE)), float(f(C.LR_LATENT))
    p = p0.astype(np.float64)
    m, v, t = np.zeros((B, 4)), np.zeros((B, 4)), np.zeros(B, np.int64)
    tp, opts = [], []
    for b in range(B):
        q = [torch.tensor(p0[b:b + 1]), torch.tensor(p0[B + 3 * b:B + 3 * b + 3]), torch.tensor(p0[4 * B + b:4 * B + b + 1]),
             torch.tensor(p0[5 * B + b * L:5 * B + (b + 1) * L])]
        tp.append(q)
        opts.append((torch.optim.Adam([{"params": q[0], "lr": C.LR_ADAM}, {"params": q[1], "lr": C.LR_ADAM}], lr=0.03),
                     torch.optim.SGD([{"params": q[2], "lr": C.LR_SCALE}, {"params": q[3], "lr": C.LR_LATENT}], lr=0.01, momentum=0.0)))
    for g, l2, l3, npairs in seq:
        _, stepped = solver_ref(p, g.astype(np.float64), L, l2, l3, npairs, C.W2, C.W3, m, v, t, lrA, lrS, lrL)
        for b in np.nonzero(stepped)[0]:
            q = tp[b]
            q[0].grad = torch.tensor(g[b:b + 1]); q[1].grad = torch.tensor(g[B + 3 * b:B + 3 * b + 3])
            q[2].grad = torch.tensor(g[4 * B + b:4 * B + b + 1]); q[3].grad = torch.tensor(g[5 * B + b * L:5 * B + (b + 1) * L])
            opts[b][0].step(); opts[b][1].step()
    adam = max(np.abs(np.concatenate([tp[b][0].numpy(), tp[b][1].numpy()]) - np.concatenate([p[b:b + 1], p[B + 3 * b:B + 3 * b + 3]])).max()
               for b in range(B))
    tv = np.stack([np.concatenate([opts[b][0].state[tp[b][k]]["exp_avg_sq"].numpy() for k in (0, 1)]) for b in range(B)])
    vrel = (np.abs(tv - v) / np.maximum(np.abs(v), 1e-300))[v > 0].max()
    return adam, vrel


@pytest.mark.parametrize("B,L", C.SOLVER_SIZES)
def test_solver_step_against_the_float64_reference(B, L):
    """200 consecutive sdfr_solver_step calls on one state, gradient magnitudes from 0 to 1e3 across the crops, a random quarter of every
    crop's iterations skipped (npairs -1, NaN loss, zero total).  After every step: stepped and total exact, adam_t = steps taken, a skipped
    crop's parameters / m / v bitwise unchanged, everything within the derived bounds of solver_ref:
      Adam parameters  steps * lr_adam * 1e-5 + 8 ulp(max |p|)   (a float32 beta2 is 0.999 + 1.3e-8, which moves sqrt(1 - beta2^t) by up to
                       6.5e-6 relative at small t; a step is at most lr_adam)
      SGD parameters   2 ulp(max |p|) per step taken (one product, one subtraction)
      m, v             1e-5 relative + 1e-30."""
    Lh = _lib.lib()
    f = np.float32
    p0, mag, seq = C.solver_inputs(B, L)
    lrA, lrS, lrL = float(f(C.LR_ADAM)), float(f(C.LR_SCALE)), float(f(C.LR_LATENT))      # the rates as the C ABI passes them
    n = p0.size
    pr = p0.astype(np.float64)
    mr, vr, tr = np.zeros((B, 4)), np.zeros((B, 4)), np.zeros(B, np.int64)
    pd, md, vd, td = T(p0), torch.zeros(B, 4, device=DEV), torch.zeros(B, 4, device=DEV), torch.zeros(B, dtype=torch.int32, device=DEV)
    crop = np.concatenate([np.arange(B), np.repeat(np.arange(B), 3), np.arange(B), np.repeat(np.arange(B), L)])
    pmax = np.abs(pr)
    p_prev, m_prev, v_prev = p0.copy(), np.zeros((B, 4), f), np.zeros((B, 4), f)
    worst = {"adam": 0.0, "sgd": 0.0, "m": 0.0, "v": 0.0}
    for it, (g, l2, l3, npairs) in enumerate(seq):
        total, stepped = filled((B,)), filled((B,), torch.int32)
        gd, l2d, l3d, npd = T(g), T(l2), T(l3), T(npairs)
        _lib.check(Lh.sdfr_solver_step(_lib.ptr(pd), _lib.ptr(gd), L, _lib.ptr(l2d), _lib.ptr(l3d), _lib.ptr(npd), C.W2, C.W3, _lib.ptr(md),
                                       _lib.ptr(vd), _lib.ptr(td), C.LR_ADAM, C.LR_SCALE, C.LR_LATENT, B, _lib.ptr(total), _lib.ptr(stepped),
                                       _lib.stream_ptr()), "sdfr_solver_step")
        torch.cuda.synchronize()
        tot_ref, st_ref = solver_ref(pr, g.astype(np.float64), L, l2, l3, npairs, C.W2, C.W3, mr, vr, tr, lrA, lrS, lrL)
        p, m, v, t = N(pd), N(md), N(vd), N(td)
        assert np.array_equal(N(stepped), st_ref), it
        assert np.array_equal(N(total), tot_ref, equal_nan=True), (it, "total")
        assert np.array_equal(t, tr), (it, "adam_t is not the number of steps taken")
        sk = st_ref == 0
        assert np.array_equal(bits(p)[sk[crop]], bits(p_prev)[sk[crop]]), (it, "a skipped crop's parameters changed")
        assert np.array_equal(bits(m)[sk], bits(m_prev)[sk]) and np.array_equal(bits(v)[sk], bits(v_prev)[sk]), (it, "a skipped crop's Adam state changed")
        pmax = np.maximum(pmax, np.maximum(np.abs(pr), np.abs(p)))
        ulp = np.spacing(pmax.astype(f)).astype(np.float64)
        steps = tr[crop]
        tol = np.where(np.arange(n) < 4 * B, steps * C.LR_ADAM * 1e-5 + 8 * ulp, 2 * ulp * steps)
        err = np.abs(p - pr)
        assert (err <= tol).all(), (it, "parameter %d (crop %d, |g| ~ %g): %.9g, reference %.9g, bound %.3g"
                                    % (int((err - tol).argmax()), crop[(err - tol).argmax()], mag[crop[(err - tol).argmax()]],
                                       p[(err - tol).argmax()], pr[(err - tol).argmax()], tol[(err - tol).argmax()]))
        for name, got, ref in (("m", m, mr), ("v", v, vr)):
            e = np.abs(got - ref) / (1e-5 * np.abs(ref) + 1e-30)
            assert e.max() <= 1.0, (it, name, "crop %d: %.9g, reference %.9g" % (e.max(1).argmax(), got.reshape(-1)[e.argmax()], ref.reshape(-1)[e.argmax()]))
            worst[name] = max(worst[name], float(e.max()) * 1e-5)
        worst["adam"] = max(worst["adam"], float(err[:4 * B].max()))
        worst["sgd"] = max(worst["sgd"], float((err[4 * B:] / ulp[4 * B:]).max()))
        p_prev, m_prev, v_prev = p, m, v
    assert 0.6 * len(seq) < tr.mean() < 0.9 * len(seq)
    print("\nLOSSTEST solver B %d L %d: Adam parameter error %.3g (bound %.3g + 8 ulp), SGD %.3g ulp, m relative %.3g, v relative %.3g"
          % (B, L, worst["adam"], len(seq) * C.LR_ADAM * 1e-5, worst["sgd"], worst["m"], worst["v"]))
    if (B, L) == (64, 3):
        adam, vrel = _torch_float32_deviation(B, L, p0, seq)
        print("LOSSTEST solver B 64 L 3, for comparison (nothing asserted): torch.optim float32 on the CPU against solver_ref: Adam parameters "
              "%.3g, v relative %.3g" % (adam, vrel))
