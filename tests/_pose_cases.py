"""The cases of the RANSAC pose tests (tests/test_pose_refs_cpu.py, tests/test_gpu_pose_ref.py): generated from seeds and from a few exactly
representable coordinates, a few KB each.  A case is the PACKED input of sdfr_ransac_pose (model / mcls [B][mcap][3], scene / scls
[B][ncap][3] float32, counts, draws or the device sampler's seed and keys, thresholds) plus what its builder knows about it (`expect`).
Every builder checks on the CPU, with the references of tests/_pose_ref.py, that its case does what it was made for.
"""
import functools
import itertools

import numpy as np

from . import _pose_ref as PR

f32, f64 = np.float32, np.float64
FAIL = (3.0, 3.0, 3.0)              # a scene colour far from every model colour: fails the gate
FAR = (40.0, 40.0, 40.0)            # where filler points live: far from everything that is scored


def pack(name, crops, T, typ, f16=False, idx=None, seed=0, keys=None, metric_thr=0.15, nocs_thr=0.15, scale_model=1.0, expect=None):
    """crops: list of (model, mcls, scene, scls); idx: list of [T][4] draws per crop, or None for the device sampler"""
    B = len(crops)
    mcap, ncap = max(1, max(len(c[0]) for c in crops)), max(1, max(len(c[2]) for c in crops))
    z = lambda cap: np.zeros((B, cap, 3), f32)
    model, mcls, scene, scls = z(mcap), z(mcap), z(ncap), z(ncap)
    for b, (m, mc, s, sc) in enumerate(crops):
        m, mc, s, sc = (np.asarray(a, f64).reshape(-1, 3) for a in (m, mc, s, sc))
        for a in (m, mc, s, sc):
            fin = np.isfinite(a)
            assert np.array_equal(a[fin].astype(f32).astype(f64), a[fin]), name + ": a coordinate is not a float32"
        if f16:
            assert np.array_equal(m.astype(np.float16).astype(f64), m), name + ": a model coordinate is not a float16"
        model[b, :len(m)], mcls[b, :len(m)], scene[b, :len(s)], scls[b, :len(s)] = m, mc, s, sc
    return dict(name=name, B=B, T=T, type=typ, f16=bool(f16), seed=int(seed), keys=np.arange(B, dtype=np.int64) if keys is None else np.asarray(keys, np.int64),
                metric_thr=float(metric_thr), nocs_thr=float(nocs_thr), scale_model=float(scale_model),
                mcnt=np.array([len(c[0]) for c in crops], np.int32), ncnt=np.array([len(c[2]) for c in crops], np.int32),
                model=model, mcls=mcls, scene=scene, scls=scls, idx=None if idx is None else np.asarray(idx, np.int32).reshape(B, T, 4),
                expect=expect or [{} for _ in crops])


def colours(n, first=0):
    """n distinct model colours on a 1/16 lattice in (0, 1]^3 (exact in float16), more than 0.06 apart"""
    k = np.arange(first, first + n)
    return np.stack([(k % 16 + 1) / 16.0, ((k // 16) % 16 + 1) / 16.0, (k // 256 + 1) / 16.0], 1)


# ---- random crops -------------------------------------------------------------------------------------------------------------------------

def rand_crop(rng, N, M, typ, f16=False, colour_outliers=0.5, clutter=0.5):
    """a car-sized ellipsoid of M model points with NOCS-like colours; N scene points: all but `clutter` of them model points under a yaw, a scale of 2
    and a translation with a little noise, the rest uniform clutter; `colour_outliers` of all colours are clutter too"""
    v = rng.normal(size=(M, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    m = (v * np.array([0.5, 0.2, 0.25])).astype(np.float16 if f16 else f32).astype(f64)
    mc = (v * 0.5 + 0.5).astype(np.float16 if f16 else f32).astype(f64)
    if typ == 0:
        m = (m * 2.0).astype(np.float16 if f16 else f32).astype(f64)     # 'kabsch' fits the model at its metric size
    yaw = rng.uniform(-np.pi, np.pi)
    c, s = np.cos(yaw), np.sin(yaw)
    R = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    n_out = int(N * clutter)
    n_in = N - n_out
    sel = rng.integers(0, M, n_in)
    p = ((2.0 if typ == 1 else 1.0) * (R @ m[sel].T).T) + np.array([0.2, 0.1, 8.0]) + rng.normal(0, 0.005, (n_in, 3))
    col = mc[sel] + rng.normal(0, 0.01, (n_in, 3))
    po = rng.uniform(p.min(0) - 0.5, p.max(0) + 0.5, (n_out, 3))
    co = rng.uniform(0, 1, (n_out, 3))
    sc = np.concatenate([col, co])
    bad = rng.random(N) < colour_outliers
    sc[bad] = rng.uniform(1.5, 2.5, (int(bad.sum()), 3))
    order = rng.permutation(N)
    return m, mc, np.concatenate([p, po])[order].astype(f32).astype(f64), sc[order].astype(f32).astype(f64)


def shape_cases():
    """T x N x M at the edges of a workgroup (256), of a hypothesis group (8) and of an LDS tile (256); the device sampler draws"""
    out = []
    # name, T, N, M, type, float16 model, colour outliers, clutter, seed offset (chosen so that every case scores at least one hypothesis)
    spec = [("edge_T1", 1, 5, 2, 0, False, 0.0, 0.0, 0), ("edge_T7", 7, 255, 255, 1, False, 0.1, 0.5, 0), ("edge_T8", 8, 256, 256, 1, False, 0.1, 0.5, 3),
            ("edge_T9", 9, 257, 257, 0, True, 0.2, 0.5, 0), ("edge_T255", 255, 5, 1, 0, False, 0.0, 0.0, 0), ("edge_T256", 256, 24, 2, 0, True, 0.0, 0.25, 0),
            ("edge_T257", 257, 513, 600, 0, False, 0.6, 0.5, 6), ("edge_T567", 567, 40, 30, 1, False, 0.3, 0.5, 7)]
    for name, T, N, M, typ, f16, co, cl, sd in spec:
        rng = np.random.default_rng(100 + sd)
        out.append(pack(name, [rand_crop(rng, N, M, typ, f16, co, cl)], T, typ, f16, seed=77 + sd, keys=[5]))
    rng = np.random.default_rng(200)
    out.append(pack("ragged", [rand_crop(rng, 5, 1, 0, False, 0.0, 0.0), rand_crop(rng, 513, 600, 0, False, 0.6), rand_crop(rng, 40, 7, 0, False, 0.2)], 64, 0,
                    seed=3, keys=[11, 1 << 40, 7]))
    for k, (typ, f16) in enumerate(((0, False), (1, False), (0, True))):
        rng = np.random.default_rng(300 + k)
        out.append(pack("random_%d" % k, [rand_crop(rng, 400 - 57 * k, 400 - 131 * k, typ, f16, 0.3)], 64, typ, f16, seed=9 + k, keys=[100 + k],
                        scale_model=2.0))
    return out


def nonfinite_pair(typ=0):
    """the same crop twice: scene point 7, a far outlier with a passing colour, finite and NaN (and point 8 infinite); draws 0 and 1 sample it"""
    rng = np.random.default_rng(400)
    m, mc, s, sc = rand_crop(rng, 60, 50, typ, False, 0.2)
    T = 32
    idx = np.stack([rng.choice(60, 4, replace=False) for _ in range(T)]).astype(np.int32)
    idx[idx == 7] = 9
    idx[idx == 8] = 10
    good = np.flatnonzero(PR.colour_nn(mc.astype(f32), sc.astype(f32))[1] <= 0.15)
    good = good[(good != 7) & (good != 8)]
    sc[7], sc[8] = sc[good[0]], sc[good[1]]
    s[7], s[8] = (90.0, 90.0, 90.0), (-90.0, 95.0, 90.0)
    idx[0], idx[1] = (7, good[0], good[1], good[2]), (good[3], 8, good[1], good[0])
    tag = "nonfinite" + ("_p" if typ else "")
    clean = pack(tag + "_clean", [(m, mc, s, sc)], T, typ, idx=[idx])
    s2 = s.copy()
    s2[7], s2[8] = (np.nan, 90.0, 90.0), (-90.0, np.inf, 90.0)
    return clean, pack(tag, [(m, mc, s2, sc)], T, typ, idx=[idx])


# ---- crafted samples ----------------------------------------------------------------------------------------------------------------------

RZ = np.array([[0.6, -0.8, 0.0], [0.8, 0.6, 0.0], [0.0, 0.0, 1.0]])        # exact on multiples of 5/8
RX = np.array([[1.0, 0.0, 0.0], [0.0, 0.6, -0.8], [0.0, 0.8, 0.6]])


def rot(R, pts):
    """R @ pts with the exact arithmetic the cases rely on: 5 R is an integer matrix and the coordinates are multiples of 5/8"""
    return (np.rint(5.0 * R) @ np.asarray(pts, f64).T).T / 5.0


TETRA = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], f64)


def sample_crop(frm, to, same_colour=False):
    """a crop whose draw (0, 1, 2, 3) is the sample frm -> to: scene = frm + 2 fillers (failing colours), model = to + 2 fillers"""
    mc = colours(6)
    model = np.concatenate([to, np.array([FAR, FAR]) + [[0, 0, 0], [1, 0, 0]]])
    scene = np.concatenate([frm, np.array([FAR, FAR]) + [[0, 1, 0], [0, 0, 1]]])
    sc = np.concatenate([mc[[0, 0, 0, 0]] if same_colour else mc[:4], [FAIL, FAIL]])
    return model, mc, scene, sc


DRAWS4 = [(0, 1, 2, 3), (3, 2, 1, 0), (0, 1, 2, 4), (1, 5, 3, 2)]


def det_v(frm, to, typ, f16):
    info = {}
    mf, mt, H, sig = PR.sample_moments(np.asarray(frm, f32), np.asarray(to, f32), f16)
    with np.errstate(all="ignore"):
        PR.rs_fit(H, mf, mt, sig, typ, info)
    return info["detV"]


def axes(frm, to, typ, f16, want_negative):
    """the same sample with its coordinate axes permuted so that the Jacobi solver's V comes out improper (det V < 0: the sorting of the
    eigenvalues is an odd permutation) or proper, as wanted; the builder's check that the branch is taken"""
    for p in itertools.permutations(range(3)):
        f, t = frm[:, p], to[:, p]
        if (det_v(f, t, typ, f16) < 0) == want_negative:
            return f, t, list(p)
    raise AssertionError("no axis order gives det V %s 0" % ("<" if want_negative else ">="))


def crafted_case(typ, f16):
    c = 2.0 if typ == 1 else 1.0
    t0 = np.array([0.25, -0.5, 1.0])
    crops, expect = [], []

    def add(kind, frm, to, **kw):
        crops.append(sample_crop(frm, to, same_colour=kw.pop("same_colour", False)))
        expect.append(dict(kind=kind, **kw))

    gen = 0.625 * np.array([[1, 0, 0], [0, 2, 0], [0, 0, 3], [-1, -1, -1]], f64) + np.array([1.25, 0.625, 2.5])
    for kind, neg in (("well", False), ("well_negV", True)):
        f, t, p = axes(gen, c * rot(RZ, gen) + t0, typ, f16, neg)
        add(kind, f, t, R=RZ[np.ix_(p, p)], c=c, t=t0[p], admitted=True, detV_negative=neg)
    mirror = np.diag([1.0, 1.0, -1.0])
    f, t, p = axes(gen, c * rot(RZ @ mirror, gen) + t0, typ, f16, True)
    add("reflection", f, t, admitted=True, detV_negative=True)
    flat = 0.625 * np.array([[1, 0, 0], [-1, 2, 0], [0, -3, 0], [2, 1, 0]], f64) + np.array([1.25, 0.625, 2.5])
    add("coplanar", flat, c * rot(RX, flat) + t0, R=RX, c=c, t=t0, admitted=True)
    # nearly collinear, still admitted (gap about 5e-3): where squaring H into H^T H costs the most digits
    thin = 0.625 * np.array([[-3, 0.125, 0], [-1, -0.125, 0.125], [1, -0.125, -0.125], [3, 0.125, 0]], f64) + np.array([1.25, 0.625, 2.5])
    add("thin", thin, c * rot(RZ, thin) + t0, R=RZ, c=c, t=t0, admitted=True)
    line = np.array([[k, 0, 0] for k in (-3.0, -1.0, 1.0, 3.0)]) + np.array([1.0, 2.0, 3.0])
    add("collinear_axis", line, c * line + t0, dir_from=[1.0, 0.0, 0.0], dir_to=[1.0, 0.0, 0.0])
    skew = 0.625 * np.array([[k, 2 * k, 2 * k] for k in (-3.0, -1.0, 1.0, 3.0)]) + np.array([1.25, 0.625, 2.5])
    add("collinear_skew", skew, c * rot(RZ, skew) + t0, dir_from=[1 / 3, 2 / 3, 2 / 3], dir_to=list(RZ @ np.array([1 / 3, 2 / 3, 2 / 3])))
    add("h0", gen, c * rot(RZ, gen) + t0, same_colour=True)
    if typ == 1:
        e_thr = np.sqrt(5.0 * 3.0 * PR.EPS32)            # sum y^2 / sum x^2 = e^2 / 5 at the rank rule's threshold
        for kind, fac in (("rank_below", 0.97), ("rank_above", 1.03)):
            e = float(f64(e_thr * fac).astype(np.float16))
            pts = np.array([[-3.0, e, 0.0], [-1.0, -e, 0.0], [1.0, -e, 0.0], [3.0, e, 0.0]])
            add(kind, pts, pts)
        d = 2.0 ** -8 if f16 else 2.0 ** -20
        add("c_below", TETRA, (3.0 - d) * TETRA, c=3.0 - d)
        add("c_above", TETRA, (3.0 + d) * TETRA, c=3.0 + d)
    f, t, p = axes(gen, c * rot(RZ, gen) + t0, typ, f16, False)
    add("oob", f, t)
    idx = [list(DRAWS4) for _ in crops]
    idx[-1] = [(0, 1, 2, 3), (0, 1, 2, 6), (-1, 1, 2, 3), (3, 2, 1, 0)]
    case = pack("crafted_%s%d" % ("kp"[typ], 16 if f16 else 32), crops, 4, typ, f16, idx=idx, expect=expect)
    # the builder's checks, by reference (a)
    for b, ex in enumerate(expect):
        fit = PR.fit_mp(case["scene"][b, :4], case["model"][b, :4] if ex["kind"] != "h0" else case["model"][b, [0, 0, 0, 0]], typ, False, f16)
        ex["fit"] = fit
        if ex.get("admitted"):
            assert fit["gap"] >= 1e-3, (case["name"], ex["kind"], fit["gap"])
            if "R" in ex:
                assert np.abs(fit["R"] - ex["R"]).max() < 1e-15 and abs(fit["c"] - ex["c"]) < 1e-15 and np.abs(fit["t"] - ex["t"]).max() < 1e-15
        if ex["kind"] == "reflection":
            assert fit["sign"] == -1
        if ex["kind"].startswith("collinear"):
            assert fit["rank"] == 1
        if ex["kind"] == "rank_below":
            assert fit["rank"] == 1 and fit["rank_margin"] < -1e-2 * 3 * PR.EPS32
        if ex["kind"] == "rank_above":
            assert fit["rank"] == 2 and fit["rank_margin"] > 1e-2 * 3 * PR.EPS32
        if ex["kind"] == "c_below":
            assert f32(fit["c"]) < f32(3.0) and fit["c_mp"] < 3
        if ex["kind"] == "c_above":
            assert f32(fit["c"]) > f32(3.0)
    return case


# ---- the identity sample: ties, thresholds, select ------------------------------------------------------------------------------------------

CROSS = np.array([[3.0, 3.0, 4.0], [1.0, 3.0, 4.0], [2.0, 4.0, 4.0], [2.0, 2.0, 4.0]])
# scene cross == model cross: H = diag(2, 2, 0), the solver does not rotate, R = I, c = 1 and t = 0 EXACTLY, for both fits and both dtypes:
# a scene point's transformed position is the point itself, so exact ties and exact threshold distances can be placed.


def ident_crop(model_extra=(), mcls_extra=(), scene_extra=(), scls_extra=(), fail_points=1):
    """model: the cross (colours 0..3 of the lattice) + extras; scene: the cross + extras + `fail_points` fillers with a failing colour"""
    mc = colours(4)
    model = np.concatenate([CROSS, np.asarray(model_extra, f64).reshape(-1, 3)])
    mcls = np.concatenate([mc, np.asarray(mcls_extra, f64).reshape(-1, 3)])
    scene = np.concatenate([CROSS, np.asarray(scene_extra, f64).reshape(-1, 3), np.array([FAR]) + np.arange(fail_points)[:, None] * [1.0, 0, 0]])
    scls = np.concatenate([mc, np.asarray(scls_extra, f64).reshape(-1, 3), np.tile(np.array([FAIL]), (fail_points, 1))])
    return model, mcls, scene, scls


def counts_case():
    """B = 4 crops with exactly 0, 1, 8 and 9 passing hypotheses of T = 16 (the RS_HG = 8 group edge of the scoring kernel)"""
    perms = list(itertools.permutations(range(4)))
    crops, idx, expect = [], [], []
    for n_pass in (0, 1, 8, 9):
        crops.append(ident_crop())
        fail_at = 4                                      # the filler's index
        draws = [(0, 1, 2, fail_at)] * 16
        where = [2, 15, 0, 7, 8, 9, 3, 11, 5][:n_pass]
        for k, t in enumerate(sorted(where)):
            draws[t] = perms[k]
        idx.append(draws)
        expect.append(dict(kind="pass_%d" % n_pass, pcount=n_pass, plist=sorted(where)))
    return pack("pass_counts", crops, 16, 0, idx=idx, expect=expect)


def tie_case(typ=0, f16=False):
    c = colours(40)
    far = lambda k: np.array(FAR) + [0.0, 0.0, float(k)]
    # crop 0, colour ties: duplicate colours at (5, 9) and across the tile edge at (255, 256); a scene colour exactly between two colours
    M = 258
    mcls = colours(M)
    mcls[9], mcls[256] = mcls[5], mcls[255]
    mcls[20], mcls[21] = (0.25, 0.03125, 2.0), (0.75, 0.03125, 2.0)          # (off the lattice: nothing else is as near as these two)
    mcls[30], mcls[31] = (0.75, 0.96875, 2.0), (0.25, 0.96875, 2.0)
    model = np.array([far(k) for k in range(M)])
    model[:4] = CROSS
    scls_x = [mcls[5], mcls[255], (0.5, 0.03125, 2.0), (0.5, 0.96875, 2.0)]
    crop0 = (model, mcls, np.concatenate([CROSS, [far(300 + k) for k in range(5)]]), np.concatenate([mcls[:4], scls_x, [FAIL]]))
    ex0 = dict(kind="tie_colour", cnn={4: 5, 5: 255, 6: 20, 7: 30})
    # crop 1, scoring ties: duplicate model POINTS with different colours, within a tile (10, 11) / (12, 13) and across tiles (14, 290);
    # a scene point exactly between two lattice points (16, 17) / (18, 19).  The first index decides, its colour makes the inlier.
    M = 300
    model = np.array([far(k) for k in range(M)])
    mcls = colours(M)
    model[:4] = CROSS
    P, Q, S, L = np.array([6.0, 6.0, 6.0]), np.array([7.0, 6.0, 6.0]), np.array([8.0, 6.0, 6.0]), np.array([5.0, 5.0, 5.0])
    model[10], model[11], model[12], model[13], model[14], model[290] = P, P, Q, Q, S, S
    model[16], model[17], model[18], model[19] = L, L + [0.25, 0, 0], L + [0.25, 1, 0], L + [0, 1, 0]
    good = np.array([0.5, 0.5, 0.96875])
    mcls[10], mcls[13], mcls[14], mcls[16], mcls[19] = good, good + [0.0625, 0, 0], good + [0, 0.0625, 0], good + [0.0625, 0.0625, 0], good + [0.125, 0, 0]
    scene_x = [P, Q, S, L + [0.125, 0, 0], L + [0.125, 1, 0]]
    scls_x = [mcls[10], mcls[13], mcls[14], mcls[16], mcls[19]]
    crop1 = (model, mcls, np.concatenate([CROSS, scene_x, [far(400)]]), np.concatenate([colours(4), scls_x, [FAIL]]))
    # P -> 10 (its colour: in); Q -> 12 (another colour: out although 13 matches); S -> 14 (in, 290 does not match);
    # L + 1/8 -> 16 (in); L + (1/8, 1) -> 18 (out although 19 matches)
    ex1 = dict(kind="tie_score", mask={4: 1, 5: 0, 6: 1, 7: 1, 8: 0}, n_inliers=7)
    idx = [[(0, 1, 2, 3), (1, 0, 3, 2), (0, 1, 2, len(crop0[2]) - 1), (0, 1, 3, 2)], [(0, 1, 2, 3), (1, 0, 3, 2), (0, 1, 2, len(crop1[2]) - 1), (0, 1, 3, 2)]]
    return pack("ties_%s%d" % ("kp"[typ], 16 if f16 else 32), [crop0, crop1], 4, typ, f16, idx=idx, expect=[ex0, ex1])


def select_case():
    """T = 264.  Sample A (the cross, 7 inliers) and sample B (a second cross, shifted in the scene: its hypothesis moves everything else
    away, 4 inliers).  crop 0: A at t = 3 and t = 260 (lanes 3 and 4 of the stride loop); crop 1: A at t = 3, 259 and 260 (259 is lane 3's
    second trip); crop 2: A at the last t only.  B elsewhere; every other draw fails the gate."""
    mcB = colours(4, first=8)
    crossB = CROSS + [0.0, 0.0, 6.0]
    extra_m = np.concatenate([crossB, [[9.0, 9.0, 9.0], [9.0, 10.0, 9.0], [10.0, 9.0, 9.0]]])
    extra_mc = np.concatenate([mcB, colours(3, first=16)])
    extra_s = np.concatenate([crossB + [10.0, 0.0, 0.0], extra_m[4:]])
    crop = ident_crop(extra_m, extra_mc, extra_s, extra_mc)
    A, Bd, F = (0, 1, 2, 3), (4, 5, 6, 7), (0, 1, 2, 11)
    T = 264
    crops, idx, expect = [], [], []
    for a_at, b_at in (((3, 260), (1, 100, 261)), ((3, 259, 260), (2, 4, 263)), ((263,), (0, 5, 262))):
        d = [F] * T
        for t in a_at:
            d[t] = A
        for t in b_at:
            d[t] = Bd
        crops.append(crop)
        idx.append(d)
        expect.append(dict(kind="select", best=a_at[0], n_inliers=7, count_b=4, a_at=a_at, b_at=b_at))
    return pack("select_ties", crops, T, 0, idx=idx, expect=expect)


D_METRIC = 0.15625


def metric_dz():
    """the smallest float32 dz with sqrt(D^2 + 0 + dz^2) == D + 1 ulp in float64"""
    target = np.nextafter(f64(D_METRIC), f64(1.0))
    dz = f32(2.0e-9)
    while True:
        z = f64(dz)
        d = np.sqrt(f64(D_METRIC) * f64(D_METRIC) + f64(0.0) * f64(0.0) + z * z)
        if d == target:
            return float(dz)
        assert d < target
        dz = np.nextafter(dz, f32(1.0))


def threshold_cases():
    out = []
    D, D1 = D_METRIC, float(np.nextafter(f64(D_METRIC), f64(1.0)))
    D2 = float(np.nextafter(f64(D1), f64(1.0)))
    cx = colours(1, first=20)
    pm = [7.0, 7.0, 0.0]
    for name, thr, m4, m5 in (("metric_at", D, 0, 0), ("metric_up1", D1, 1, 0), ("metric_up2", D2, 1, 1)):
        crop = ident_crop([pm], cx, [[7.0 + D, 7.0, 0.0], [7.0 + D, 7.0, metric_dz()]], [cx[0], cx[0]])
        out.append(pack(name, [crop], 4, 0, idx=[list(DRAWS4[:2]) + [(0, 1, 2, 6), (3, 1, 6, 2)]], metric_thr=thr,
                        expect=[dict(kind="metric", mask={4: m4, 5: m5}, n_inliers=4 + m4 + m5)]))
    t32 = f32(0.15)
    lo, hi = np.nextafter(t32, f32(0)), np.nextafter(t32, f32(1))
    pc = [9.0, 9.0, 0.0]
    col = ident_crop([pc], [[0.0, 0.0, 0.0]], [pc, pc, pc], [[float(lo), 0, 0], [float(t32), 0, 0], [float(hi), 0, 0]])
    four = ident_crop()
    five = ident_crop([pc], cx, [pc], cx)
    out.append(pack("thresholds", [col, four, five], 4, 0, idx=[list(DRAWS4[:2]) + [(0, 1, 2, 7), (3, 1, 7, 2)], list(DRAWS4[:2]) + [(0, 1, 2, 4), (4, 1, 3, 2)],
                                                                list(DRAWS4[:2]) + [(0, 1, 2, 5), (5, 1, 3, 2)]],
                    expect=[dict(kind="colour_thr", mask={4: 1, 5: 0, 6: 0}, n_inliers=5, found=1), dict(kind="count4", n_inliers=4, found=0),
                            dict(kind="count5", n_inliers=5, found=1)]))
    # final fit rank-deficient (procrustes): a far-coloured copy of every cross point sits at a lower index, so the scoring search lands on
    # it and the 4 sampled points are NOT inliers; the 6 inliers lie on a line along x, and so do their colour-NN model points
    line = np.array([[20.0 + k, 5.0, 5.0] for k in range(6)])
    lc = colours(6, first=24)
    model = np.concatenate([CROSS, CROSS, line])
    mcls = np.concatenate([colours(4, first=40) + [0.0, 0.0, 0.5], colours(4), lc])
    scene = np.concatenate([CROSS, line, [FAR]])
    scls = np.concatenate([colours(4), lc, [FAIL]])
    out.append(pack("final_deficient", [(model, mcls, scene, scls)], 4, 1, idx=[list(DRAWS4[:2]) + [(0, 1, 2, 10), (10, 1, 3, 2)]],
                    expect=[dict(kind="final_deficient", n_inliers=6, found=0, best=0)]))
    return out


# (the names alone, so that collecting the tests builds nothing)
CASE_NAMES = ("edge_T1", "edge_T7", "edge_T8", "edge_T9", "edge_T255", "edge_T256", "edge_T257", "edge_T567", "ragged", "random_0", "random_1", "random_2",
              "pass_counts", "select_ties", "metric_at", "metric_up1", "metric_up2", "thresholds", "final_deficient", "nonfinite_clean", "nonfinite", "nonfinite_p_clean", "nonfinite_p",
              "crafted_k32", "ties_k32", "crafted_k16", "ties_k16", "crafted_p32", "ties_p32", "crafted_p16", "ties_p16")


@functools.lru_cache(maxsize=None)
def all_cases():
    """name -> case, every case of the suite"""
    cases = shape_cases() + [counts_case(), select_case()] + threshold_cases() + list(nonfinite_pair(0)) + list(nonfinite_pair(1))
    for typ in (0, 1):
        for f16 in (False, True):
            cases += [crafted_case(typ, f16), tie_case(typ, f16)]
    out = {c["name"]: c for c in cases}
    assert tuple(out) == CASE_NAMES
    return out


@functools.lru_cache(maxsize=None)
def restated(name):
    """restatement (b) of a case, computed once"""
    return PR.restate(all_cases()[name])


def crop_alone(case, b):
    """crop b of a case as a case of its own (capacities shrunk to the crop's own counts)"""
    N, M = int(case["ncnt"][b]), int(case["mcnt"][b])
    sl = lambda a, n: a[b:b + 1, :max(n, 1)].copy()
    one = dict(case, B=1, name="%s[%d]" % (case["name"], b), keys=case["keys"][b:b + 1], mcnt=case["mcnt"][b:b + 1], ncnt=case["ncnt"][b:b + 1],
               model=sl(case["model"], M), mcls=sl(case["mcls"], M), scene=sl(case["scene"], N), scls=sl(case["scls"], N),
               idx=None if case["idx"] is None else case["idx"][b:b + 1], expect=case["expect"][b:b + 1])
    return one
