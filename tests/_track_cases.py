"""Cases of the joint fit's tests (tests/test_track_cpu.py runs the host program on them, tests/test_gpu_track.py the kernel): the smallest
shapes at which each rule of sdfr_track_step can go wrong.  T 1 and 3; views per track 1 / 1, 2, 5 / 0, 3 / 1024 / 1025; L 3, 8, 40, 256;
unit 0 / 1; t 1 and 7; share_scale 0 / 1; weights NULL, given, one zero, one NaN; each flag that keeps a view out; a non-finite entry in a
latent and in a pose column; a scale step that would end non-positive; each rate 0; broken voff entries.  Built with numpy on the CPU;
arrays are read-only.
"""
import functools

import numpy as np

from tests import _align_cases as AC
from tests import _align_ref as AR
from tests import _track_ref as TR

RATES = (1e-2, 2e-2, 5e-3, 1e-2, 3e-2)
BROKEN_VOFF = ((0, -4, 3, 8), (0, 3, 2, 2), (0, 3, 3, 99), (0, 1 << 40, 1 << 41, 1 << 42), (2, 1, 9, 8))


def step_cases():
    """(views, L, unit, t, share, weights, special).  views: the tracks' view counts, or with special "voff<i>" the table BROKEN_VOFF[i] over
    8 views.  weights: None | "given" | "zero" | "nan" (the second view of the call, or its only one).  special: None | "flag1" "flag2"
    "flag8" "flag16" (that flag on the hit view) | "nan_latent" | "inf_pose" | "big_latent" (1e300: float32 overflows) | "neg_scale" |
    "track_overflow" (z = 0 with a gradient near float32's largest: the walk is not finite though every entry is) | "all_bad" (every view
    of the second track flagged) | "lr0" | "pose0" .. "pose4" (that rate 0) | "frozen" (every rate 0) | "minus_zero"."""
    cases = [((1,), 3, 1, 1, 0, None, None), ((1,), 3, 1, 1, 1, None, None), ((1, 2, 5), 8, 1, 7, 1, "given", None), ((1, 2, 5), 8, 0, 7, 0, "given", None),
             ((0, 3), 8, 0, 7, 1, None, None), ((1024,), 3, 1, 1, 1, "given", None), ((1025,), 3, 1, 1, 1, None, None), ((1, 2, 5), 40, 1, 1, 0, "zero", None),
             ((1, 2, 5), 256, 0, 7, 1, "nan", None), ((1, 2, 5), 256, 1, 1, 0, None, None)]
    cases += [((1, 2, 5), 8, 1, 7, i % 2, None, "flag%d" % f) for i, f in enumerate((1, 2, 8, 16))]
    cases += [((1, 2, 5), 8, 1, 7, 1, "given", "nan_latent"), ((1, 2, 5), 8, 0, 1, 0, None, "inf_pose"), ((1, 2, 5), 3, 1, 7, 1, None, "big_latent"),
              ((1, 2, 5), 8, 1, 7, 1, None, "neg_scale"), ((1, 2, 5), 8, 1, 7, 0, None, "neg_scale"), ((1, 2, 5), 8, 1, 1, 1, None, "track_overflow"),
              ((1, 2, 5), 8, 1, 7, 0, "given", "all_bad")]
    cases += [((1, 2, 5), 8, u, 7, s, None, r) for u, s, r in ((1, 1, "lr0"), (0, 0, "pose0"), (1, 1, "pose1"), (1, 0, "pose2"), (1, 1, "pose3"), (1, 1, "pose4"),
                                                                (1, 0, "pose4"), (1, 1, "frozen"))]
    cases += [((0, 0, 0), 8, 1, 7, i % 2, "given", "voff%d" % i) for i in range(len(BROKEN_VOFF))]
    cases += [((1,), 8, 0, 1, 1, None, "minus_zero"), ((1,), 8, 1, 1, 0, None, "minus_zero")]
    return cases


def case_id(c):
    return "v%s_L%d_u%d_t%d_s%d_%s_%s" % ("-".join(map(str, c[0])), c[1], c[2], c[3], c[4], c[5], c[6])


def hit_view(voff):
    """the view the special of a case is planted on: the second view of the first track with two or more, else view 0"""
    for t in range(len(voff) - 1):
        if voff[t + 1] - voff[t] >= 2:
            return int(voff[t]) + 1
    return 0


@functools.lru_cache(maxsize=None)
def step_case(views, L, unit, t, share, weights, special):
    """a dict of sdfr_track_step's arrays and scalars: z m v scale sm sv voff weight theta tm tv pose z_view g view_loss vflags loss tflags
    (what the outputs hold before the call) code_reg lr lr_pose; share and unit as given"""
    special = special or ""
    if special.startswith("voff"):
        voff = np.array(BROKEN_VOFF[int(special[4:])], np.int64)
        V = 8
    else:
        voff = np.concatenate([[0], np.cumsum(views)]).astype(np.int64)
        V = int(voff[-1])
    T = len(voff) - 1
    rng = np.random.default_rng(9900 + 31 * t + 7 * V + L + 3 * share)
    z = (0.1 * rng.standard_normal((T, L))).astype(np.float32)
    old = t > 1
    m = (1e-3 * rng.standard_normal((T, L))).astype(np.float32) if old else np.zeros((T, L), np.float32)
    v = (1e-6 * rng.uniform(0, 1, (T, L))).astype(np.float32) if old else np.zeros((T, L), np.float32)
    scale = rng.uniform(1.2, 2.4, T).astype(np.float32)
    sm = (1e-3 * rng.standard_normal(T)).astype(np.float32) if old else np.zeros((T,), np.float32)
    sv = (1e-6 * rng.uniform(0, 1, T)).astype(np.float32) if old else np.zeros((T,), np.float32)
    theta, _ = AC.random_poses(rng, V)
    tm = (1e-3 * rng.standard_normal((V, 5))).astype(np.float32) if old else np.zeros((V, 5), np.float32)
    tv = (1e-6 * rng.uniform(0, 1, (V, 5))).astype(np.float32) if old else np.zeros((V, 5), np.float32)
    g = np.concatenate([0.02 * rng.standard_normal((V, L)), 0.05 * rng.standard_normal((V, 5))], 1)
    view_loss = rng.uniform(0.01, 0.05, V)
    vflags = np.zeros((V,), np.int32)
    z_view = rng.standard_normal((V, L)).astype(np.float32)               # stale on purpose: a stepped track overwrites it
    weight = None
    hit = hit_view(voff) if not special.startswith("voff") else 1
    if weights is not None:
        weight = rng.uniform(0.5, 2.0, V).astype(np.float32)
        if weights == "zero":
            weight[hit] = 0
        if weights == "nan":
            weight[hit] = np.nan
    lr, lr_pose = 5e-3, list(RATES)
    well_formed = not special.startswith("voff") and TR.count(voff, 0, V) >= 0 and max(views) <= TR.MAX_VIEWS
    own = TR.track_of(voff) if well_formed else np.zeros((V,), np.int64)
    if share and well_formed:
        theta[:, 4] = scale[own]
    if special.startswith("flag"):
        vflags[hit] = int(special[4:])
    elif special == "nan_latent":
        g[hit, 1] = np.nan
    elif special == "inf_pose":
        g[hit, L + 2] = np.inf
    elif special == "big_latent":
        g[hit, 0] = 1e300
    elif special == "neg_scale":
        tr = own[hit]
        if share:
            scale[tr], sm[tr], theta[own == tr, 4], g[own == tr, L + 4] = 1e-3, 1.0, 1e-3, 5.0
        else:
            theta[hit, 4], tm[hit, 4], g[hit, L + 4] = 1e-3, 1.0, 5.0
    elif special == "track_overflow":
        tr = own[hit]
        z[tr] = 0
        g[own == tr, 0] = 3e38
    elif special == "all_bad":
        vflags[own == 1] = 2
    elif special == "lr0":
        lr = 0.0
    elif special.startswith("pose"):
        lr_pose[int(special[4:])] = 0.0
    elif special == "frozen":
        lr, lr_pose = 0.0, [0.0] * 5
    elif special == "minus_zero":
        g[0, 0:L:2] = -0.0
        g[0, L + 4] = -0.0
    pose = AR.pose_row(theta)
    loss = np.full((T,), -3.5, np.float64)
    tflags = np.full((T,), 0x5A5A, np.int32)
    out = dict(z=z, m=m, v=v, scale=scale, sm=sm, sv=sv, voff=voff, theta=theta, tm=tm, tv=tv, pose=pose, z_view=z_view, g=g, view_loss=view_loss,
               vflags=vflags, loss=loss, tflags=tflags)
    for a in out.values():
        a.setflags(write=False)
    if weight is not None:
        weight.setflags(write=False)
    out.update(weight=weight, code_reg=1e-4, lr=lr, lr_pose=tuple(lr_pose), share=share, unit=unit, t=t, L=L, T=T, V=V)
    return out


def restate(c):
    """_track_ref.step on a case dict"""
    return TR.step(c["z"], c["m"], c["v"], c["scale"], c["sm"], c["sv"], c["share"], c["voff"], c["weight"], c["theta"], c["tm"], c["tv"], c["pose"],
                   c["z_view"], c["g"], c["view_loss"], c["vflags"], c["unit"], c["code_reg"], c["lr"], c["lr_pose"], c["t"], loss=c["loss"],
                   tflags=c["tflags"])


def same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def check_step_case(case, want):
    """what each case was built to show, on the restatement's result"""
    views, L, unit, t, share, weights, special = case
    c = step_case(*case)
    special = special or ""
    voff, V, T = c["voff"], c["V"], c["T"]
    before = {k: c[k] for k in ("z", "m", "v", "scale", "sm", "sv", "theta", "tm", "tv", "pose", "z_view", "loss")}
    if special.startswith("voff") or max(views) > TR.MAX_VIEWS:
        bad = [TR.count(voff, tr, V) < 0 for tr in range(T)]
        assert any(bad) and [bool(f == TR.BAD_TABLE) for f in want["tflags"]] == bad
        for tr in np.nonzero(bad)[0]:
            assert same(want["loss"][tr], c["loss"][tr]) and same(want["z"][tr], c["z"][tr])
        if all(bad):
            for k, a in before.items():
                assert same(want[k], a), k
            assert same(want["vflags"], c["vflags"])
        return
    own, hit = TR.track_of(voff), hit_view(voff)
    skipped_v = (want["vflags"] & TR.SKIPPED) != 0
    stepped = want["tflags"] == 0
    for tr in range(T):
        mine = own == tr
        if not stepped[tr]:                                               # nothing of it moves
            for k in ("z", "m", "v", "scale", "sm", "sv"):
                assert same(want[k][tr], c[k][tr]), (k, tr)
            for k in ("theta", "tm", "tv", "pose", "z_view"):
                assert same(want[k][mine], c[k][mine]), (k, tr)
            assert skipped_v[mine].all()
        else:
            assert (want["z_view"][mine] == want["z"][tr]).all()
            if share:
                assert (want["theta"][mine, 4] == want["scale"][tr]).all() and (want["pose"][mine, 5] == want["scale"][tr]).all()
    for vi in np.nonzero(skipped_v)[0]:                                       # an unusable view keeps its pose state
        for k in ("tm", "tv"):
            assert same(want[k][vi], c[k][vi]), (k, vi)
        assert same(want["theta"][vi, :4], c["theta"][vi, :4]) and same(want["pose"][vi, :5], c["pose"][vi, :5])
    if 0 in views:
        e = views.index(0)
        assert want["tflags"][e] == 7 and want["loss"][e] == 0
    planted = special.startswith("flag") or special in ("nan_latent", "inf_pose", "big_latent") or weights in ("zero", "nan") or (special == "neg_scale" and not share)
    if planted:
        assert skipped_v[hit] and stepped[own[hit]] and skipped_v.sum() == 1
    if (special == "neg_scale" and share) or special == "track_overflow":
        assert want["tflags"][own[hit]] == TR.SKIPPED and stepped.sum() == T - 1 and np.isfinite(c["g"].astype(np.float32)).all()
    if special == "all_bad":
        assert want["tflags"][1] == TR.NO_USABLE | TR.SKIPPED and want["loss"][1] == 0 and stepped[0] and stepped[2]
    if special in ("lr0", "frozen"):
        assert same(want["z"], c["z"]) and same(want["m"], c["m"]) and same(want["v"], c["v"]) and stepped.all()
    if special.startswith("pose") or special == "frozen":
        for i in (range(5) if special == "frozen" else [int(special[4:])]):
            if i == 4 and share:
                assert same(want["scale"], c["scale"]) and same(want["sm"], c["sm"])
            else:
                assert same(want["theta"][:, i], c["theta"][:, i]) and same(want["tm"][:, i], c["tm"][:, i])
    if special in ("", "minus_zero") and weights in (None, "given") and 0 not in views:
        assert stepped.all() and not skipped_v.any() and (want["theta"][:, :4] != c["theta"][:, :4]).all() and (want["z"] != c["z"]).any()
    if share and stepped.all():
        assert same(want["tm"][:, 4], c["tm"][:, 4]) and same(want["tv"][:, 4], c["tv"][:, 4])         # a shared scale: the views' own state rests


# ---- fits ------------------------------------------------------------------------------------------------------------------------------------

FIT_VOFF = (0, 2, 3)                         # two tracks over the three shapes of _align_cases.fit_case: a track of two views, a track of one
FIT_WEIGHTS = (1.0, 2.5, 0.75)


@functools.lru_cache(maxsize=None)
def fit_case(name, seed, k):
    """(samples, soff, voff, z0 [T][L], scale0 [T], theta0 [V][5], weights, k, clamp): _align_cases.fit_case's three shapes as the views of
    two tracks; a track starts from its first view's latent and scale"""
    samples, soff, z0, theta0, k, clamp = AC.fit_case(name, seed, 3, k)
    voff = np.array(FIT_VOFF, np.int64)
    first = voff[:-1]
    zt, st = np.array(z0[first]), np.array(theta0[first, 4])
    w = np.array(FIT_WEIGHTS, np.float32)
    for a in (voff, zt, st, w):
        a.setflags(write=False)
    return samples, soff, voff, zt, st, theta0, w, k, clamp
