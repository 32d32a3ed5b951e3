"""Cases of the pose-and-shape fit's tests (tests/test_align_cpu.py runs the host program on them, tests/test_gpu_align.py the kernels): the
smallest shapes at which each mechanism can go wrong.  k 1, 63, 64, 1025, 2049 (slot, chunk and fold boundaries), L 3, 8, 40, 256 (L + 7 > 32
crosses the column fold), B 1 and 3 with an empty shape, a broken soff entry, an unusable pose and a row exactly on the cube's face.  Built
with numpy on the CPU; arrays are read-only.
"""
import functools

import numpy as np

from tests import _align_ref as AR
from tests import _complete_cases as CC
from tests import _encode_cases as EC
from tests import _encode_ref as ER

CLAMP = 0.2                                              # metres
SEED = CC.SEED
ETA, S_MAX = float(np.float32(0.02)), 1.0               # float32 values, as the C ABI takes them (metres)
K_LIST = (1, 63, 64, 1025, 2049)
L_LIST = (3, 8, 40, 256)

# The pose whose lattice positions are exact in float32: cos 1, sin 0, trans (0.5, -0.25, 3), scale 2.  FACE maps to x = (1, -0.3, 0.1) up
# to the rounding of its last two coordinates -- exactly on the face x0 = 1, inside the cube --, BEYOND one float32 step outside it.
EXACT_POSE = np.array([1.0, 0.0, 0.5, -0.25, 3.0, 2.0], np.float32)
FACE = np.array([3.0, 0.1, 6.2], np.float32)
BEYOND = np.array([np.nextafter(np.float32(3.0), np.float32(4.0)), 0.1, 6.2], np.float32)

# 4 x the worst deviation of the float32 CPU emulation from the float64 loop over the ten steps of the trajectory cases, in
# max(|z_emulated - z_float64|, |theta_emulated - theta_float64|) (profiles/align_notes.md has the measured values; tests/test_align_cpu.py
# re-measures them).  The seeds are the first of 1, 2, ... at which no row of the float64 run comes within 100 fwd_tol of a kink.
# (w128: seeds 1, 2 and 3 were refused -- a row 0.014 margins from a bound, rows 0.58 and 0.997 margins from a face.)
TRAJECTORY_BOUND = {"w128": 8.3e-7, "lat8": 2.9e-6, "asset": 1.45e-6}
TRAJECTORY_SEED = {"w128": 4, "lat8": 1, "asset": 1}


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def to_camera(x, pose_b):
    """lattice positions [n][3] (float64) -> camera-frame points (float64): scale (rot_yaw diag(1, -1, 1) x + trans)"""
    c, s, t, sc = float(pose_b[0]), float(pose_b[1]), np.asarray(pose_b[2:5], np.float64), float(pose_b[5])
    xs = np.asarray(x, np.float64) * np.array([1.0, -1.0, 1.0])
    r = np.stack([c * xs[:, 0] + s * xs[:, 2], xs[:, 1], -s * xs[:, 0] + c * xs[:, 2]], 1)
    return sc * (r + t)


def random_poses(rng, B):
    yaw = rng.uniform(-3, 3, B).astype(np.float32)
    theta = np.stack([yaw, rng.uniform(-1, 1, B), rng.uniform(-0.5, 0.5, B), rng.uniform(2, 5, B), rng.uniform(1.2, 2.4, B)], 1).astype(np.float32)
    return theta, AR.pose_row(theta)


# ---- observation rows: the views of the completion's cases, whose points are camera-frame already --------------------------------------------

def sample_cases():
    """(B, counts, F, normals, special): special None | "on_sensor" | "far_sensor" | "bad_points" (a NaN and an infinite coordinate)"""
    return [(1, (257,), 4, "all", None), (3, (65, 0, 1), 1, "holes", None), (3, (1, 257, 65), 64, "none", None), (1, (0,), 0, "all", None),
            (1, (65,), 4, "all", "on_sensor"), (1, (65,), 64, "holes", "far_sensor"), (3, (65, 65, 65), 4, "holes", "bad_points"), (1, (1,), 1, "none", None)]


@functools.lru_cache(maxsize=None)
def sample_case(B, counts, F, normals, special):
    """(points float32 [N][3], ptoff, origin float32 [3], normals float64 [N][3] or None)"""
    pts, ptoff, _, origin, nrm = CC.view_case(B, counts, F, normals, special if special in ("on_sensor", "far_sensor") else None)
    pts = np.array(pts)
    if special == "bad_points":
        pts[3, 1], pts[70, 0], pts[140] = np.nan, np.inf, -np.inf
    return _ro(pts, ptoff, origin) + (nrm,)


BROKEN_PTOFF = CC.BROKEN_PTOFF


# ---- the iteration's rows ----------------------------------------------------------------------------------------------------------------------

def rows_cases():
    """(B, counts, k, draw, L, unit, bad_pose): with B = 3 the second shape is empty; bad_pose: the shape whose pose is unusable, or -1"""
    out = [(3, (2 * k + 3, 0, 70), k, 1, 3, 1, -1) for k in K_LIST]
    out += [(3, (65, 0, 72), 65, 0, 8, 0, 2), (1, (40,), 63, 1, 40, 1, -1), (3, (1025, 0, 1030), 1025, 0, 256, 1, 0), (1, (64,), 64, 0, 3, 1, 0)]
    return out


@functools.lru_cache(maxsize=None)
def rows_case(B, counts, k, draw, L, unit, bad_pose):
    """(samples [S][5] camera frame, soff, z [B][L], pose [B][6]).  Lattice positions uniform in [-1.15, 1.15]^3 taken to the camera frame by
    each shape's pose, so about a third of the rows leave the cube; shape 0 has EXACT_POSE and FACE / BEYOND as its first two samples; a third
    of the bounds exact, some NaN."""
    rng = np.random.default_rng(8000 + 31 * k + 7 * B + L)
    soff = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    S = int(soff[-1])
    _, pose = random_poses(rng, B)
    pose[0] = EXACT_POSE
    samples = np.zeros((S, 5), np.float32)
    for b in range(B):
        n = counts[b]
        samples[soff[b]:soff[b + 1], :3] = to_camera(rng.uniform(-1.15, 1.15, (n, 3)), pose[b]).astype(np.float32)
    samples[0, :3] = FACE
    if counts[0] > 1:
        samples[1, :3] = BEYOND
    lo = rng.uniform(-0.3, 0.3, S).astype(np.float32)
    width = rng.uniform(0, 0.3, S).astype(np.float32)
    width[::3] = 0
    samples[:, 3], samples[:, 4] = lo, lo + width
    samples[5::11, 3:] = np.nan
    if bad_pose >= 0:
        pose[bad_pose, 5] = 0.0 if bad_pose else np.nan
    z = (0.3 * rng.standard_normal((B, L))).astype(np.float32)
    return _ro(samples, soff, z, pose)


BROKEN_SOFF = (([0, -4, 75, 115], None), ([0, 80, 75, 115], None), ([0, 65, 65, 999], None), ([0, 65, 65, 137], 100), ([0, 1 << 40, 1 << 41, 1 << 42], None))


# ---- the reduce on synthetic predictions and Jacobians -------------------------------------------------------------------------------------------

def reduce_cases():
    """(B, k, L, Jstride, bad_pose)"""
    out = [(3, k, 3, 6, -1) for k in K_LIST]
    out += [(1, 64, 8, 11, -1), (3, 63, 40, 43, 0), (1, 1025, 40, 48, -1), (3, 65, 256, 259, -1), (1, 2049, 256, 259, -1), (3, 2049, 8, 16, 2)]
    return out


@functools.lru_cache(maxsize=None)
def reduce_case(B, k, L, Jstride, bad_pose, unit_scale=False):
    """(pred, lo, hi [B k], J [B k][Jstride], cam [B k][3], pose [B][6], flags [B]): the completion's planted case (rows on the clamp's edges,
    non-finite values, lo > hi, unbounded sides, an infinite Jacobian entry on a row that counts; shape 1 left out) with metric bounds
    (scaled by the shape's scale, so the mix of kinds survives), camera-frame points of random poses, and NaN / infinite entries planted in
    the position columns of J on rows with and without a pull.  unit_scale: every scale is exactly 1 and the bounds are the completion's."""
    pred, lo, hi, J, flags = (np.array(a) for a in CC.reduce_case(B, k, L, Jstride))
    rng = np.random.default_rng(9000 + 31 * k + 7 * B + L)
    _, pose = random_poses(rng, B)
    if unit_scale:
        pose[:, 5] = 1.0
    per_row = np.repeat(pose, k, 0)
    cam = np.concatenate([to_camera(rng.uniform(-1, 1, (k, 3)), pose[b]) for b in range(B)]).astype(np.float32)
    if not unit_scale:
        lo, hi = (per_row[:, 5] * lo).astype(np.float32), (per_row[:, 5] * hi).astype(np.float32)
    if k > 40:
        J[(3 + 5 * 5) % k, L + 1] = np.nan                    # on the row planted as (0.06, 0.02, 0.06): satisfied, no pull -- it must add nothing
        J[17 % k, L + 2] = np.inf
    if bad_pose >= 0:
        pose[bad_pose, 5] = np.nan                            # (the reduce itself does not judge a pose: the metric prediction is NaN)
    return _ro(pred, lo, hi, J, cam, pose, flags)


# ---- the step ----------------------------------------------------------------------------------------------------------------------------------

def step_cases():
    """(B, L, unit, t, rates): rates picks the learning rates -- "all", "frozen_pose" (every pose rate 0), "frozen_latent" (lr 0), "no_scale"""
    return [(1, 3, 1, 1, "all"), (5, 3, 1, 7, "all"), (5, 8, 0, 3, "no_scale"), (5, 40, 1, 400, "frozen_pose"), (5, 256, 1, 2, "frozen_latent"),
            (3, 256, 0, 800, "all")]


@functools.lru_cache(maxsize=None)
def step_case(B, L, unit, t, rates):
    """(z, m, v [B][L], theta, tm, tv [B][5], pose [B][6], g float64 [B][L + 5], flags [B], code_reg, lr, lr_pose [5]): the encoder's step case
    (shape 1 z = 0, shape 2 flagged empty, shape 3 a NaN latent gradient, shape 4 a gradient that overflows float32) with a pose.  Shape 0's
    pose gradient is ordinary; with B = 3, shape 2's scale is 1e-3 with a large positive scale gradient (its update would make it negative:
    skipped unless the scale is frozen); with B = 5, shape 1's scale gradient is infinite."""
    z, m, v, gl, flags, code_reg, lr = EC.step_case(B, L, unit, t)
    flags = np.array(flags)
    rng = np.random.default_rng(9500 + 31 * t + 7 * B + L)
    theta, pose = random_poses(rng, B)
    tm = (1e-3 * rng.standard_normal((B, 5))).astype(np.float32) if t > 1 else np.zeros((B, 5), np.float32)
    tv = (1e-6 * rng.uniform(0, 1, (B, 5))).astype(np.float32) if t > 1 else np.zeros((B, 5), np.float32)
    g = np.concatenate([np.array(gl), 0.05 * rng.standard_normal((B, 5))], 1)
    if B == 3:
        flags[2] = 0
        theta[2, 4], g[2, L + 4], tm[2, 4] = 1e-3, 5.0, 1.0
        pose[2] = AR.pose_row(theta[2])[0]
    if B == 5:
        g[1, L + 4] = np.inf
    lr_pose = {"all": (1e-2, 2e-2, 5e-3, 1e-2, 3e-2), "frozen_pose": (0.0,) * 5, "frozen_latent": (1e-2,) * 5, "no_scale": (1e-2, 1e-2, 1e-2, 1e-2, 0.0)}[rates]
    return _ro(z, m, v, theta, tm, tv, pose, g, flags) + (code_reg, 0.0 if rates == "frozen_latent" else lr, lr_pose)


# ---- fits ------------------------------------------------------------------------------------------------------------------------------------

FIT_SCALE = 1.5                              # every shape of a fit case has this scale, so one metric clamp serves them all
FIT_OFFSET = (0.012, 0.008, -0.006, 0.01, 0.02)            # start minus truth in yaw, tx, ty, tz, scale: non-zero in every parameter
OUTSIDE_ROW = 6                              # this row of shape 0 (an exact row) is moved to lattice x = (1.3, 0.1, -0.2): it leaves the cube


@functools.lru_cache(maxsize=None)
def fit_case(name, seed, B, k):
    """(samples [B k][5] float32 camera frame and metric, soff, z0, theta0 [B][5] float32, k, clamp): the completion's mixed-row fit case
    (by row index mod 6: 0, 1 exact; 2, 3 one-sided; 4 satisfied; 5 invalid) seen through one true pose per shape -- its positions taken to
    the camera frame, its bounds multiplied by the scale --, the fit starting FIT_OFFSET away from that pose."""
    from tests import _encode_traj as ET
    lat, soff, z0, k = CC.fit_case(name, seed, B, k)
    rng = np.random.default_rng(9800 + 131 * seed + B)
    theta, _ = random_poses(rng, B)
    theta[:, 4] = FIT_SCALE
    pose = AR.pose_row(theta)
    out = np.zeros((len(lat), 5), np.float32)
    for b in range(B):
        sl = slice(int(soff[b]), int(soff[b + 1]))
        x = lat[sl, :3].astype(np.float64)
        if b == 0:
            x[OUTSIDE_ROW] = (1.3, 0.1, -0.2)
        out[sl, :3] = to_camera(x, pose[b]).astype(np.float32)
        out[sl, 3:] = (np.float32(FIT_SCALE) * lat[sl, 3:]).astype(np.float32)
    theta0 = (theta + np.asarray(FIT_OFFSET, np.float32)).astype(np.float32)
    return _ro(out, soff, z0, theta0) + (k, FIT_SCALE * ET.CLAMPS[name])


FIT = dict(lr=5e-3, lr_pose=(2e-3, 2e-3, 2e-3, 2e-3, 2e-3), lr_step=5, lr_factor=0.1, code_reg=1e-4)


def kink_margin(net, inputs, pred, lo, hi, pose, cam, k, clamp):
    """per row: the distance to the nearest kink over 100 times the float32 error that could carry the row across it; inf for a row the rule
    leaves out.  The kinks of the loss -- the metric prediction on a bound that lies inside the clamp, or on the clamp -- are measured against m = 100 fwd_tol
    scale (the decoder's own forward tolerance, in metres); the cube's faces |x_a| = 1 against 100 times the rounding of a lattice
    coordinate, 2^-24 (|q| / scale + |trans| + 1)."""
    from tests import _decoder_ref as DR
    r = DR.evaluate(net, inputs, "f32")
    pose = np.repeat(np.asarray(pose, np.float64), k, 0)
    sc = pose[:, 5]
    m = 100.0 * DR.fwd_tol(net, r, "f32") * sc
    p, lo, hi = sc * np.asarray(pred, np.float64), np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    x = AR.lattice_x(cam, pose)
    face = np.abs(1.0 - np.abs(x)).min(1) / (100.0 * 2.0 ** -24 * (np.abs(np.asarray(cam, np.float64)).max(1) / sc + np.abs(pose[:, 2:5]).max(1) + 1.0))
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(p) & (lo <= hi)
        d = np.abs(np.abs(p) - clamp)                        # the clamp itself; a bound is a kink of its own only strictly inside the clamp
        for bound in (lo, hi):
            d = np.where(np.abs(bound) < clamp, np.minimum(d, np.abs(p - bound)), d)
    return np.where(ok, d / m, np.inf), face


def run(name, decoder, ft, samples, soff, z0, theta0, k, iters, watch_margin=False, **fit):
    from tests import _prior_train_cases as PC
    net = PC.net(name)
    margins, faces, trace = [], [], []
    cams = {}

    def watch(it, inputs, pred, lo, hi, J, pose):
        if watch_margin:
            B = len(pose)
            cam = np.concatenate([np.asarray(samples)[int(soff[b]):int(soff[b]) + k, :3] for b in range(B)])       # draw off: the first k rows
            a, f = kink_margin(net, inputs, pred, lo, hi, pose, cam, k, fit["clamp"])
            margins.append(a), faces.append(f)

    out = AR.loop(decoder, samples, soff, z0, theta0, iters, k, False, unit=True, ft=ft, watch=watch, trace=trace, **fit)
    out["trace"], out["z0"], out["theta0"] = trace, np.asarray(z0), np.asarray(theta0)
    if watch_margin:
        out["margin"], out["face"] = np.array(margins), np.array(faces)
    return out


def cpu_runs(name, seed=None):
    from tests import _encode_traj as ET
    from tests import _prior_train_cases as PC
    net = PC.net(name)
    samples, soff, z0, theta0, k, clamp = fit_case(name, TRAJECTORY_SEED[name] if seed is None else seed, ET.B, ET.K)
    ref = run(name, ET.decoder64(net), np.float64, samples, soff, z0, theta0, k, ET.STEPS, watch_margin=True, clamp=clamp, **FIT)
    emu = run(name, ET.decoder32(net), np.float32, samples, soff, z0, theta0, k, ET.STEPS, clamp=clamp, **FIT)
    return ref, emu


def deviation(a, b):
    """the worst difference of two runs' traces, in max(|z - z'|, |theta - theta'|)"""
    return max(max(float(np.abs(za.astype(np.float64) - zb).max()), float(np.abs(ta.astype(np.float64) - tb).max())) for (za, ta), (zb, tb) in zip(a, b))
