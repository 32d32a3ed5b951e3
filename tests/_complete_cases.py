"""Cases of the shape-completion tests (tests/test_complete_cpu.py runs the host program on them, tests/test_gpu_complete.py the kernels): the
smallest shapes at which each mechanism can go wrong.  Views: 0, 1, 65 and 257 points per shape (no point, one, more than a wave, more than a
workgroup), F 0, 1, 4, 64, B 1 and 3, normals present, absent and partly NaN / zero, a point on the sensor, points whose rows leave the
cube, a pose with scale 0.  The reduce: k 1, 63, 64, 65 (the 64 slots of a chunk), 1023, 1025, 2049 (chunk boundaries), L 1, 3, 33, 256 (one
column group, two, nine).  Built with numpy on the CPU; arrays are read-only.
"""
import functools

import numpy as np

from tests import _complete_ref as CR
from tests import _encode_cases as EC
from tests import _encode_ref as ER
from tests import _encode_traj as ET
from tests import _prior_train_cases as PC

CLAMP = EC.CLAMP
SEED = 0x5DF0E2C0DE
ETA, S_MAX = float(np.float32(0.01)), 0.5               # float32 values, as the C ABI takes them

# 4 x the worst deviation of the float32 CPU emulation (tests/_decoder_ref.emulate) from the float64 loop over the ten steps of the mixed-row
# trajectory cases, in max |z_emulated - z_float64| (profiles/complete_notes.md has the measured values; tests/test_complete_cpu.py
# re-measures them).  The seeds are the first of 1, 2, ... at which no row of the float64 run comes within 100 fwd_tol of a kink.
TRAJECTORY_BOUND = {"w128": 9.3e-5, "lat8": 1.7e-7, "asset": 3.2e-7}
TRAJECTORY_SEED = {"w128": 1, "lat8": 1, "asset": 1}


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


# ---- views: (B, counts, F, normals: "all" | "none" | "holes", special: None | "scale0" | "on_sensor" | "far_sensor") -----------------------

def view_cases():
    return [(1, (257,), 4, "all", None), (3, (65, 0, 1), 1, "holes", None), (3, (1, 257, 65), 64, "none", None), (1, (0,), 0, "all", None),
            (3, (65, 65, 65), 0, "all", "scale0"), (3, (65, 65, 65), 4, "holes", "scale0"), (1, (65,), 4, "all", "on_sensor"),
            (1, (65,), 64, "holes", "far_sensor"), (1, (1,), 1, "none", None)]


@functools.lru_cache(maxsize=None)
def view_case(B, counts, F, normals, special):
    """(points float32 [N][3], normals float64 [N][3] or None, ptoff, pose float32 [B][6], origin float32 [3]).  Lattice positions uniform in
    [-1.15, 1.15]^3 -- one point in six starts outside the cube, and offsets carry others over its faces --, taken to the camera frame by
    each shape's pose."""
    rng = np.random.default_rng(4000 + 131 * sum(counts) + 7 * B + F)
    ptoff = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    N = int(ptoff[-1])
    yaw = rng.uniform(-3, 3, B).astype(np.float32)
    pose = np.stack([np.cos(yaw), np.sin(yaw), rng.uniform(-1, 1, B), rng.uniform(-0.5, 0.5, B), rng.uniform(2, 5, B), rng.uniform(1.2, 2.4, B)],
                    1).astype(np.float32)
    x = rng.uniform(-1.15, 1.15, (N, 3))
    pts = np.zeros((N, 3), np.float32)
    for b in range(B):
        c, s, t, sc = float(pose[b, 0]), float(pose[b, 1]), pose[b, 2:5].astype(np.float64), float(pose[b, 5])
        xs = x[ptoff[b]:ptoff[b + 1]] * np.array([1.0, -1.0, 1.0])
        r = np.stack([c * xs[:, 0] + s * xs[:, 2], xs[:, 1], -s * xs[:, 0] + c * xs[:, 2]], 1)
        pts[ptoff[b]:ptoff[b + 1]] = (sc * (r + t)).astype(np.float32)
    nrm = None
    if normals != "none":
        nrm = rng.standard_normal((N, 3))
        if normals == "holes" and N:
            nrm[::5] = np.nan
            nrm[1::7] = 0.0
            nrm[2::11, 1] = np.inf
    origin = np.zeros(3, np.float32)
    if special == "scale0":
        pose[1, 5] = 0.0
        pose[2, 3] = np.nan
    if special == "on_sensor":
        inside = np.nonzero((np.abs(x) < 0.9).all(1))[0]
        origin = pts[inside[0]].copy()                        # the sensor sits on a point inside the cube: its ray has no length
    if special == "far_sensor":
        origin = np.array([30.0, -2.0, -40.0], np.float32)
    return _ro(pts, ptoff, pose, origin) + (nrm,)


BROKEN_PTOFF = ([0, -4, 130, 195], [0, 80, 75, 195], [0, 65, 130, 999], [5, 3, 1, 0], [0, 1 << 40, 1 << 41, 1 << 42], [0, 65, 65, 100])


# ---- interval rows from the encoder's cases ----------------------------------------------------------------------------------------------------

def rows_cases():
    return [(3, (2 * k + 3, 1, 0), k, 1, 3, 1) for k in (1, 65, ER.CHUNK + 1)] + [(3, (65, 0, 72), 65, 0, 3, 1), (1, (40,), 65, 1, 8, 0),
                                                                                  (5, (1, 0, 300, 17, 64), 65, 1, 256, 1), (5, (70, 0, 300, 65, 64), 64, 0, 33, 1)]


@functools.lru_cache(maxsize=None)
def rows_case(B, counts, k, draw, L, unit):
    """(samples [S][5], soff, z): the encoder's case with an upper bound behind the target, a third of the rows exact"""
    samples, soff, z = EC.rows_case(B, counts, k, draw, L, unit)
    rng = np.random.default_rng(5000 + len(samples))
    width = rng.uniform(0, 0.3, len(samples)).astype(np.float32)
    width[::3] = 0
    s5 = np.concatenate([samples, (samples[:, 3] + width)[:, None]], 1).astype(np.float32)
    return _ro(s5)[0], soff, z


K_LIST = (1, 63, 64, 65, 1023, 1025, 2049)


def reduce_cases():
    return [(3, k, 3, 6) for k in K_LIST] + [(1, 65, 1, 4), (3, 65, 33, 36), (1, 65, 256, 259), (5, 2049, 33, 40), (5, 65, 8, 11)]


@functools.lru_cache(maxsize=None)
def reduce_case(B, k, L, Jstride):
    """(pred, lo, hi [B k], J [B k][Jstride], flags [B]): the encoder's planted case (shape 0 the clamp's edges and non-finite values, shape 1
    left out, the last shape an infinite Jacobian entry on a row that counts) with its target as the lower bound and, by row index mod 4: 0 an
    equal upper bound, 1 an upper bound up to 0.1 above, 2 the interval moved below the target (so the prediction tends to lie above it), 3 an
    unbounded side.  Then planted: lo > hi, both bounds infinite, a NaN bound, a prediction exactly on a bound, bounds beyond the clamp."""
    pred, target, J, flags = (np.array(a) for a in EC.reduce_case(B, k, L, Jstride))
    rng = np.random.default_rng(6000 + 31 * k + 7 * B + L)
    n = B * k
    lo, hi = target.copy(), target.copy()
    w = rng.uniform(0, 0.1, n).astype(np.float32)
    i = np.arange(n)
    hi[i % 4 == 1] += w[i % 4 == 1]
    lo[i % 4 == 2] -= w[i % 4 == 2] + np.float32(0.05)
    hi[i % 4 == 2] -= np.float32(0.05)
    hi[i % 8 == 3] = np.inf
    lo[i % 8 == 7] = -np.inf
    c = np.float32(CLAMP)
    plants = [(0.03, 0.05, 0.04), (0.01, -np.inf, np.inf), (0.01, np.nan, 0.05), (0.01, 0.0, np.nan), (0.02, 0.02, 0.06), (0.06, 0.02, 0.06),
              (0.0, 0.2, 0.3), (0.15, 0.2, 0.3), (-0.3, -0.2, 0.3), (0.05, -0.0, 0.0), (c, 0.0, c), (np.nextafter(c, np.float32(1)), 0.0, c)]
    for j, (p, a, e) in enumerate(plants):
        r = (3 + j * 5) % k
        pred[r], lo[r], hi[r] = p, a, e
    return _ro(pred, lo, hi, J, flags)


# ---- fits ------------------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def fit_case(name, seed, B, k):
    """(samples [B k][5] float32, soff, z0, k): the rows of the encoder's trajectory case -- each starts 0.01 or more from its target t and
    inside the clamp -- turned into a mix by row index mod 6: 0, 1 exact [t, t]; 2, 3 one-sided, a free-space row's kind: the interval of
    width 0.05 that ends at t and lies on the far side of it from the start prediction p0, so the row pulls; 4 satisfied: [min(p0, t) - 0.02, max(p0, t) +
    0.02], no pull; 5 invalid (NaN bounds)."""
    samples, soff, z0, k = ET.fit_case(name, seed, B, k)
    net = PC.net(name)
    zn0 = ER.normalised(z0.astype(np.float64), True, np.float64)
    out = np.zeros((len(samples), 5), np.float32)
    out[:, :4] = samples
    for b in range(B):
        sl = slice(int(soff[b]), int(soff[b + 1]))
        pts, t = samples[sl, :3].astype(np.float64), samples[sl, 3].astype(np.float64)
        p0 = ET.decoder64(net)(np.concatenate([np.repeat(zn0[b:b + 1], len(pts), 0), pts], 1))[0]
        i = np.arange(len(pts))
        lo, hi = t.copy(), t.copy()
        one = (i % 6 == 2) | (i % 6 == 3)
        lo[one & (p0 > t)] -= 0.05
        hi[one & (p0 < t)] += 0.05
        sat = i % 6 == 4
        lo[sat], hi[sat] = np.minimum(p0, t)[sat] - 0.02, np.maximum(p0, t)[sat] + 0.02
        lo[i % 6 == 5] = hi[i % 6 == 5] = np.nan
        out[sl, 3], out[sl, 4] = lo, hi
    return _ro(out)[0], soff, z0, k


def kink_margin(net, inputs, pred, lo, hi, clamp):
    """per row: the distance to the nearest kink of the interval loss -- the prediction on a clamped bound, or on the clamp -- over
    m = 100 fwd_tol of that row; inf for a row the rule leaves out"""
    from tests import _decoder_ref as DR
    r = DR.evaluate(net, inputs, "f32")
    m = 100.0 * DR.fwd_tol(net, r, "f32")
    p, lo, hi = np.asarray(pred, np.float64), np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(p) & (lo <= hi)
        cp, cl, ch = np.clip(p, -clamp, clamp), np.clip(lo, -clamp, clamp), np.clip(hi, -clamp, clamp)
        d = np.minimum(np.minimum(np.abs(cp - cl), np.abs(cp - ch)), np.abs(np.abs(p) - clamp))
    return np.where(ok, d / m, np.inf)


def run(name, decoder, ft, samples, soff, z0, k, iters, watch_margin=False, **fit):
    net = PC.net(name)
    margins, zs = [], []

    def watch(it, inputs, pred, lo, hi, J):
        if watch_margin:
            margins.append(kink_margin(net, inputs, pred, lo, hi, fit["clamp"]))

    out = CR.loop(decoder, samples, soff, z0, iters, k, False, unit=True, ft=ft, watch=watch, zs=zs, **fit)
    out["zs"], out["z0"] = zs, np.asarray(z0)
    if watch_margin:
        out["margin"] = np.array(margins)
    return out


def cpu_runs(name, seed=None):
    net = PC.net(name)
    samples, soff, z0, k = fit_case(name, TRAJECTORY_SEED[name] if seed is None else seed, ET.B, ET.K)
    ref = run(name, ET.decoder64(net), np.float64, samples, soff, z0, k, ET.STEPS, watch_margin=True, clamp=ET.CLAMPS[name], **ET.FIT)
    emu = run(name, ET.decoder32(net), np.float32, samples, soff, z0, k, ET.STEPS, clamp=ET.CLAMPS[name], **ET.FIT)
    return ref, emu
