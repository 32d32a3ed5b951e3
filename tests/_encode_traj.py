"""Fits of the shape-encoder tests that run a decoder: the cases, the float64 reference runs and the float32 emulation runs, all on the CPU
(tests/test_encode_cpu.py checks and calibrates on them, tests/test_gpu_encode.py compares the device with them).

Trajectory cases: B shapes x K rows, every row on every iteration (draw off), STEPS steps.  The targets are the same decoder's values at
another unit latent plus a fixed offset pattern, so no row starts on the loss's kink p = t; a case is admitted only if no row of the float64
run comes within m = 100 fwd_tol of a kink on any step (margin > 1 below).  The seeds in tests/_encode_cases.TRAJECTORY_SEED were chosen so.
"""
import functools

import numpy as np

from tests import _decoder_ref as DR
from tests import _encode_cases as EC
from tests import _encode_ref as ER
from tests import _prior_train_cases as PC

NAMES = ("w128", "lat8", "asset")
STEPS, B, K = 10, 2, 96
FIT = dict(lr=5e-3, lr_step=5, lr_factor=0.1, code_reg=1e-4)
CLAMPS = {"w128": 0.1, "lat8": 0.3, "asset": 0.1}          # lat8's values on the cube all lie below -0.12: a clamp of 0.1 would leave it no gradient
OFFSETS = (0.021, -0.034, 0.047, -0.019, 0.038, -0.052)

# the recovery case: seed 2 of the seeds 1 .. 8 tried on the CPU; its float64 loop goes from a loss of 0.1258 to 0.00094 (seeds 4, 6 and 7 end
# in another minimum, above a tenth of their initial loss, and were not taken)
RECOVERY = dict(n=4096, iters=200, lr=2e-2, lr_step=120, lr_factor=0.1, clamp=0.1, seed=2)


def decoder64(net):
    def run(x):
        r = DR.evaluate(net, x, "f32", want_masses=False)
        return r.out, r.J
    return run


def decoder32(net):
    def run(x):
        e = DR.emulate(net, np.asarray(x, np.float32))
        return e.out, e.J
    return run


def _unit(rng, n, L):
    z = rng.standard_normal((n, L))
    return z / np.linalg.norm(z, axis=1, keepdims=True)


@functools.lru_cache(maxsize=None)
def fit_case(name, seed, B, k):
    """(samples [B k][4] float32, soff, z0 [B][L] float32 (not of unit length), k).  The points are the first k per shape, of uniform candidates
    in the cube, at which the float64 decoder's value at the start latent lies 0.01 inside the clamp, the target 0.005 inside it and the two
    0.01 apart: rows that carry a gradient and start away from every kink."""
    net = PC.net(name)
    L = net.n_inputs - 3
    clamp = CLAMPS[name]
    rng = np.random.default_rng(7000 + 131 * seed + L)
    z_true = _unit(rng, B, L).astype(np.float32)
    z0 = (_unit(rng, B, L) * rng.uniform(0.7, 1.3, (B, 1))).astype(np.float32)
    zn0 = ER.normalised(z0.astype(np.float64), True, np.float64)
    rows = []
    for b in range(B):
        pts = rng.uniform(-1, 1, (40 * k, 3)).astype(np.float32)
        val = decoder64(net)(np.concatenate([np.repeat(z_true[b:b + 1], len(pts), 0), pts], 1).astype(np.float64))[0]
        p0 = decoder64(net)(np.concatenate([np.repeat(zn0[b:b + 1], len(pts), 0), pts.astype(np.float64)], 1))[0]
        t = (val + np.asarray(OFFSETS)[np.arange(len(pts)) % len(OFFSETS)]).astype(np.float32)
        keep = np.nonzero((np.abs(p0) < clamp - 0.01) & (np.abs(t) < clamp - 0.005) & (np.abs(p0 - t) > 0.01))[0]
        assert len(keep) >= k, (name, b, len(keep))
        rows.append(np.concatenate([pts[keep[:k]], t[keep[:k], None]], 1))
    samples = np.concatenate(rows).astype(np.float32)
    soff = np.arange(B + 1, dtype=np.int64) * k
    for a in (samples, soff, z0):
        a.setflags(write=False)
    return samples, soff, z0, k


def kink_margin(net, inputs, pred, target, clamp):
    """per row: the distance to the nearest kink of the loss over m = 100 fwd_tol of that row"""
    r = DR.evaluate(net, inputs, "f32")
    m = 100.0 * DR.fwd_tol(net, r, "f32")
    p, t = np.asarray(pred, np.float64), np.asarray(target, np.float64)
    d = np.minimum(np.abs(np.clip(p, -clamp, clamp) - np.clip(t, -clamp, clamp)), np.abs(np.abs(p) - clamp))
    return d / m


def run(name, decoder, ft, samples, soff, z0, k, iters, watch_margin=False, **fit):
    net = PC.net(name)
    margins, zs = [], []

    def watch(it, inputs, pred, target, J):
        if watch_margin:
            margins.append(kink_margin(net, inputs, pred, target, fit["clamp"]))

    out = ER.loop(decoder, samples, soff, z0, iters, k, False, unit=True, ft=ft, watch=watch, zs=zs, **fit)
    out["zs"], out["z0"] = zs, np.asarray(z0)
    if watch_margin:
        out["margin"] = np.array(margins)
    return out


def cpu_runs(name):
    net = PC.net(name)
    samples, soff, z0, k = fit_case(name, EC.TRAJECTORY_SEED[name], B, K)
    ref = run(name, decoder64(net), np.float64, samples, soff, z0, k, STEPS, watch_margin=True, clamp=CLAMPS[name], **FIT)
    emu = run(name, decoder32(net), np.float32, samples, soff, z0, k, STEPS, clamp=CLAMPS[name], **FIT)
    return ref, emu


@functools.lru_cache(maxsize=None)
def recovery_case():
    """w128: (samples [n][4], soff, z_true [1][3], z0 = -z_true): the decoder's own values at a known unit latent, the start on the far side"""
    net = PC.net("w128")
    rng = np.random.default_rng(RECOVERY["seed"])
    z_true = _unit(rng, 1, 3).astype(np.float32)
    pts = rng.uniform(-1, 1, (RECOVERY["n"], 3)).astype(np.float32)
    val = decoder64(net)(np.concatenate([np.repeat(z_true, len(pts), 0), pts], 1).astype(np.float64))[0]
    samples = np.concatenate([pts, val.astype(np.float32)[:, None]], 1)
    return samples, np.array([0, len(pts)], np.int64), z_true, (-z_true).copy()


@functools.lru_cache(maxsize=None)
def recovery_reference():
    samples, soff, _, z0 = recovery_case()
    fit = {k: RECOVERY[k] for k in ("lr", "lr_step", "lr_factor", "clamp")}
    return run("w128", decoder64(PC.net("w128")), np.float64, samples, soff, z0, RECOVERY["n"], RECOVERY["iters"], code_reg=1e-4, **fit)
