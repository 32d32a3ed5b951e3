"""Cases of the shape-encoder tests (tests/test_encode_cpu.py runs the host program on them, tests/test_gpu_encode.py the kernels): the smallest
shapes at which each mechanism can go wrong.  k 1, 63, 64, 65 (the 64 slots of a chunk), chunk - 1, chunk, chunk + 1 and 2 chunk + 76 (three
partial sums, a ragged last one); B 1, 3, 5 with ragged counts that include 0 and 1; L 3, 8, 256 (one column group, and nine of 32); the
Jacobian's own stride L + 3 and a wider one.  Built with numpy on the CPU; arrays are read-only.
"""
import functools

import numpy as np

from tests._encode_ref import CHUNK, EMPTY

CLAMP = 0.1
SEED = 0x5DF0E2C0DE
K_LIST = (1, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 76)

# 4 x the worst deviation of the float32 CPU emulation (tests/_decoder_ref.emulate) from the float64 loop over the ten steps of the trajectory
# cases, in max |z_emulated - z_float64| (profiles/encode_notes.md has the measured values; tests/test_encode_cpu.py re-measures them)
TRAJECTORY_BOUND = {"w128": 6.1e-5, "lat8": 3.6e-7, "asset": 3.9e-7}
TRAJECTORY_SEED = {"w128": 1, "lat8": 1, "asset": 1}


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


# (B, counts, k, draw, L, unit)
def rows_cases():
    out = []
    for k in K_LIST:
        out.append((3, (2 * k + 3, 1, 0), k, 1, 3, 1))
    for k in (1, 65, CHUNK + 1):
        out.append((3, (k, 0, k + 7), k, 0, 3, 1))
    out.append((1, (40,), 65, 1, 8, 0))
    out.append((5, (1, 0, 300, 17, 64), 65, 1, 256, 1))
    out.append((5, (70, 0, 300, 65, 64), 64, 0, 8, 1))
    return out


@functools.lru_cache(maxsize=None)
def rows_case(B, counts, k, draw, L, unit):
    """(samples [S][4], soff [B + 1], z [B][L]); the second shape's latent is exactly zero when there is one"""
    rng = np.random.default_rng(1000 + 31 * k + 7 * B + L)
    soff = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    samples = rng.uniform(-1, 1, (int(soff[-1]), 4)).astype(np.float32)
    z = (0.3 * rng.standard_normal((B, L))).astype(np.float32)
    if B > 1:
        z[1] = 0.0
    return _ro(samples, soff, z)


# (B, k, L, Jstride)
def reduce_cases():
    out = [(3, k, 3, 6) for k in K_LIST]
    out += [(1, 65, 8, 11), (5, 65, 256, 259), (3, 200, 3, 9), (5, 2 * CHUNK + 76, 8, 16), (1, 1, 256, 300)]
    return out


@functools.lru_cache(maxsize=None)
def reduce_case(B, k, L, Jstride):
    """(pred [B k], target [B k], J [B k][Jstride], flags [B]) with planted rows.  Shape 0: pred == target; |pred| exactly at the clamp and
    one ulp beyond; both beyond the clamp on the same side (with a NaN Jacobian row there: its factor is 0, it must add nothing); NaN / inf in
    pred or target.  Shape 1 (B >= 2): every row left out.  The last shape (B >= 3): an infinite Jacobian entry on a row that counts, so the
    gradient is not finite.  Shape 2 of B = 5 is flagged empty on entry."""
    rng = np.random.default_rng(2000 + 31 * k + 7 * B + L)
    n = B * k
    c = np.float32(CLAMP)
    target = rng.uniform(-0.15, 0.15, n).astype(np.float32)
    pred = (target + rng.normal(0, 0.03, n)).astype(np.float32)
    J = rng.standard_normal((n, Jstride)).astype(np.float32)
    plants = [(0.03, 0.03), (c, 0.02), (-c, 0.02), (np.nextafter(c, np.float32(1)), 0.02), (np.nextafter(-c, np.float32(-1)), 0.02),
              (0.2, 0.3), (-0.2, -0.5), (np.nan, 0.01), (0.01, np.inf), (-np.inf, np.nan), (c, c), (0.2, 0.05)]
    for i, (p, t) in enumerate(plants):
        r = (i * 7) % k
        pred[r], target[r] = p, t
        if i == 5:
            J[r] = np.nan
    if B >= 2:
        pred[k:2 * k] = np.nan
    if B >= 3:
        r = (B - 1) * k + (k // 2)
        pred[r], target[r], J[r, 0] = 0.0, 0.05, np.inf
    flags = np.zeros((B,), np.int32)
    if B == 5:
        flags[2] = EMPTY
    return _ro(pred, target, J, flags)


# (B, L, unit, t), or (B, L, unit, t, lr) for a learning rate that is not the schedule's
def step_cases():
    return [(1, 3, 1, 1), (3, 3, 1, 7), (3, 3, 1, 7, 0.0), (3, 3, 0, 1), (5, 8, 1, 400), (5, 8, 0, 3), (5, 256, 1, 2), (3, 256, 0, 800)]


@functools.lru_cache(maxsize=None)
def step_case(B, L, unit, t, lr=None):
    """(z, m, v [B][L], g_zn float64 [B][L], flags [B], code_reg, lr); lr: the schedule's at step t, or the one given -- sdfr_encode_step at
    lr = 0 still runs Adam, so m and v move and z does not.  Shape 1: z = 0 (with unit the gradient through the 1e-12 floor; without,
    no regulariser term).  Shape 2: flagged empty.  Shape 3: a NaN gradient element.  Shape 4: a gradient that overflows float32."""
    rng = np.random.default_rng(3000 + 31 * t + 7 * B + L + unit)
    z = (0.3 * rng.standard_normal((B, L))).astype(np.float32)
    m = (1e-3 * rng.standard_normal((B, L))).astype(np.float32) if t > 1 else np.zeros((B, L), np.float32)
    v = (1e-6 * rng.uniform(0, 1, (B, L))).astype(np.float32) if t > 1 else np.zeros((B, L), np.float32)
    g = 0.05 * rng.standard_normal((B, L))
    flags = np.zeros((B,), np.int32)
    if B > 1:
        z[1] = 0.0
    if B > 2:
        flags[2] = EMPTY
    if B > 3:
        g[3, L // 2] = np.nan
    if B > 4:
        g[4, 0] = 1e60
    return _ro(z, m, v, g, flags) + (1e-4, 5e-3 * 0.1 ** (t // 400) if lr is None else lr)
