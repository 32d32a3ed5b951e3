"""Cases of the start-search tests (tests/test_search_cpu.py runs the host program on them, tests/test_gpu_search.py the kernels): the
smallest shapes at which each mechanism can go wrong.  Rows: k 1, 63, 64, 1025, 2049 (a row, a workgroup short of one, two and three
chunks), L 3, 8, 40, 256, B 1 and 3, 1 to 5 starts a shape in uneven numbers, unit and raw latents, posed and unposed, NaN bounds, an
unusable pose, owners of -1 and B, draw on and off.  The select: ties, +-0, infinities, NaN, flagged starts, keep above the usable count,
empty shapes, one start, 4096 starts with many ties, broken tables.  Built with numpy on the CPU; arrays are read-only.
"""
import functools

import numpy as np

from tests import _align_cases as AC
from tests import _complete_cases as CC

SEED = CC.SEED
CLAMP = {False: CC.CLAMP, True: AC.CLAMP}             # lattice units without a pose, metres with one
K_LIST = AC.K_LIST                                    # (1, 63, 64, 1025, 2049)
L_LIST = AC.L_LIST                                    # (3, 8, 40, 256)


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def rows_cases():
    """(B, counts, starts per shape, k, draw, L, unit, posed, bad_owner): with B = 3 the second shape is empty; bad_owner plants owners of -1 and B"""
    out = [(3, (2 * k + 3, 0, 70), (2, 1, 3), k, 1, 3, 1, posed, True) for k in K_LIST for posed in (False, True)]
    out += [(1, (40,), (5,), 63, 1, 8, 0, True, False), (1, (64,), (1,), 64, 0, 40, 1, False, True), (3, (1025, 0, 1030), (1, 2, 4), 1025, 0, 256, 1, True, False),
            (3, (65, 0, 72), (3, 1, 2), 65, 0, 8, 0, False, False), (1, (300,), (4,), 64, 1, 256, 1, False, False)]
    return out


@functools.lru_cache(maxsize=None)
def rows_case(B, counts, starts, k, draw, L, unit, posed, bad_owner):
    """(samples [S][5], soff, own int32 [N], z [N][L], pose [N][6] or None).  Posed: the alignment's camera-frame samples of B shapes; every
    start's pose is its shape's with a small yaw and trans offset, so some rows leave the cube under one start and stay under another; the
    second start of shape 0 repeats the first's pose (equal xyz columns), one start has an unusable pose.  Unposed: the same rows taken as
    lattice rows.  The starts of the shapes are interleaved, so `own` is not sorted."""
    samples, soff, _, pose_b = AC.rows_case(B, counts, k, draw, L, unit, -1)
    rng = np.random.default_rng(12000 + 31 * k + 7 * B + L + sum(starts))
    own = np.concatenate([np.full(n, b, np.int32) for b, n in enumerate(starts)])
    own = own[rng.permutation(len(own))]
    if bad_owner:
        own = np.concatenate([own[:1], np.array([-1], np.int32), own[1:], np.array([B], np.int32)]).astype(np.int32)
    N = len(own)
    z = (0.3 * rng.standard_normal((N, L))).astype(np.float32)
    pose = None
    if posed:
        pose = np.zeros((N, 6), np.float32)
        first = {}
        for s in range(N):
            b = int(np.clip(own[s], 0, B - 1))
            p = np.array(pose_b[b], np.float32)
            valid = 0 <= own[s] < B
            if valid and b == 0 and first.get(b, -1) >= 0:
                p = pose[first[b]].copy()                     # the second start of shape 0: the first's pose
                first[b] = -1
            else:
                dy = np.float32(rng.uniform(-0.05, 0.05))
                yaw = np.float32(np.arctan2(p[1], p[0])) + dy
                p[0], p[1] = np.float32(np.cos(np.float64(yaw))), np.float32(np.sin(np.float64(yaw)))
                p[2:5] += rng.uniform(-0.03, 0.03, 3).astype(np.float32)
                if valid:
                    first.setdefault(b, s)
            pose[s] = p
        pose[np.nonzero(own == B - 1)[0][-1], 5] = 0.0        # an unusable pose: the last start of the last shape (which has samples)
    return _ro(samples, soff, own, z) + (None if pose is None else _ro(pose)[0],)


def reduce_cases():
    """(N, k, posed, bad_pose): the completion's / the alignment's planted reduce case, its shapes taken as starts"""
    return [(3, k, posed, -1) for k in K_LIST for posed in (False, True)] + [(5, 2049, False, -1), (3, 2049, True, 2), (1, 65, True, -1)]


@functools.lru_cache(maxsize=None)
def reduce_case(N, k, posed, bad_pose):
    """(pred, lo, hi [N k], pose [N][6] or None, flags [N], J, cam): J and cam only so that the fits' own reduce can be run on the same rows"""
    if posed:
        pred, lo, hi, J, cam, pose, flags = AC.reduce_case(N, k, 3, 6, bad_pose)
        return pred, lo, hi, pose, flags, J, cam
    pred, lo, hi, J, flags = CC.reduce_case(N, k, 3, 6)
    return pred, lo, hi, None, flags, J, None


# ---- the select: (loss float64 [N], flags int32 [N], coff int64 [B + 1], N, keep) ------------------------------------------------------------

def _crafted():
    nan, inf = np.nan, np.inf
    col = np.array([0.5, 0.25, 0.25, -0.0, 0.0, inf, nan, 0.25, -inf, 1e-300, 0.0, 3.0, 0.5], np.float64)
    fl = np.zeros(len(col), np.int32)
    fl[[1, 11]] = [2, 16]                                     # a tied start without rows, a start with a bad pose
    fl[12] = 4                                                # bit 2 (not stepped) does not keep a start from being ranked
    return col, fl


def select_cases():
    col, fl = _crafted()
    n = len(col)
    out = {}
    for keep in (1, 3, 8, 64):
        out["crafted_keep%d" % keep] = (col, fl, np.array([0, n], np.int64), n, keep)
    # uneven shapes, an empty one, one start, a shape whose starts are all unusable
    loss = np.concatenate([col, [0.125], [np.nan, np.inf], col[::-1]])
    flags = np.concatenate([fl, [0], [0, 0], fl[::-1]]).astype(np.int32)
    coff = np.array([0, n, n, n + 1, n + 3, 2 * n + 3], np.int64)
    out["uneven"] = (loss, flags, coff, len(loss), 4)
    out["one_flagged_start"] = (np.array([0.5]), np.array([1], np.int32), np.array([0, 1], np.int64), 1, 2)
    out["no_starts"] = (np.zeros(0), np.zeros(0, np.int32), np.array([0, 0, 0], np.int64), 0, 2)
    rng = np.random.default_rng(77)
    big = rng.integers(0, 40, 4096).astype(np.float64) / 8.0  # 4096 starts of one shape, 40 values: many ties
    big[rng.integers(0, 4096, 50)] = np.nan
    bf = np.where(rng.uniform(size=4096) < 0.1, 8, 0).astype(np.int32)
    for keep in (1, 64):
        out["big_keep%d" % keep] = (big, bf, np.array([0, 4096], np.int64), 4096, keep)
    out["big_in_a_batch"] = (np.concatenate([col, big, col]), np.concatenate([fl, bf, fl]).astype(np.int32),
                             np.array([0, n, n + 4096, 2 * n + 4096], np.int64), 2 * n + 4096, 5)
    for a in out.values():
        _ro(*a[:3])
    return out


def broken_select_cases():
    """(loss, flags, coff, N, keep): tables that are negative, decreasing, beyond N, or hold more than 4096 starts, on shapes of 1 and of 4097
    starts.  loss and flags hold EXACTLY the words a correct walk may read (the entries of the good shapes come first), so any read through
    a broken entry leaves the buffer."""
    one = (np.array([0.5, 0.25]), np.zeros(2, np.int32))
    out = [one + (np.array(c, np.int64), 2, 2) for c in ([0, 1, -1, 2], [0, 1, 0, 2], [0, 1, 9, 2], [-1, 1, 2], [0, 1, 1 << 40], [1 << 40, 1 << 41])]
    many = (np.linspace(0, 1, 4097), np.zeros(4097, np.int32))
    out += [many + (np.array([0, 4097], np.int64), 4097, 2), many + (np.array([0, 1, 4097], np.int64), 4097, 64)]
    # claimed N beyond the arrays: the table is fine as far as N says, so only the good shape's words may be read
    out += [(np.array([0.5]), np.zeros(1, np.int32), np.array([0, 1, 5000], np.int64), 5000, 2)]
    return out
