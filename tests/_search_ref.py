"""A numpy restatement of the search for a fit's start (csrc/search.hip, csrc/search_cells.h; include/sdfr.h has the contract), written from
the header's comments.  TEST INFRASTRUCTURE ONLY: no device code.

Three rules: a start's rows (rows: the completion's or the alignment's rows of the shape own[s], drawn as that shape draws, with the
start's own latent and pose), the loss alone (reduce: the fits' row rules, the summation order of tests/_encode_ref.py over the two
columns loss and count) and the ranking (select: rank counting by (loss, index) over the usable starts of a shape).
"""
import numpy as np

from tests import _align_ref as AR
from tests import _complete_ref as CR
from tests import _encode_ref as ER

MAX_KEEP, MAX_STARTS = 64, 4096
UNUSABLE = ER.EMPTY | ER.NO_ROWS | ER.BAD_TABLE | AR.BAD_POSE


def rows(samples, soff, B, own, k, draw_on, seed, it, z, unit, pose=None, S=None, shape0=0):
    """sdfr_search_rows: (inputs [N k][L + 3], cam [N k][3] (zeros without a pose), lo [N k], hi [N k], zn [N][L], flags [N])"""
    samples = np.asarray(samples, np.float32).reshape(-1, 5)
    S = len(samples) if S is None else S
    z = np.asarray(z, np.float32)
    N, L = z.shape
    inputs, cam = np.zeros((N * k, L + 3), np.float32), np.zeros((N * k, 3), np.float32)
    lo, hi = np.zeros((N * k,), np.float32), np.zeros((N * k,), np.float32)
    zn, flags = ER.normalised(z, unit), np.zeros((N,), np.int32)
    for s in range(N):
        o = int(own[s])
        if not 0 <= o < B:                            # nothing is read through it
            flags[s] = ER.BAD_TABLE
            continue
        sub = np.array([int(soff[o]), int(soff[o + 1])], np.int64)
        sl = slice(s * k, (s + 1) * k)
        if pose is None:
            inputs[sl], lo[sl], hi[sl], _, fl = CR.rows(samples[:S], sub, 1, k, draw_on, seed, it, z[s:s + 1], unit, S=S, shape0=shape0 + o)
        else:
            inputs[sl], cam[sl], lo[sl], hi[sl], _, fl = AR.rows(samples[:S], sub, 1, k, draw_on, seed, it, z[s:s + 1], unit,
                                                                 np.asarray(pose, np.float32).reshape(N, 6)[s:s + 1], S=S, shape0=shape0 + o)
        flags[s] = fl[0]
    return inputs, cam, lo, hi, zn, flags


def reduce(pred, lo, hi, pose, N, k, clamp, flags):
    """sdfr_search_reduce: (loss float64 [N], flags with bit 1 added, part [N][chunks][2])"""
    pred = np.asarray(pred, np.float32)
    with np.errstate(all="ignore"):
        p = pred if pose is None else (np.repeat(np.asarray(pose, np.float32).reshape(N, 6)[:, 5], k) * pred).astype(np.float32)
        e, _, ok = CR.row_rule(p, lo, hi, clamp)
    vals = np.stack([e, ok.astype(np.float64)], 1)
    chunks = (k + ER.CHUNK - 1) // ER.CHUNK
    part = np.zeros((N, chunks, 2), np.float64)
    loss = np.zeros((N,), np.float64)
    flags = np.asarray(flags, np.int32).copy()
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(N):
            tot = np.zeros((2,), np.float64)
            for ch in range(chunks):
                part[s, ch] = ER.chunk_sum(vals[s * k + ch * ER.CHUNK:s * k + min(k, (ch + 1) * ER.CHUNK)])
                tot = tot + part[s, ch]
            if tot[1] > 0:
                loss[s] = tot[0] / tot[1]
            else:
                flags[s] |= ER.NO_ROWS
    return loss, flags, part


def usable(loss, flags):
    return ((np.asarray(flags, np.int32) & UNUSABLE) == 0) & np.isfinite(np.asarray(loss, np.float64))


def select(loss, flags, coff, N, keep):
    """sdfr_search_select by rank counting: (order int32 [B][keep], count int32 [B]).  loss and flags may be shorter than N says: nothing is
    read through a broken entry."""
    B = len(coff) - 1
    order, count = np.full((B, keep), -1, np.int32), np.zeros((B,), np.int32)
    for b in range(B):
        a, e = int(coff[b]), int(coff[b + 1])
        if a < 0 or e < a or e > N or e - a > MAX_STARTS:
            count[b] = -1
            continue
        l, ok = np.asarray(loss[a:e], np.float64), usable(loss[a:e], flags[a:e])
        count[b] = min(keep, int(ok.sum()))
        for i in np.nonzero(ok)[0]:
            with np.errstate(invalid="ignore"):
                before = ok & ((l < l[i]) | ((l == l[i]) & (np.arange(e - a) < i)))
            r = int(before.sum())
            if r < keep:
                order[b, r] = a + i
    return order, count


def select_lexsort(loss, flags, coff, N, keep):
    """the same by a stable sort: numpy.lexsort over (index, loss) of the usable starts (+0.0 added first, so -0.0 ties with 0.0)"""
    B = len(coff) - 1
    order, count = np.full((B, keep), -1, np.int32), np.zeros((B,), np.int32)
    for b in range(B):
        a, e = int(coff[b]), int(coff[b + 1])
        if a < 0 or e < a or e > N or e - a > MAX_STARTS:
            count[b] = -1
            continue
        idx = np.nonzero(usable(loss[a:e], flags[a:e]))[0]
        l = np.asarray(loss[a:e], np.float64)[idx] + 0.0
        idx = idx[np.lexsort((idx, l))][:keep]
        count[b] = len(idx)
        order[b, :len(idx)] = a + idx
    return order, count


def fibonacci_codes(C):
    """sphere_codes(3, C) restated: z = 1 - (2 i + 1) / C, r = sqrt(1 - z z), phi = i pi (3 - sqrt(5)) in float64, rounded to float32 and
    normalised there"""
    i = np.arange(C, dtype=np.float64)
    z = 1.0 - (2.0 * i + 1.0) / C
    r = np.sqrt(1.0 - z * z)
    phi = i * (np.pi * (3.0 - np.sqrt(5.0)))
    c = np.stack([r * np.cos(phi), r * np.sin(phi), z], 1).astype(np.float32)
    return c / np.maximum(np.sqrt((c * c).sum(1, keepdims=True)), np.float32(1e-12))
