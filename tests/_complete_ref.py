"""A numpy restatement of shape completion from one view (csrc/complete.hip, csrc/complete_cells.h; include/sdfr.h has the contract), written
from the header's comments.  TEST INFRASTRUCTURE ONLY: no device code.

Three rules: the interval row rule (row_rule), the rows of one observed point (view_rows) and the interval fit's iteration (rows, reduce --
the summation order is tests/_encode_ref.py's -- and loop, which shares Adam with _encode_ref.step).  Float64 operations are numpy's, one
rounding each, in the order the header gives; `ft` as in _encode_ref.
"""
import numpy as np

from tests import _encode_ref as ER

BAD_POSE, BAD_TABLE = 4, 8
MAX_FREE = 64


def row_rule(p, lo, hi, clamp):
    """(e float64, w float32, ok bool) per row"""
    p, lo, hi, c = np.asarray(p, np.float32), np.asarray(lo, np.float32), np.asarray(hi, np.float32), np.float32(clamp)
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(p) & (lo <= hi) & (np.isfinite(lo) | np.isfinite(hi))
        cp, cl, ch = (np.minimum(np.maximum(v, -c), c) for v in (p, lo, hi))
        d = np.where(cp < cl, cp.astype(np.float64) - cl.astype(np.float64), np.where(cp > ch, cp.astype(np.float64) - ch.astype(np.float64), 0.0))
        w = np.where((p >= -c) & (p <= c), np.sign(d), 0.0)
    return np.where(ok, np.abs(d), 0.0), np.where(ok, w, 0.0).astype(np.float32), ok


def rows(samples, soff, B, k, draw_on, seed, it, z, unit, S=None, shape0=0):
    """sdfr_bound_rows: (inputs [B k][L + 3], lo [B k], hi [B k], zn [B][L], flags [B]): the encoder's rows, once per bound"""
    samples = np.asarray(samples, np.float32).reshape(-1, 5)
    S = len(samples) if S is None else S
    inputs, lo, zn, flags = ER.rows(samples[:, [0, 1, 2, 3]], soff, B, k, draw_on, seed, it, z, unit, S=S, shape0=shape0)
    _, hi, _, _ = ER.rows(samples[:, [0, 1, 2, 4]], soff, B, k, draw_on, seed, it, z, unit, S=S, shape0=shape0)
    return inputs, lo, hi, zn, flags


def reduce(pred, lo, hi, J, L, B, k, clamp, flags):
    """sdfr_bound_reduce: (loss float64 [B], g_zn float64 [B][L], flags with bit 1 added, part [B][chunks][L + 2])"""
    J = np.asarray(J, np.float32)
    e, w, ok = row_rule(pred, lo, hi, clamp)
    with np.errstate(invalid="ignore", over="ignore"):
        terms = np.where(w[:, None] != 0, w[:, None].astype(np.float64) * J[:, :L].astype(np.float64), 0.0)
    vals = np.concatenate([terms, e[:, None], ok[:, None].astype(np.float64)], 1)
    chunks = (k + ER.CHUNK - 1) // ER.CHUNK
    part = np.zeros((B, chunks, L + 2), np.float64)
    loss, g = np.zeros((B,), np.float64), np.zeros((B, L), np.float64)
    flags = np.asarray(flags, np.int32).copy()
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(B):
            tot = np.zeros((L + 2,), np.float64)
            for ch in range(chunks):
                part[b, ch] = ER.chunk_sum(vals[b * k + ch * ER.CHUNK:b * k + min(k, (ch + 1) * ER.CHUNK)])
                tot = tot + part[b, ch]
            n_ok = tot[L + 1]
            if n_ok > 0:
                loss[b], g[b] = tot[L] / n_ok, tot[:L] / n_ok
            else:
                flags[b] |= ER.NO_ROWS
    return loss, g, flags, part


def reduce64(pred, lo, hi, J, L, B, k, clamp, flags):
    """the reduce on float64 predictions (the float64 loop): the same rule without the float32 rounding of the clamped values"""
    p, lo, hi = np.asarray(pred, np.float64), np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(p) & (lo <= hi) & (np.isfinite(lo) | np.isfinite(hi))
        cp, cl, ch = np.clip(p, -clamp, clamp), np.clip(lo, -clamp, clamp), np.clip(hi, -clamp, clamp)
        d = np.where(cp < cl, cp - cl, np.where(cp > ch, cp - ch, 0.0))
        w = np.where(ok & (p >= -clamp) & (p <= clamp), np.sign(d), 0.0)
    loss, g = np.zeros((B,)), np.zeros((B, L))
    flags = np.asarray(flags, np.int32).copy()
    for b in range(B):
        sl = slice(b * k, (b + 1) * k)
        n = ok[sl].sum()
        if n > 0:
            loss[b] = np.where(ok[sl], np.abs(d[sl]), 0.0).sum() / n
            g[b] = (w[sl, None] * np.asarray(J, np.float64)[sl, :L]).sum(0) / n
        else:
            flags[b] |= ER.NO_ROWS
    return loss, g, flags


def loop(decoder, samples, soff, z0, iters, k, draw_on, seed=0, lr=5e-3, lr_step=None, lr_factor=0.1, clamp=0.1, code_reg=1e-4, unit=True,
         ft=np.float32, watch=None, zs=None):
    """_encode_ref.loop for interval samples [S][5]; watch(it, inputs, pred, lo, hi, J)"""
    z = np.array(z0, ft)
    B, L = z.shape
    m, v = np.zeros_like(z), np.zeros_like(z)
    lr_step = max(1, iters // 2) if lr_step is None else lr_step
    hist = np.zeros((iters, B), np.float64)
    flags = np.zeros((B,), np.int32)
    for it in range(iters):
        inputs, lo, hi, _, flags = rows(samples, soff, B, k, draw_on, seed, it, z.astype(np.float32), unit)
        if ft is not np.float32:
            inputs, zn = inputs.astype(ft), ER.normalised(z, unit, ft)
            for b in range(B):
                if not flags[b]:
                    inputs[b * k:(b + 1) * k, :L] = zn[b]
        pred, J = decoder(inputs)
        if watch is not None:
            watch(it, inputs, pred, lo, hi, J)
        if ft is np.float32:
            loss, g, flags, _ = reduce(pred, lo, hi, J, L, B, k, clamp, flags)
        else:
            loss, g, flags = reduce64(pred, lo, hi, J, L, B, k, clamp, flags)
        hist[it] = loss
        z, m, v, flags = ER.step(z, m, v, g, flags, unit, code_reg, lr * lr_factor ** (it // lr_step), it + 1, ft)
        if zs is not None:
            zs.append(z.copy())
    return {"z": z, "zn": ER.normalised(z, unit, ft), "history": hist, "flags": flags, "m": m, "v": v}


# ---- the rows of a view ----------------------------------------------------------------------------------------------------------------------

def table_ok(ptoff, b, N):
    a, e = int(ptoff[b]), int(ptoff[b + 1])
    return a >= 0 and e >= a and e <= N


def pose_ok(pose_b):
    return bool(np.isfinite(pose_b).all() and pose_b[5] > 0)


def owner(ptoff, B, N, g):
    """the binary search of verify_owner on the table as it is, then the check of the entry found; -1 without an owner"""
    if B < 1:
        return -1
    lo, hi = 0, B
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if int(ptoff[mid]) <= g:
            lo = mid
        else:
            hi = mid
    return lo if table_ok(ptoff, lo, N) and int(ptoff[lo]) <= g < int(ptoff[lo + 1]) else -1


def u_of(seed, shape, i, f):
    """u in [0, 1) of slots f (array) of point i of shape `shape`"""
    f = np.asarray(f, np.uint64)
    key = (np.uint64(shape) << np.uint64(40)) | (np.uint64(i) << np.uint64(8)) | f
    with np.errstate(over="ignore"):
        h = ER.mix64(np.uint64(seed & 0xFFFFFFFFFFFFFFFF) ^ ER.mix64(key * ER.GOLDEN + np.uint64(1)))
    return (h >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def lattice_x(p, pose_b):
    """x = diag(1, -1, 1) rot_yaw^T (p / scale - trans) in float64, one rounding per operation: verify_point_x before its rounding"""
    p, q = np.asarray(p, np.float32).astype(np.float64), np.asarray(pose_b, np.float32).astype(np.float64)
    c, s, sc = q[0], q[1], q[5]
    q0, q1, q2 = p[0] / sc - q[2], p[1] / sc - q[3], p[2] / sc - q[4]
    return np.array([c * q0 - s * q2, -q1, s * q0 + c * q2])


def _slot(valid, x, lo, hi):
    f = np.asarray(x, np.float64).astype(np.float32)
    with np.errstate(invalid="ignore"):
        ok = bool(valid) and bool((np.abs(f) <= 1).all())
    if not ok:
        return np.array([0, 0, 0, np.nan, np.nan], np.float32)
    return np.array([f[0], f[1], f[2], np.float32(lo), np.float32(hi)], np.float32)


def view_rows(points, normals, ptoff, pose, origin, F, eta, s_max, seed, shape0=0, N=None):
    """sdfr_view_samples: (rows float32 [N (3 + F)][5], flags int32 [B])"""
    points = np.asarray(points, np.float32).reshape(-1, 3)
    N = len(points) if N is None else N
    pose = np.asarray(pose, np.float32).reshape(-1, 6)
    B = len(pose)
    eta, s_max = float(np.float32(eta)), float(np.float32(s_max))              # the C ABI takes them as float32
    P = 3 + F
    out = np.zeros((N * P, 5), np.float32)
    flags = np.array([BAD_TABLE if not table_ok(ptoff, b, N) else (0 if pose_ok(pose[b]) else BAD_POSE) for b in range(B)], np.int32).reshape(B)
    fe = np.float32(eta)
    with np.errstate(all="ignore"):
        for g in range(N):
            b = owner(ptoff, B, N, g)
            blk = out[g * P:(g + 1) * P]
            if b < 0 or not pose_ok(pose[b]):
                blk[:] = _slot(False, np.zeros(3), 0, 0)
                continue
            i = g - int(ptoff[b])
            x, o = lattice_x(points[g], pose[b]), lattice_x(origin, pose[b])
            blk[0] = _slot(True, x, 0, 0)
            n_ok, nh = False, np.zeros(3)
            if normals is not None:
                n = np.asarray(normals[g], np.float64)
                c, s = np.float64(pose[b, 0]), np.float64(pose[b, 1])
                m = np.array([c * n[0] - s * n[2], -n[1], s * n[0] + c * n[2]])
                ln = np.sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2])
                n_ok = bool(np.isfinite(ln) and ln > 0)
                if n_ok:
                    nh = m / ln
            blk[1] = _slot(n_ok, x + eta * nh, fe, fe)
            blk[2] = _slot(n_ok, x - eta * nh, -fe, -fe)
            d = x - o
            r = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
            r_ok = bool(np.isfinite(r) and r > 0)
            dh = d / r if r_ok else np.zeros(3)
            reach = np.fmin(s_max, r)
            if F:
                u = u_of(seed, shape0 + b, i, np.arange(F))
                s = ((np.arange(F, dtype=np.float64) + u) / np.float64(F)) * reach
                for f in range(F):
                    blk[3 + f] = _slot(r_ok, x - s[f] * dh, 0, s[f])
    return out, flags
