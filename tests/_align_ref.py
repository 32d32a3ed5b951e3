"""A numpy restatement of the pose-and-shape fit to one view (csrc/align.hip, csrc/align_cells.h; include/sdfr.h has the contract), written
from the header's comments.  TEST INFRASTRUCTURE ONLY: no device code.

Four rules: the camera-frame observation rows of one point (sample_rows), the iteration's rows under a pose (rows), the loss and the gradient
with respect to latent, yaw, trans and scale (reduce -- the summation order is tests/_encode_ref.py's) and the update (step).  loop chains
them around any decoder callable.  Float64 operations are numpy's, one rounding each, in the order the header gives.  `ft` as in
_encode_ref: np.float32 restates the kernels, np.float64 gives the loop torch's float64 autograd and torch.optim.Adam run.
"""
import numpy as np

from tests import _complete_ref as CR
from tests import _encode_ref as ER

BAD_POSE = 16
POSE = 5                                   # yaw tx ty tz scale
NO_STEP = ER.EMPTY | ER.NO_ROWS | ER.BAD_TABLE | BAD_POSE


# ---- the observation rows ------------------------------------------------------------------------------------------------------------------

def _slot(valid, q, lo, hi):
    with np.errstate(over="ignore", invalid="ignore"):
        f = np.asarray(q, np.float64).astype(np.float32)
    if not (bool(valid) and bool(np.isfinite(f).all())):
        return np.array([0, 0, 0, np.nan, np.nan], np.float32)
    return np.array([f[0], f[1], f[2], np.float32(lo), np.float32(hi)], np.float32)


def sample_rows(points, normals, ptoff, origin, F, eta, s_max, seed, shape0=0, N=None):
    """sdfr_align_samples: (rows float32 [N (3 + F)][5], flags int32 [B])"""
    points = np.asarray(points, np.float32).reshape(-1, 3)
    N = len(points) if N is None else N
    B = len(ptoff) - 1
    eta, s_max = float(np.float32(eta)), float(np.float32(s_max))              # the C ABI takes them as float32
    P = 3 + F
    out = np.zeros((N * P, 5), np.float32)
    flags = np.array([0 if CR.table_ok(ptoff, b, N) else CR.BAD_TABLE for b in range(B)], np.int32).reshape(B)
    fe = np.float32(eta)
    o = np.asarray(origin, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        for g in range(N):
            b = CR.owner(ptoff, B, N, g)
            blk = out[g * P:(g + 1) * P]
            if b < 0 or not np.isfinite(points[g]).all():
                blk[:] = _slot(False, np.zeros(3), 0, 0)
                continue
            i = g - int(ptoff[b])
            x = points[g].astype(np.float64)
            blk[0] = _slot(True, x, 0, 0)
            n_ok, nh = False, np.zeros(3)
            if normals is not None:
                n = np.asarray(normals[g], np.float64)
                ln = np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
                n_ok = bool(np.isfinite(ln) and ln > 0)
                if n_ok:
                    nh = n / ln
            blk[1] = _slot(n_ok, x + eta * nh, fe, fe)
            blk[2] = _slot(n_ok, x - eta * nh, -fe, -fe)
            d = x - o
            r = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
            r_ok = bool(np.isfinite(r) and r > 0)
            dh = d / r if r_ok else np.zeros(3)
            reach = np.fmin(s_max, r)
            if F:
                u = CR.u_of(seed, shape0 + b, i, np.arange(F))
                s = ((np.arange(F, dtype=np.float64) + u) / np.float64(F)) * reach
                for f in range(F):
                    blk[3 + f] = _slot(r_ok, x - s[f] * dh, 0, s[f])
    return out, flags


# ---- the iteration's rows ------------------------------------------------------------------------------------------------------------------

def lattice_x(q, pose):
    """x = diag(1, -1, 1) rot_yaw^T (q / scale - trans) in float64 for q [n][3] and pose [6] or [n][6], one rounding per operation, in the
    order of verify_point_x64"""
    q, p = np.asarray(q).astype(np.float64), np.asarray(pose).astype(np.float64)
    p = p if p.ndim == 2 else p[None]
    c, s, sc = p[:, 0], p[:, 1], p[:, 5]
    with np.errstate(all="ignore"):
        q0, q1, q2 = q[:, 0] / sc - p[:, 2], q[:, 1] / sc - p[:, 3], q[:, 2] / sc - p[:, 4]
        return np.stack([c * q0 - s * q2, -q1, s * q0 + c * q2], 1)


def pose_row(theta, ft=np.float32):
    """the pose rows [B][6] of theta [B][5]: cos and sin in double of the yaw, rounded once to ft"""
    theta = np.asarray(theta, ft).reshape(-1, POSE)
    y = theta[:, 0].astype(np.float64)
    return np.concatenate([np.cos(y).astype(ft)[:, None], np.sin(y).astype(ft)[:, None], theta[:, 1:]], 1).astype(ft)


def pose_ok(pose_b):
    return bool(np.isfinite(pose_b).all() and pose_b[5] > 0)


def rows(samples, soff, B, k, draw_on, seed, it, z, unit, pose, S=None, shape0=0):
    """sdfr_align_rows: (inputs [B k][L + 3], cam [B k][3], lo [B k], hi [B k], zn [B][L], flags [B])"""
    pose = np.asarray(pose, np.float32).reshape(B, 6)
    inputs, lo, hi, zn, flags = CR.rows(samples, soff, B, k, draw_on, seed, it, z, unit, S=S, shape0=shape0)
    L = zn.shape[1]
    cam = inputs[:, L:].copy()
    for b in range(B):
        if flags[b]:
            continue
        sl = slice(b * k, (b + 1) * k)
        if not pose_ok(pose[b]):
            flags[b] = BAD_POSE
            inside = np.zeros((k,), bool)
            x = np.zeros((k, 3), np.float32)
        else:
            with np.errstate(over="ignore", invalid="ignore"):
                x = lattice_x(cam[sl], pose[b]).astype(np.float32)
                inside = (np.abs(x) <= 1).all(1)
        inputs[sl, L:] = np.where(inside[:, None], x, np.float32(0))
        lo[sl], hi[sl] = np.where(inside, lo[sl], np.float32(np.nan)), np.where(inside, hi[sl], np.float32(np.nan))
    return inputs, cam, lo, hi, zn, flags


# ---- loss and gradient -----------------------------------------------------------------------------------------------------------------------

def dpm(pred, J, cam, pose, L):
    """d pm / d (zn, yaw, tx, ty, tz, scale) [n][L + 5] in float64 for pose [n][6], each operation as align_cells.h writes it"""
    p, J, q, ps = (np.asarray(a).astype(np.float64) for a in (pred, J, cam, pose))
    c, sn, sc = ps[:, 0], ps[:, 1], ps[:, 5]
    gx, gy, gz = J[:, L], J[:, L + 1], J[:, L + 2]
    with np.errstate(all="ignore"):
        x = lattice_x(q, ps)
        lat = sc[:, None] * J[:, :L]
        yaw = sc * (gz * x[:, 0] - gx * x[:, 2])
        tx = -(sc * (gx * c + gz * sn))
        ty = sc * gy
        tz = sc * (gx * sn - gz * c)
        s2 = sc * sc
        u0, u1, u2 = -(q[:, 0] / s2), -(q[:, 1] / s2), -(q[:, 2] / s2)
        t0, t1, t2 = gx * (c * u0 - sn * u2), gy * u1, gz * (sn * u0 + c * u2)
        scl = p + sc * ((t0 - t1) + t2)
    return np.concatenate([lat, np.stack([yaw, tx, ty, tz, scl], 1)], 1)


def reduce(pred, lo, hi, J, cam, pose, L, B, k, clamp, flags):
    """sdfr_align_reduce: (loss float64 [B], g float64 [B][L + 5], flags with bit 1 added, part [B][chunks][L + 7])"""
    pred, J, pose = np.asarray(pred, np.float32), np.asarray(J, np.float32), np.asarray(pose, np.float32).reshape(B, 6)
    per_row = np.repeat(pose, k, 0)
    with np.errstate(all="ignore"):
        pm = (per_row[:, 5] * pred).astype(np.float32)
        e, w, ok = CR.row_rule(pm, lo, hi, clamp)
        terms = np.where(w[:, None] != 0, w[:, None].astype(np.float64) * dpm(pred, J, cam, per_row, L), 0.0)
    G = L + POSE
    vals = np.concatenate([terms, e[:, None], ok[:, None].astype(np.float64)], 1)
    chunks = (k + ER.CHUNK - 1) // ER.CHUNK
    part = np.zeros((B, chunks, G + 2), np.float64)
    loss, g = np.zeros((B,), np.float64), np.zeros((B, G), np.float64)
    flags = np.asarray(flags, np.int32).copy()
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(B):
            tot = np.zeros((G + 2,), np.float64)
            for ch in range(chunks):
                part[b, ch] = ER.chunk_sum(vals[b * k + ch * ER.CHUNK:b * k + min(k, (ch + 1) * ER.CHUNK)])
                tot = tot + part[b, ch]
            n_ok = tot[G + 1]
            if n_ok > 0:
                loss[b], g[b] = tot[G] / n_ok, tot[:G] / n_ok
            else:
                flags[b] |= ER.NO_ROWS
    return loss, g, flags, part


def reduce64(pred, lo, hi, J, cam, pose, L, B, k, clamp, flags):
    """the reduce of the float64 loop: float64 predictions and pose [B][6], no float32 rounding anywhere, plain sums"""
    pose = np.asarray(pose, np.float64).reshape(B, 6)
    per_row = np.repeat(pose, k, 0)
    p, lo, hi = per_row[:, 5] * np.asarray(pred, np.float64), np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(p) & (lo <= hi) & (np.isfinite(lo) | np.isfinite(hi))
        cp, cl, ch = np.clip(p, -clamp, clamp), np.clip(lo, -clamp, clamp), np.clip(hi, -clamp, clamp)
        d = np.where(cp < cl, cp - cl, np.where(cp > ch, cp - ch, 0.0))
        w = np.where(ok & (p >= -clamp) & (p <= clamp), np.sign(d), 0.0)
        D = np.where(w[:, None] != 0, w[:, None] * dpm(pred, J, cam, per_row, L), 0.0)
    loss, g = np.zeros((B,)), np.zeros((B, L + POSE))
    flags = np.asarray(flags, np.int32).copy()
    for b in range(B):
        sl = slice(b * k, (b + 1) * k)
        n = ok[sl].sum()
        if n > 0:
            loss[b] = np.where(ok[sl], np.abs(d[sl]), 0.0).sum() / n
            g[b] = D[sl].sum(0) / n
        else:
            flags[b] |= ER.NO_ROWS
    return loss, g, flags


# ---- the update --------------------------------------------------------------------------------------------------------------------------------

def adam(p, m, v, g, lr, bc1, bc2, ft):
    """latent_adam on arrays: (p, m, v) after the update"""
    b1, b2, eps, omb2, one = ft(0.9), ft(0.999), ft(1e-8), ft(0.001), ft(1)
    with np.errstate(all="ignore"):
        mb = (b1 * m + (one - b1) * g).astype(ft)
        vb = (b2 * v + (omb2 * g) * g).astype(ft)
        denom = (np.sqrt(vb) / ft(np.sqrt(bc2)) + eps).astype(ft)
        return (p - ft(lr / bc1) * (mb / denom)).astype(ft), mb, vb


def step(z, m, v, theta, tm, tv, pose, g, flags, unit, code_reg, lr, lr_pose, t, ft=np.float32):
    """sdfr_align_step: (z, m, v, theta, tm, tv, pose, flags) after the update (copies).  g [B][L + 5] float64."""
    z, m, v, theta, tm, tv, pose = (np.array(a, ft) for a in (z, m, v, theta, tm, tv, pose))
    flags = np.asarray(flags, np.int32).copy()
    B, L = z.shape
    bc1, bc2 = ER.bias(t, ft)
    f32 = ft is np.float32
    lr, code_reg = ft(np.float32(lr) if f32 else lr), ft(np.float32(code_reg) if f32 else code_reg)
    lr_pose = [ft(np.float32(r) if f32 else r) for r in lr_pose]
    with np.errstate(all="ignore"):
        for b in range(B):
            gl, gp = np.asarray(g[b, :L], np.float64).astype(ft), np.asarray(g[b, L:], np.float64).astype(ft)
            if unit:
                nrm = ER.latent_norm(z[b], ft)
                dot = ft(0)
                for i in range(L):
                    dot = ft(dot + ft(ft(z[b, i] / nrm) * gl[i]))
                gz = ((gl - (z[b] / nrm) * dot) / nrm).astype(ft)
            else:
                nz = ft(np.sqrt(ER.seq_sumsq(z[b], ft)))
                gz = (gl + code_reg * (z[b] / nz)).astype(ft) if nz > 0 else gl.copy()
            sc = adam(theta[b, 4], tm[b, 4], tv[b, 4], gp[4], lr_pose[4], bc1, bc2, ft)[0] if lr_pose[4] != 0 else theta[b, 4]
            if (flags[b] & NO_STEP) or not np.isfinite(gz).all() or not np.isfinite(gp).all() or not (np.isfinite(sc) and sc > 0):
                flags[b] |= ER.SKIPPED
                continue
            if lr != 0:
                z[b], m[b], v[b] = adam(z[b], m[b], v[b], gz, lr, bc1, bc2, ft)
            for i in range(POSE):
                if lr_pose[i] != 0:
                    theta[b, i], tm[b, i], tv[b, i] = adam(theta[b, i], tm[b, i], tv[b, i], gp[i], lr_pose[i], bc1, bc2, ft)
            pose[b] = pose_row(theta[b], ft)[0]
    return z, m, v, theta, tm, tv, pose, flags


# ---- the loop ----------------------------------------------------------------------------------------------------------------------------------

def loop(decoder, samples, soff, z0, theta0, iters, k, draw_on, seed=0, lr=5e-3, lr_pose=(1e-2,) * POSE, lr_step=None, lr_factor=0.1, clamp=0.2,
         code_reg=1e-4, unit=True, ft=np.float32, watch=None, trace=None):
    """The whole fit with any decoder callable: decoder(inputs [n][L + 3]) -> (pred [n], J [n][L + 3]).  Returns a dict with z (raw), zn,
    theta, pose, history [iters][B] (the loss per iteration, before its step), flags of the last iteration and the Adam states.
    watch(it, inputs, pred, lo, hi, J, pose): called per iteration; trace: a list that receives (z, theta) after every step."""
    z, theta = np.array(z0, ft), np.array(theta0, ft).reshape(-1, POSE)
    B, L = z.shape
    m, v, tm, tv = np.zeros_like(z), np.zeros_like(z), np.zeros_like(theta), np.zeros_like(theta)
    pose = pose_row(theta, ft)
    lr_step = max(1, iters // 2) if lr_step is None else lr_step
    hist = np.zeros((iters, B), np.float64)
    flags = np.zeros((B,), np.int32)
    for it in range(iters):
        inputs, cam, lo, hi, _, flags = rows(samples, soff, B, k, draw_on, seed, it, z.astype(np.float32), unit, pose.astype(np.float32))
        if ft is not np.float32:                    # the float64 loop: latent columns, positions and the cube test without the float32 rounding
            inputs, zn = inputs.astype(ft), ER.normalised(z, unit, ft)
            _, lo, hi, _, _ = CR.rows(samples, soff, B, k, draw_on, seed, it, z.astype(np.float32), unit)
            for b in range(B):
                if flags[b]:
                    continue
                sl = slice(b * k, (b + 1) * k)
                x = lattice_x(cam[sl], pose[b])
                inside = (np.abs(x) <= 1).all(1)
                inputs[sl, :L], inputs[sl, L:] = zn[b], np.where(inside[:, None], x, 0.0)
                lo[sl], hi[sl] = np.where(inside, lo[sl], np.nan), np.where(inside, hi[sl], np.nan)
        pred, J = decoder(inputs)
        if watch is not None:
            watch(it, inputs, pred, lo, hi, J, pose)
        if ft is np.float32:
            loss, g, flags, _ = reduce(pred, lo, hi, J, cam, pose, L, B, k, clamp, flags)
        else:
            loss, g, flags = reduce64(pred, lo, hi, J, cam, pose, L, B, k, clamp, flags)
        hist[it] = loss
        f = lr_factor ** (it // lr_step)
        z, m, v, theta, tm, tv, pose, flags = step(z, m, v, theta, tm, tv, pose, g, flags, unit, code_reg, lr * f, [r * f for r in lr_pose], it + 1, ft)
        if trace is not None:
            trace.append((z.copy(), theta.copy()))
    return {"z": z, "zn": ER.normalised(z, unit, ft), "theta": theta, "pose": pose, "history": hist, "flags": flags, "m": m, "v": v, "tm": tm, "tv": tv}
