"""A numpy restatement of the shape encoder's three kernels (csrc/encode.hip, csrc/encode_cells.h, csrc/latent_cells.h; include/sdfr.h has the
contract), written from the header's comments.  TEST INFRASTRUCTURE ONLY: no device code.

The float64 sums follow the header's order (chunks of 1024 rows; 64 slots per chunk, slot j summing rows j, j + 64, ... in ascending order; the
slots folded by halves; chunk sums in chunk order) and the float32 steps are rounded where the kernels round them, so the kernels and the host
program tests/encode_host/encode_host.cpp must reproduce it bit for bit.  `ft` is the type of those float steps: np.float32 restates the
kernels, np.float64 gives the loop torch's float64 autograd and torch.optim.Adam run (tests/test_encode_cpu.py).
"""
import numpy as np

CHUNK, SLOTS = 1024, 64
MAX_L, MAX_K = 256, 1 << 20
EMPTY, NO_ROWS, SKIPPED, BAD_TABLE = 1, 2, 4, 8
GOLDEN = np.uint64(0x9E3779B97F4A7C15)


def mix64(z):
    """splitmix64's finaliser on uint64 arrays"""
    z = np.asarray(z, np.uint64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def mulhi64(a, b):
    """the upper 64 bits of the 128-bit product of uint64 arrays"""
    a, b = np.asarray(a, np.uint64), np.asarray(b, np.uint64)
    m, s = np.uint64(0xFFFFFFFF), np.uint64(32)
    al, ah, bl, bh = a & m, a >> s, b & m, b >> s
    with np.errstate(over="ignore"):
        t = al * bl
        u = ah * bl + (t >> s)
        w = al * bh + (u & m)
        return ah * bh + (u >> s) + (w >> s)


def draw(seed, it, b, s, count):
    """the sample (relative to the shape's first) rows s (array) of shape b take on iteration it"""
    s = np.asarray(s, np.uint64)
    key = (np.uint64(it) << np.uint64(40)) | (np.uint64(b) << np.uint64(24)) | s
    with np.errstate(over="ignore"):
        h = mix64(np.uint64(seed & 0xFFFFFFFFFFFFFFFF) ^ mix64(key * GOLDEN + np.uint64(1)))
    return mulhi64(h, np.uint64(count)).astype(np.int64)


def seq_sumsq(z, ft):
    ss = ft(0)
    for c in z:
        ss = ft(ss + ft(c * c))
    return ss


def latent_norm(z, ft=np.float32):
    """max(||z||, 1e-12), the squares summed in index order"""
    z = np.asarray(z, ft)
    return max(ft(np.sqrt(seq_sumsq(z, ft))), ft(1e-12))


def normalised(z, unit, ft=np.float32):
    z = np.asarray(z, ft)
    if not unit:
        return z.copy()
    return np.stack([zb / latent_norm(zb, ft) for zb in z]).astype(ft) if len(z) else z.copy()


def rows(samples, soff, B, k, draw_on, seed, it, z, unit, S=None, shape0=0):
    """sdfr_encode_rows: (inputs [B k][L + 3], target [B k], zn [B][L], flags [B])"""
    samples = np.asarray(samples, np.float32).reshape(-1, 4)
    S = len(samples) if S is None else S
    z = np.asarray(z, np.float32)
    L = z.shape[1]
    zn = normalised(z, unit)
    inputs = np.zeros((B * k, L + 3), np.float32)
    target = np.zeros((B * k,), np.float32)
    flags = np.zeros((B,), np.int32)
    for b in range(B):
        a, e = int(soff[b]), int(soff[b + 1])
        count = -1 if (a < 0 or e < a or e > S) else e - a
        if count < 0 or (not draw_on and count > 0 and k > count):
            flags[b] = BAD_TABLE
            continue
        if count == 0:
            flags[b] = EMPTY
            continue
        src = a + (draw(seed, it, shape0 + b, np.arange(k), count) if draw_on else np.arange(k))
        inputs[b * k:(b + 1) * k, :L] = zn[b]
        inputs[b * k:(b + 1) * k, L:] = samples[src, :3]
        target[b * k:(b + 1) * k] = samples[src, 3]
    return inputs, target, zn, flags


def row_rule(p, t, clamp):
    """(e float64, w float32, ok bool) per row"""
    p, t, c = np.asarray(p, np.float32), np.asarray(t, np.float32), np.float32(clamp)
    ok = np.isfinite(p) & np.isfinite(t)
    with np.errstate(invalid="ignore"):
        cp, ct = np.minimum(np.maximum(p, -c), c), np.minimum(np.maximum(t, -c), c)
        d = cp.astype(np.float64) - ct.astype(np.float64)
        w = np.where((p >= -c) & (p <= c), np.sign(d), 0.0)
    return np.where(ok, np.abs(d), 0.0), np.where(ok, w, 0.0).astype(np.float32), ok


def chunk_sum(vals):
    """the header's order on vals [n <= CHUNK][columns] float64"""
    n, nc = vals.shape
    acc = np.zeros((SLOTS, nc), np.float64)
    for r0 in range(0, n, SLOTS):
        m = min(SLOTS, n - r0)
        acc[:m] = acc[:m] + vals[r0:r0 + m]
    o = SLOTS // 2
    while o > 0:
        acc[:o] = acc[:o] + acc[o:2 * o]
        o //= 2
    return acc[0].copy()


def reduce(pred, target, J, L, B, k, clamp, flags):
    """sdfr_encode_reduce: (loss float64 [B], g_zn float64 [B][L], flags with bit 1 added, part [B][chunks][L + 2])"""
    J = np.asarray(J, np.float32)
    e, w, ok = row_rule(pred, target, clamp)
    with np.errstate(invalid="ignore", over="ignore"):
        terms = np.where(w[:, None] != 0, w[:, None].astype(np.float64) * J[:, :L].astype(np.float64), 0.0)
    vals = np.concatenate([terms, e[:, None], ok[:, None].astype(np.float64)], 1)
    chunks = (k + CHUNK - 1) // CHUNK
    part = np.zeros((B, chunks, L + 2), np.float64)
    loss, g = np.zeros((B,), np.float64), np.zeros((B, L), np.float64)
    flags = np.asarray(flags, np.int32).copy()
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(B):
            tot = np.zeros((L + 2,), np.float64)
            for ch in range(chunks):
                part[b, ch] = chunk_sum(vals[b * k + ch * CHUNK:b * k + min(k, (ch + 1) * CHUNK)])
                tot = tot + part[b, ch]
            n_ok = tot[L + 1]
            if n_ok > 0:
                loss[b], g[b] = tot[L] / n_ok, tot[:L] / n_ok
            else:
                flags[b] |= NO_ROWS
    return loss, g, flags, part


def bias(t, ft=np.float32):
    return ft(1.0 - 0.9 ** t), ft(1.0 - 0.999 ** t)


def step(z, m, v, g_zn, flags, unit, code_reg, lr, t, ft=np.float32):
    """sdfr_encode_step: (z, m, v, flags) after the update (copies)"""
    z, m, v = np.array(z, ft), np.array(m, ft), np.array(v, ft)
    flags = np.asarray(flags, np.int32).copy()
    B, L = z.shape
    bc1, bc2 = bias(t, ft)
    lr, code_reg = ft(np.float32(lr) if ft is np.float32 else lr), ft(np.float32(code_reg) if ft is np.float32 else code_reg)
    b1, b2, eps, omb2, one = ft(0.9), ft(0.999), ft(1e-8), ft(0.001), ft(1)
    with np.errstate(all="ignore"):
        for b in range(B):
            g = np.asarray(g_zn[b], np.float64).astype(ft)
            if unit:
                nrm = latent_norm(z[b], ft)
                dot = ft(0)
                for i in range(L):
                    dot = ft(dot + ft(ft(z[b, i] / nrm) * g[i]))
                gz = ((g - (z[b] / nrm) * dot) / nrm).astype(ft)
            else:
                nz = ft(np.sqrt(seq_sumsq(z[b], ft)))
                gz = (g + code_reg * (z[b] / nz)).astype(ft) if nz > 0 else g.copy()
            if (flags[b] & (EMPTY | NO_ROWS | BAD_TABLE)) or not np.isfinite(gz).all():
                flags[b] |= SKIPPED
                continue
            mb = (b1 * m[b] + (one - b1) * gz).astype(ft)
            vb = (b2 * v[b] + (omb2 * gz) * gz).astype(ft)
            denom = (np.sqrt(vb) / ft(np.sqrt(bc2)) + eps).astype(ft)
            z[b] = (z[b] - ft(lr / bc1) * (mb / denom)).astype(ft)
            m[b], v[b] = mb, vb
    return z, m, v, flags


def loop(decoder, samples, soff, z0, iters, k, draw_on, seed=0, lr=5e-3, lr_step=None, lr_factor=0.1, clamp=0.1, code_reg=1e-4, unit=True,
         ft=np.float32, watch=None, zs=None):
    """The whole fit with any decoder callable: decoder(inputs [n][L + 3]) -> (pred [n], J [n][>= L]).  Returns a dict with z (raw), zn (as
    the decoder sees the final z), history [iters][B] (float64 loss per iteration, before its step), flags of the last iteration.
    watch(it, inputs, pred, target, J): called per iteration (the trajectory test's kink margin); zs: a list that receives z after every step."""
    z = np.array(z0, ft)
    B, L = z.shape
    m, v = np.zeros_like(z), np.zeros_like(z)
    lr_step = max(1, iters // 2) if lr_step is None else lr_step
    hist = np.zeros((iters, B), np.float64)
    flags = np.zeros((B,), np.int32)
    for it in range(iters):
        inputs, target, _, flags = rows(samples, soff, B, k, draw_on, seed, it, z.astype(np.float32), unit)
        if ft is not np.float32:                    # the float64 loop: the latent columns without the float32 rounding
            inputs, zn = inputs.astype(ft), normalised(z, unit, ft)
            for b in range(B):
                if not flags[b]:
                    inputs[b * k:(b + 1) * k, :L] = zn[b]
        pred, J = decoder(inputs)
        if watch is not None:
            watch(it, inputs, pred, target, J)
        if ft is np.float32:
            loss, g, flags, _ = reduce(pred, target, J, L, B, k, clamp, flags)
        else:
            loss, g, flags = reduce64(pred, target, J, L, B, k, clamp, flags)
        hist[it] = loss
        z, m, v, flags = step(z, m, v, g, flags, unit, code_reg, lr * lr_factor ** (it // lr_step), it + 1, ft)
        if zs is not None:
            zs.append(z.copy())
    return {"z": z, "zn": normalised(z, unit, ft), "history": hist, "flags": flags, "m": m, "v": v}


def reduce64(pred, target, J, L, B, k, clamp, flags):
    """the reduce on float64 predictions (the float64 loop): the same rule without the float32 rounding of the clamped values"""
    p, t = np.asarray(pred, np.float64), np.asarray(target, np.float64)
    ok = np.isfinite(p) & np.isfinite(t)
    d = np.clip(p, -clamp, clamp) - np.clip(t, -clamp, clamp)
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
            flags[b] |= NO_ROWS
    return loss, g, flags
