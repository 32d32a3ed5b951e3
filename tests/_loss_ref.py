"""float64 references of the refinement loop's losses and solver step, written from the reference's formulas (pipelines/optimizer.py:13-52,
166-237): plain numpy, float64 arithmetic on the float32 inputs, no sklearn, no autograd.  Independent of oracle/sdf_oracle.py (which works in
float32 and is under test itself); tests/test_loss_refs_cpu.py ties them to the reference's recorded output (golden G12), to the oracle and to
torch.optim in float64.

Every search also returns, per rendered pixel / estimated point, its CANDIDATE SET: every distinct value whose distance lies within DELTA of
the minimum.  A float32 kernel may legitimately pick any member, so a kernel's gradient row is compared with the row of some member
(tests/test_gpu_losses.py); the share of rows with more than one member is bounded on the inputs themselves (test_loss_refs_cpu.py)."""
from types import SimpleNamespace

import numpy as np

DELTA = 1e-5          # absolute: the distances here are O(1); the project's float32 tolerance for these losses (test_gpu_batch.py)


def loss_2d_ref(rend, target, diam, threshold, delta=DELTA):
    """optimizer.py:200-237.  rend, target float32 (3, H, W).  For every rendered pixel (float32 channel sum != 0, :213) the smallest distance
    between its colour and target * clamp(diam - pixel distance, 0) over ALL pixels of the image (:224-233); "sum of indices" rule (:214);
    mean over the minima under the threshold, NaN if there are none (:234).
    Returns loss, nvalid, grad (3, H, W) and per rendered pixel q: ys, xs, mins (Q,), valid (Q,), cands[q] (k, 3) the distinct weighted-target
    values within delta of the minimum (the first is the argmin), rows[q] (k, 3) the gradient row d loss / d rend[:, y, x] of each.
    nvalid counts the minima under the threshold also where the index rule returns loss 0 (the reference never forms them there)."""
    r32 = np.asarray(rend, np.float32)
    H, W = r32.shape[1:]
    r = r32.astype(np.float64)
    t = np.asarray(target, np.float32).astype(np.float64).reshape(3, H * W)
    ys, xs = np.nonzero((r32[0] + r32[1]) + r32[2])                    # float32 sum over the channels, in torch's order
    Q = ys.size
    index_rule = bool(ys.sum() + xs.sum())                             # `if rendering_nonzero_idxs.sum():`  (:214)
    yy, xx = np.divmod(np.arange(H * W), W)
    mins = np.zeros(Q)
    cands, dists = [], []
    for q0 in range(0, Q, 256):
        y, x = ys[q0:q0 + 256], xs[q0:q0 + 256]
        w = np.maximum(diam - np.sqrt((yy[None] - y[:, None]) ** 2.0 + (xx[None] - x[:, None]) ** 2.0), 0.0)         # (q, HW)   :224-225
        m = t[None] * w[:, None, :]                                                                                 # (q, 3, HW) :227
        v = r[:, y, x].T                                                                                            # (q, 3)
        d = np.sqrt(((m - v[:, :, None]) ** 2).sum(1))                                                              # (q, HW)   :232
        a = d.argmin(1)
        dm = d[np.arange(y.size), a]
        mins[q0:q0 + 256] = dm
        near = d <= dm[:, None] + delta
        for i in range(y.size):
            if near[i].sum() == 1:
                cands.append(m[i, :, a[i]][None]); dists.append(dm[i:i + 1])
                continue
            idx = np.nonzero(near[i])[0]
            idx = np.concatenate([[a[i]], idx[idx != a[i]]])
            vals, first = np.unique(m[i][:, idx].T, axis=0, return_index=True)
            order = np.sort(first)                                       # distinct values, the argmin's first
            cands.append(m[i][:, idx[order]].T); dists.append(d[i, idx[order]])
    valid = mins < threshold
    nvalid = int(valid.sum())
    rows = []
    grad = np.zeros((3, H, W))
    for q in range(Q):
        if valid[q] and index_rule:
            with np.errstate(divide="ignore", invalid="ignore"):
                g = np.where(dists[q][:, None] > 0, (r[:, ys[q], xs[q]][None] - cands[q]) / dists[q][:, None], 0.0) / nvalid
        else:
            g = np.zeros_like(cands[q])
        rows.append(g)
        grad[:, ys[q], xs[q]] = g[0]
    if not index_rule:
        loss = 0.0                                                      # :235-236
    else:
        loss = float(mins[valid].mean()) if nvalid else float("nan")    # :234
    return SimpleNamespace(loss=loss, nvalid=nvalid, grad=grad, ys=ys, xs=xs, mins=mins, valid=valid, cands=cands, rows=rows,
                           index_rule=index_rule)


def loss_3d_ref(est, lidar, scale, threshold, delta=DELTA):
    """optimizer.py:166-198 with frustum = float32(lidar / scale) (:84).  est (ne, 3), lidar (nl, 3) float32.  Brute-force float64 distance
    matrix; pairs closer than threshold / scale (:188); mean pair distance (:193).
    Returns loss, npairs (-1 when a cloud is empty: the loop skips the crop, :127-129), g_est (ne, 3), g_scale and per estimated point: mins,
    paired, cand_idx[j] (k,) the lidar indices within delta of the minimum (the argmin first; several indices of one position are one
    candidate), rows[j] (k, 3) the gradient row of each and gs_rows[j] (k,) its term of d loss / d scale."""
    e32 = np.asarray(est, np.float32).reshape(-1, 3)
    l32 = np.asarray(lidar, np.float32).reshape(-1, 3)
    ne, nl = e32.shape[0], l32.shape[0]
    if ne == 0 or nl == 0:
        return SimpleNamespace(loss=0.0, npairs=-1, g_est=np.zeros((ne, 3)), g_scale=0.0, mins=np.zeros(ne), paired=np.zeros(ne, bool),
                               cand_idx=[np.zeros(0, int)] * ne, rows=[np.zeros((1, 3))] * ne, gs_rows=[np.zeros(1)] * ne, thr=0.0)
    s32 = np.float32(scale)
    s = float(s32)
    fr = (l32 / s32).astype(np.float32).astype(np.float64)              # :84
    e = e32.astype(np.float64)
    thr = float(threshold) / s                                          # :188
    mins = np.zeros(ne)
    cand_idx = []
    for j0 in range(0, ne, 512):
        d = np.sqrt(((e[j0:j0 + 512, None, :] - fr[None]) ** 2).sum(-1))
        a = d.argmin(1)
        dm = d[np.arange(d.shape[0]), a]
        mins[j0:j0 + 512] = dm
        near = d <= dm[:, None] + delta
        for i in range(d.shape[0]):
            if near[i].sum() == 1:
                cand_idx.append(a[i:i + 1])
                continue
            idx = np.nonzero(near[i])[0]
            idx = np.concatenate([[a[i]], idx[idx != a[i]]])
            _, first = np.unique(fr[idx], axis=0, return_index=True)
            cand_idx.append(idx[np.sort(first)])
    paired = mins < thr
    npairs = int(paired.sum())
    rows, gs_rows = [], []
    g_est = np.zeros((ne, 3))
    g_scale = 0.0
    for j in range(ne):
        k = cand_idx[j].size
        if not paired[j]:
            rows.append(np.zeros((k, 3))); gs_rows.append(np.zeros(k))
            continue
        f = fr[cand_idx[j]]
        diff = f - e[j][None]
        dd = np.sqrt((diff ** 2).sum(1))
        with np.errstate(divide="ignore", invalid="ignore"):
            u = np.where(dd[:, None] > 0, diff / dd[:, None], 0.0) / npairs   # d loss / d (frustum point)
        rows.append(-u)
        gs_rows.append((u * (-f / s)).sum(1))                           # d (lidar / scale) / d scale = -(lidar / scale) / scale
        g_est[j] = -u[0]
        g_scale += gs_rows[-1][0]
    loss = float(mins[paired].mean()) if npairs else 0.0                # :192-195
    return SimpleNamespace(loss=loss, npairs=npairs, g_est=g_est, g_scale=g_scale, mins=mins, paired=paired, cand_idx=cand_idx, rows=rows,
                           gs_rows=gs_rows, thr=thr)


def solver_ref(params, grads, L, loss2d, loss3d, npairs, w2, w3, m, v, t, lr_adam, lr_scale, lr_latent):
    """One MultipleOptimizer step (optimizer.py:13-52) for B crops, in float64, IN PLACE on params / m / v / t.
    params, grads: float64 flat [ yaw(B) | trans(B,3) | scale(B) | latent(B,L) ]; m, v float64 (B, 4); t int (B,).
    Adam (betas 0.9 / 0.999, eps 1e-8, bias corrections as torch.optim.Adam forms them) on yaw and trans, plain SGD on scale and latent.
    The loss of the skip rule is what the loop forms, in float32: w3 * loss3d + w2 * loss2d (:146); a crop with npairs < 0 (:127-129), a NaN
    or a zero total (:149-151) is skipped: its parameters, m, v and t stay untouched.  Returns total (float32, B) and stepped (B,)."""
    B = t.shape[0]
    total = np.float32(w3) * np.asarray(loss3d, np.float32) + np.float32(w2) * np.asarray(loss2d, np.float32)
    skip = (np.asarray(npairs) < 0) | np.isnan(total) | (total == 0)
    b1, b2, eps = 0.9, 0.999, 1e-8
    for b in np.nonzero(~skip)[0]:
        t[b] += 1
        bc1, bc2 = 1.0 - b1 ** int(t[b]), 1.0 - b2 ** int(t[b])
        at = [b, B + 3 * b, B + 3 * b + 1, B + 3 * b + 2]
        for i in range(4):
            g = grads[at[i]]
            m[b, i] = b1 * m[b, i] + (1.0 - b1) * g
            v[b, i] = b2 * v[b, i] + (1.0 - b2) * g * g
            denom = np.sqrt(v[b, i]) / np.sqrt(bc2) + eps
            params[at[i]] -= (lr_adam / bc1) * (m[b, i] / denom)
        params[4 * B + b] -= lr_scale * grads[4 * B + b]
        sl = slice(5 * B + b * L, 5 * B + (b + 1) * L)
        params[sl] -= lr_latent * grads[sl]
    return total, (~skip).astype(np.int32)


def match_rows(got, rows):
    """The acceptance rule of a gradient row: got (n, 3) against rows[i] (k_i, 3), the rows of the members of i's candidate set.
    Returns err (n,), the smallest max-abs difference to a member, and pick (n,), that member's position (0: the reference's own argmin)."""
    got = np.asarray(got, np.float64).reshape(-1, 3)
    err = np.zeros(got.shape[0])
    pick = np.zeros(got.shape[0], np.int64)
    for i, r in enumerate(rows):
        e = np.abs(r - got[i][None]).max(1)
        pick[i] = int(e.argmin())
        err[i] = e[pick[i]]
    return err, pick
