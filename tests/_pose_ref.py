"""Two references of the RANSAC pose initialisation (csrc/pose.hip, csrc/pose_cells.h, csrc/jacobi3.h).

(a) `fit_mp`, `colour_nn_brute`, `score_brute`: the OPERATIONS, independent of the kernel's algorithm.  The fit is Kabsch / Umeyama through
    an SVD of H itself, R = U diag(1, 1, det(U V^T)) V^T, in mpmath at 50 digits; the nearest neighbours are brute force in float64 and the
    inlier decisions carry their distance to the threshold.
(b) `restate`: pose_cells.h again in numpy float32 / float64 and Python integers, the same operations in the same order: the first-index
    tie rules, the 256-lane trees of rs_block_sum and rs_select_kernel, the block-stride accumulation of the final fit, the ballot-order
    compaction into plist.  The host build of pose_cells.h (tests/pose_host) and the GPU kernels must equal it bit for bit.
The float32 fused multiply-adds of the scoring search are evaluated exactly: a float64 evaluation is kept only where it is provably the
single rounding (see `fma32`), the remaining candidates go through rational arithmetic and are counted in FMA_EXACT.
"""
import struct
from fractions import Fraction

import numpy as np

f32, f64 = np.float32, np.float64
TPB, HG = 256, 8
U32, U64 = 2.0 ** -24, 2.0 ** -53
EPS32 = 1.1920928955078125e-07
FMA_EXACT = {"candidates": 0, "exact_path": 0}


# ---- (b) the restatement ------------------------------------------------------------------------------------------------------------------

def store(x, f16):
    """a float64 value stored in the numpy dtype of its array and read back (rs_round)"""
    x = np.asarray(x, f64).astype(f32)
    return (x.astype(np.float16) if f16 else x).astype(f64)


def jacobi3(S):
    """sdfr_jacobi3: S [3][3] float64 -> lam (descending), V (eigenvectors as columns)"""
    S = [[f64(S[i][j]) for j in range(3)] for i in range(3)]
    V = [[f64(1.0 if i == j else 0.0) for j in range(3)] for i in range(3)]
    one = f64(1.0)
    big, unscale = f64(0.0), one
    for i in range(3):
        for j in range(i, 3):
            big = np.abs(S[i][j]) if np.abs(S[i][j]) > big else big
    if big > 0.0 and (big < 1e-100 or big > 1e100) and big <= 1.7976931348623157e308:          # an exact power of two brings it to [1, 2)
        e = min(1000, -(int(np.frexp(big)[1]) - 1))
        sc, unscale = np.ldexp(one, e), np.ldexp(one, -e)
        S = [[S[i][j] * sc for j in range(3)] for i in range(3)]
    for _ in range(32):
        off = S[0][1] * S[0][1] + S[0][2] * S[0][2] + S[1][2] * S[1][2]
        dia = S[0][0] * S[0][0] + S[1][1] * S[1][1] + S[2][2] * S[2][2]
        if not (off > f64(1e-36) * dia):
            break
        for p in range(2):
            for q in range(p + 1, 3):
                apq = S[p][q]
                if apq == 0.0:
                    continue
                theta = (S[q][q] - S[p][p]) / (f64(2.0) * apq)
                tt = (one if theta >= 0.0 else -one) / (np.abs(theta) + np.sqrt(theta * theta + one))
                c = one / np.sqrt(tt * tt + one)
                s = tt * c
                for k in range(3):
                    skp, skq = S[k][p], S[k][q]
                    S[k][p] = c * skp - s * skq
                    S[k][q] = s * skp + c * skq
                for k in range(3):
                    spk, sqk = S[p][k], S[q][k]
                    S[p][k] = c * spk - s * sqk
                    S[q][k] = s * spk + c * sqk
                for k in range(3):
                    vkp, vkq = V[k][p], V[k][q]
                    V[k][p] = c * vkp - s * vkq
                    V[k][q] = s * vkp + c * vkq
    o = [0, 1, 2]
    for i in range(2):
        for j in range(2 - i):
            if S[o[j]][o[j]] < S[o[j + 1]][o[j + 1]]:
                o[j], o[j + 1] = o[j + 1], o[j]
    lam = np.array([S[o[i]][o[i]] * unscale for i in range(3)], f64)
    return lam, np.array([[V[k][o[i]] for i in range(3)] for k in range(3)], f64)


def rs_fit(H, mf, mt, sig, typ, info=None):
    """rs_fit: returns (ok, R, c, t, ratio); info (a dict) receives detV"""
    z = f64(0.0)
    H = [[f64(H[i][j]) for j in range(3)] for i in range(3)]
    mf, mt, sig = [f64(v) for v in mf], [f64(v) for v in mt], f64(sig)
    S = [[H[0][i] * H[0][j] + H[1][i] * H[1][j] + H[2][i] * H[2][j] for j in range(3)] for i in range(3)]
    lam, V = jacobi3(S)
    s1, s2 = np.sqrt(lam[0] if lam[0] > 0.0 else z), np.sqrt(lam[1] if lam[1] > 0.0 else z)
    U = [[z, z, z] for _ in range(3)]
    for k in range(2):
        for i in range(3):
            U[i][k] = H[i][0] * V[0][k] + H[i][1] * V[1][k] + H[i][2] * V[2][k]
    n1 = np.sqrt(U[0][0] * U[0][0] + U[1][0] * U[1][0] + U[2][0] * U[2][0])
    if not (n1 > 0.0):
        U[0][0], U[1][0], U[2][0], n1 = f64(1.0), z, z, f64(1.0)
    for i in range(3):
        U[i][0] = U[i][0] / n1
    d12 = U[0][0] * U[0][1] + U[1][0] * U[1][1] + U[2][0] * U[2][1]
    for i in range(3):
        U[i][1] = U[i][1] - d12 * U[i][0]
    n2 = np.sqrt(U[0][1] * U[0][1] + U[1][1] * U[1][1] + U[2][1] * U[2][1])
    if not (n2 > 1e-300):
        a = 0 if np.abs(U[0][0]) < 0.6 else 1
        e = [z, z, z]
        e[a] = f64(1.0)
        d = e[0] * U[0][0] + e[1] * U[1][0] + e[2] * U[2][0]
        for i in range(3):
            U[i][1] = e[i] - d * U[i][0]
        n2 = np.sqrt(U[0][1] * U[0][1] + U[1][1] * U[1][1] + U[2][1] * U[2][1])
    for i in range(3):
        U[i][1] = U[i][1] / n2
    U[0][2] = U[1][0] * U[2][1] - U[2][0] * U[1][1]
    U[1][2] = U[2][0] * U[0][1] - U[0][0] * U[2][1]
    U[2][2] = U[0][0] * U[1][1] - U[1][0] * U[0][1]
    detV = (V[0][0] * (V[1][1] * V[2][2] - V[1][2] * V[2][1]) - V[0][1] * (V[1][0] * V[2][2] - V[1][2] * V[2][0]) +
            V[0][2] * (V[1][0] * V[2][1] - V[1][1] * V[2][0]))
    if info is not None:
        info["detV"] = float(detV)
    sv = f64(-1.0) if detV < 0.0 else f64(1.0)
    R = [[U[i][0] * V[j][0] + U[i][1] * V[j][1] + sv * U[i][2] * V[j][2] for j in range(3)] for i in range(3)]
    ratio = s2 / s1 if s1 > 0.0 else z
    t = [z, z, z]
    if typ == 1:
        if not (s2 > s1 * f64(3.0) * f64(EPS32)):
            return False, np.array(R, f64), z, np.array(t, f64), ratio
        hv = [H[i][0] * V[0][2] + H[i][1] * V[1][2] + H[i][2] * V[2][2] for i in range(3)]
        s3 = U[0][2] * hv[0] + U[1][2] * hv[1] + U[2][2] * hv[2]
        c = (s1 + s2 + sv * s3) / sig
        for i in range(3):
            t[i] = mt[i] - c * (R[i][0] * mf[0] + R[i][1] * mf[1] + R[i][2] * mf[2])
    else:
        c = f64(1.0)
        for i in range(3):
            a = R[i][0] * (mt[0] - mf[0]) + R[i][1] * (mt[1] - mf[1]) + R[i][2] * (mt[2] - mf[2])
            bb = R[i][0] * mt[0] + R[i][1] * mt[1] + R[i][2] * mt[2]
            t[i] = a - bb + mt[i]
    return True, np.array(R, f64), c, np.array(t, f64), ratio


def sample_moments(fp, tp, f16):
    """rs_sample_moments: fp, tp [4][3] float32 -> mf, mt, H, sig (float64)"""
    fp, tp = np.asarray(fp, f32), np.asarray(tp, f32)
    sf = ((fp[0] + fp[1]) + fp[2]) + fp[3]
    st = ((tp[0] + tp[1]) + tp[2]) + tp[3]
    mf = (sf / f32(4.0)).astype(f64)
    mt = store((st / f32(4.0)).astype(f64), f16)
    fc = store(fp.astype(f64) - mf, False)
    tc = store(tp.astype(f64) - mt, f16)
    sig = f64(0.0)
    for k in range(4):
        for d in range(3):
            sig = sig + fc[k][d] * fc[k][d]
    H = np.empty((3, 3), f64)
    for i in range(3):
        for j in range(3):
            H[i, j] = ((tc[0][i] * fc[0][j] + tc[1][i] * fc[1][j]) + tc[2][i] * fc[2][j]) + tc[3][i] * fc[3][j]
    return mf, mt, H, sig


def hyp_row(R, c, t):
    """rs_hyp_row: the float64 product R c and t stored to float32, one rounding per entry"""
    row = np.empty(12, f32)
    for i in range(3):
        for j in range(3):
            row[i * 4 + j] = f32(f64(R[i][j]) * f64(c))
        row[i * 4 + 3] = f32(t[i])
    return row


def sample_fit(fp, tp, f16, typ):
    """pose_sample_fit: returns (pass, bits, row)"""
    mf, mt, H, sig = sample_moments(fp, tp, f16)
    ok, R, c, t, ratio = rs_fit(H, mf, mt, sig, typ)
    bits, row, ps = 0, None, False
    if ok and not (f32(c) > f32(3.0)):
        bits, ps, row = 2, True, hyp_row(R, c, t)
    if ratio < 1e-3:
        bits |= 4
    return ps, bits, row


def fma32(a, b, c):
    """round32(a * b + c) of float32 arrays, one rounding.  p = a * b is exact in float64 (48 bits).  s = p + c in float64 with its error e
    (TwoSum): the exact sum lies within half a float64 ulp of s, so it rounds to float32 as s does unless s itself is a midpoint of two
    neighbouring float32 values -- the only float64 numbers at which the float32 rounding changes.  Those with e != 0 are decided by
    rational arithmetic."""
    p = a.astype(f64) * b.astype(f64)
    c = c.astype(f64)
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    r = s.astype(f32)
    FMA_EXACT["candidates"] += r.size
    sus = np.flatnonzero((e != 0) & (r.astype(f64) != s) & np.isfinite(s))
    if sus.size:
        rf, sf = r.reshape(-1), s.reshape(-1)
        other = np.nextafter(rf[sus], np.where(sf[sus] > rf[sus].astype(f64), f32(np.inf), f32(-np.inf)).astype(f32))
        mid = (rf[sus].astype(f64) + other.astype(f64)) * 0.5
        for k in np.flatnonzero(mid == sf[sus]):
            i = sus[k]
            FMA_EXACT["exact_path"] += 1
            exact = Fraction(float(p.reshape(-1)[i])) + Fraction(float(c.reshape(-1)[i]))
            lo, hi = sorted((float(rf[i]), float(other[k])))
            rf[i] = f32(hi if exact > Fraction(float(mid[k])) else lo)
        r = rf.reshape(r.shape)
    return r


def transform(row, pts):
    """rs_transform of [n][3] float32 points"""
    h, x, y, z = np.asarray(row, f32), pts[:, 0], pts[:, 1], pts[:, 2]
    return np.stack([((h[0] * x + h[1] * y) + h[2] * z) + h[3], ((h[4] * x + h[5] * y) + h[6] * z) + h[7],
                     ((h[8] * x + h[9] * y) + h[10] * z) + h[11]], 1)


def nn_search(tp, mp):
    """rs_nn_search: a candidate replaces the best only when strictly nearer, candidates in index order (tile after tile): the first index
    of the smallest float32 distance; 0 when no distance compares (NaN)"""
    out = np.zeros(len(tp), np.int64)
    for lo in range(0, len(tp), 128):
        t = tp[lo:lo + 128]
        dx, dy, dz = (t[:, None, k] - mp[None, :, k] for k in range(3))
        d2 = fma32(dx, dx, fma32(dy, dy, dz * dz))
        d2 = np.where(np.isnan(d2), f32(np.inf), d2)
        out[lo:lo + 128] = np.argmin(d2, 1)
    return out


def inlier(tp, nn, mp, mc, sc, metric_thr, nocs_thr32):
    dd = tp.astype(f64) - mp[nn].astype(f64)
    d = np.sqrt(dd[:, 0] * dd[:, 0] + dd[:, 1] * dd[:, 1] + dd[:, 2] * dd[:, 2])
    cc = sc - mc[nn]
    dc = np.sqrt(cc[:, 0] * cc[:, 0] + cc[:, 1] * cc[:, 1] + cc[:, 2] * cc[:, 2])
    return (d < f64(metric_thr)) & (dc < f32(nocs_thr32))


def colour_nn(mc, sc):
    """rs_cnn_kernel: (index, float64 distance); first index of the smallest (dx^2 + dy^2) + dz^2"""
    idx, dist = np.zeros(len(sc), np.int32), np.empty(len(sc), f64)
    m = mc.astype(f64)
    for p in range(len(sc)):
        d = sc[p].astype(f64) - m
        d2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
        d2 = np.where(np.isnan(d2), np.inf, d2)
        idx[p] = np.argmin(d2)
        dist[p] = np.sqrt(d2[idx[p]])
    return idx, dist


def select(counts):
    """rs_select_kernel: lane tid walks t = tid, tid + 256, ... and takes strictly larger counts; the tree folds lane tid + o into tid"""
    T = len(counts)
    sc, st = [0] * TPB, [-1] * TPB
    for tid in range(TPB):
        for t in range(tid, T, TPB):
            if counts[t] > sc[tid]:
                sc[tid], st[tid] = int(counts[t]), t
    o = TPB // 2
    while o > 0:
        for tid in range(o):
            c2, t2 = sc[tid + o], st[tid + o]
            if c2 > sc[tid] or (c2 == sc[tid] and t2 >= 0 and (st[tid] < 0 or t2 < st[tid])):
                sc[tid], st[tid] = c2, t2
        o >>= 1
    return st[0], sc[0]


def block_sum(terms, rows):
    """terms [n][K] float64 of the points `rows` (ascending): lane p % 256 adds its terms in order from 0.0, the tree folds the lanes"""
    K = terms.shape[1]
    red = np.zeros((TPB, K), f64)
    for r, v in zip(rows, terms):
        red[r % TPB] = red[r % TPB] + v
    o = TPB // 2
    while o > 0:
        red[:o] = red[:o] + red[o:2 * o]
        o >>= 1
    return red[0].copy()


def final_fit(model, scene, cnn_idx, mask, N, ni, typ, f16, scale_model):
    """rs_final_kernel from a mask and the colour-NN table: (found, n_inliers, scale, rot [9], tra [3])"""
    ok = N >= 5 and ni >= 5
    R, c, t = np.zeros((3, 3), f64), f64(0.0), np.zeros(3, f64)
    if ok:
        rows = np.flatnonzero(mask[:N])
        m, s = model[cnn_idx[rows]].astype(f64), scene[rows].astype(f64)
        v6 = block_sum(np.concatenate([m, s, np.ones((len(rows), 1))], 1), rows)
        n = v6[6]
        with np.errstate(all="ignore"):
            mf, mt = store(v6[0:3] / n, f16), store(v6[3:6] / n, False)
        fc, tc = store(m - mf, f16), store(s - mt, False)
        terms = np.empty((len(rows), 10), f64)
        for i in range(3):
            for j in range(3):
                terms[:, i * 3 + j] = tc[:, i] * fc[:, j]
        terms[:, 9] = (fc[:, 0] * fc[:, 0] + fc[:, 1] * fc[:, 1]) + fc[:, 2] * fc[:, 2]
        v10 = block_sum(terms, rows)
        ok, R, c, t, _ = rs_fit(v10[:9].reshape(3, 3), mf, mt, v10[9], typ)
    found = 1 if ok else 0
    n_in = ni if ok else max(ni, 0)
    scale = (f32(c) if typ == 1 else f32(scale_model)) if ok else f32(0)
    rot = np.asarray(R, f64).astype(f32).reshape(9) if ok else np.zeros(9, f32)
    tra = np.asarray(t, f64).astype(f32) if ok else np.zeros(3, f32)
    return found, n_in, f32(scale), rot, tra


def hyp_stage(case, b, idx, cnn_idx, cnn_d):
    """rs_hyp_kernel of crop b from an index table and a colour-NN table: gate, counts (-1 / 0), hyp rows (dict t -> row), plist"""
    N, M, T = int(case["ncnt"][b]), int(case["mcnt"][b]), case["T"]
    model, scene = case["model"][b], case["scene"][b]
    gate, counts, rows, plist = np.zeros(T, np.int32), np.full(T, -1, np.int32), {}, []
    for t in range(T):
        if not (N >= 5 and M >= 1):
            continue
        ii = idx[t]
        if not all(0 <= int(i) < N for i in ii):
            continue
        if any(cnn_d[i] > case["nocs_thr"] for i in ii):
            continue
        ps, bits, row = sample_fit(scene[ii], model[cnn_idx[ii]], case["f16"], case["type"])
        gate[t] = 1 | bits
        if ps:
            counts[t], rows[t] = 0, row
            plist.append(t)          # ballot order within a wave, wave order within a block, block after block: ascending t
    return gate, counts, rows, np.array(plist, np.int32)


def score_stage(case, b, rows):
    """counts of the hypotheses in `rows` (dict t -> float32 row) by rs_score_kernel's rules; integer sums in any order"""
    N, M = int(case["ncnt"][b]), int(case["mcnt"][b])
    mp, mc, sp, sc = case["model"][b][:M], case["mcls"][b][:M], case["scene"][b][:N], case["scls"][b][:N]
    out = {}
    with np.errstate(all="ignore"):
        for t, row in rows.items():
            tp = transform(row, sp)
            out[t] = inlier(tp, nn_search(tp, mp), mp, mc, sc, case["metric_thr"], f32(case["nocs_thr"]))
    return out


def restate(case, device=None):
    """The whole chain of every crop.  `device`: optional dict of a run's own outputs; where it has an upstream stage's output (idx,
    cnn_idx / cnn_d, hyp, counts, best, mask) the next stage is restated from THAT, so that each link is judged on its own."""
    B, T, ncap = case["B"], case["T"], case["scene"].shape[1]
    dev = device or {}
    o = dict(idx=np.zeros((B, T, 4), np.int32), cnn_idx=np.full((B, ncap), -7, np.int32), cnn_d=np.full((B, ncap), -7.0, f64),
             gate=np.zeros((B, T), np.int32), counts=np.zeros((B, T), np.int32), hyp=np.full((B, T, 12), -7.0, f32),
             plist=np.full((B, T), -7, np.int32), pcount=np.zeros(B, np.int32), best=np.zeros(B, np.int32), n_inliers=np.zeros(B, np.int32),
             mask=np.full((B, ncap), -7, np.int32), found=np.zeros(B, np.int32), scale=np.zeros(B, f32), rot=np.zeros((B, 9), f32),
             tra=np.zeros((B, 3), f32))
    from sdflabel_amd.pose import sample_indices_numpy
    for b in range(B):
        N, M = int(case["ncnt"][b]), int(case["mcnt"][b])
        o["idx"][b] = case["idx"][b] if case["idx"] is not None else sample_indices_numpy(case["seed"], int(case["keys"][b]), N, T)
        idx = dev["idx"][b] if "idx" in dev else o["idx"][b]
        with np.errstate(all="ignore"):
            ci, cd = colour_nn(case["mcls"][b][:M], case["scls"][b][:N])
        o["cnn_idx"][b, :N], o["cnn_d"][b, :N] = ci, cd
        if "cnn_idx" in dev:
            ci, cd = dev["cnn_idx"][b, :N], dev["cnn_d"][b, :N]
        with np.errstate(all="ignore"):
            gate, counts, rows, plist = hyp_stage(case, b, idx, ci, cd)
        o["gate"][b], o["pcount"][b], o["plist"][b, :len(plist)] = gate, len(plist), plist
        for t, row in rows.items():
            o["hyp"][b, t] = row
        if "hyp" in dev:
            rows = {t: dev["hyp"][b, t] for t in rows}
        masks = score_stage(case, b, rows)
        for t, m in masks.items():
            counts[t] = int(m.sum())
        o["counts"][b] = counts
        if "counts" in dev:
            counts = dev["counts"][b]
        bt, ni = select(counts)
        o["best"][b] = bt
        if "best" in dev:
            bt = int(dev["best"][b])
            ni = int(dev["counts"][b][bt]) if bt >= 0 else 0
        if bt >= 0 and bt not in masks:          # (a device winner the restatement did not score: its mask from the device's row)
            masks.update(score_stage(case, b, {bt: dev["hyp"][b, bt]}))
        mask = masks[bt].astype(np.int32) if bt >= 0 else np.zeros(N, np.int32)
        o["mask"][b, :N] = mask
        if "mask" in dev:
            mask = dev["mask"][b, :N]
        with np.errstate(all="ignore"):
            fin = final_fit(case["model"][b], case["scene"][b], ci, mask, N, ni, case["type"], case["f16"], case["scale_model"])
        o["found"][b], o["n_inliers"][b], o["scale"][b], o["rot"][b], o["tra"][b] = fin
    return o


# ---- the case file of tests/pose_host ------------------------------------------------------------------------------------------------------

OUT_FIELDS = (("idx", np.int32, lambda B, n, T: (B, T, 4)), ("cnn_idx", np.int32, lambda B, n, T: (B, n)), ("cnn_d", f64, lambda B, n, T: (B, n)),
              ("gate", np.int32, lambda B, n, T: (B, T)), ("counts", np.int32, lambda B, n, T: (B, T)), ("hyp", f32, lambda B, n, T: (B, T, 12)),
              ("plist", np.int32, lambda B, n, T: (B, T)), ("pcount", np.int32, lambda B, n, T: (B,)), ("best", np.int32, lambda B, n, T: (B,)),
              ("n_inliers", np.int32, lambda B, n, T: (B,)), ("mask", np.int32, lambda B, n, T: (B, n)), ("found", np.int32, lambda B, n, T: (B,)),
              ("scale", f32, lambda B, n, T: (B,)), ("rot", f32, lambda B, n, T: (B, 9)), ("tra", f32, lambda B, n, T: (B, 3)))


def case_bytes(case):
    B, ncap, mcap, T = case["B"], case["scene"].shape[1], case["model"].shape[1], case["T"]
    head = struct.pack("<8iq2d2f", B, ncap, mcap, T, case["type"], int(case["f16"]), int(case["idx"] is not None), 0, case["seed"],
                       case["metric_thr"], case["nocs_thr"], case["scale_model"], 0.0)
    parts = [head, case["mcnt"].astype(np.int32).tobytes(), case["ncnt"].astype(np.int32).tobytes(), np.asarray(case["keys"], np.int64).tobytes()]
    parts += [np.ascontiguousarray(case[k], f32).tobytes() for k in ("model", "mcls", "scene", "scls")]
    if case["idx"] is not None:
        parts.append(np.ascontiguousarray(case["idx"], np.int32).tobytes())
    return b"".join(parts)


def parse_out(raw, case):
    B, ncap, T = case["B"], case["scene"].shape[1], case["T"]
    out, at = {}, 0
    for name, dt, shp in OUT_FIELDS:
        shape = shp(B, ncap, T)
        n = int(np.prod(shape)) * np.dtype(dt).itemsize
        out[name] = np.frombuffer(raw[at:at + n], dt).reshape(shape)
        at += n
    assert at == len(raw)
    return out


def defined_equal(a, b, case, what=""):
    """every integer and every DEFINED float bit of two runs' outputs: hyp rows of passing hypotheses, plist[:pcount], mask[:N],
    cnn_idx[:N], cnn_d[:N]"""
    def bits(x, y, name):
        x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
        assert x.dtype == y.dtype and x.shape == y.shape, (what, name)
        if x.dtype.kind == "f":          # a NaN equals a NaN whatever its payload; -0 differs from +0
            nan = np.isnan(x)
            assert np.array_equal(nan, np.isnan(y)), (what, name)
            x, y = np.where(nan, 0, x), np.where(nan, 0, y)
        assert x.tobytes() == y.tobytes(), (what, name, np.argwhere(x != y)[:4].tolist())
    for k in ("idx", "gate", "counts", "pcount", "best", "n_inliers", "found", "scale", "rot", "tra"):
        bits(a[k], np.asarray(b[k]).reshape(a[k].shape), k)
    for b_ in range(case["B"]):
        N, pc = int(case["ncnt"][b_]), int(a["pcount"][b_])
        for k in ("cnn_idx", "cnn_d", "mask"):
            bits(a[k][b_, :N], b[k][b_, :N], k)
        bits(a["plist"][b_, :pc], b["plist"][b_, :pc], "plist")
        ps = a["counts"][b_] >= 0
        bits(a["hyp"][b_][ps], b["hyp"][b_][ps], "hyp")


# ---- (a) the independent reference ---------------------------------------------------------------------------------------------------------

def _mp():
    import mpmath
    mpmath.mp.dps = 50
    return mpmath


def fit_mp(frm, to, typ, f16_from=False, f16_to=False, numpy_means=True):
    """Kabsch (typ 0) / Umeyama (typ 1) of to ~ c R from + t through the SVD of H = sum to_c from_c^T itself, at 50 digits.  The means and the
    centred values are rounded to the arrays' dtypes as numpy stores them (that rounding belongs to the data, not to the fit): the means are
    numpy's own `mean(axis=0)` of the arrays in their dtypes (a sample of 4), or with numpy_means=False the exact means rounded once (the
    final fit: the sum of hundreds of float32 values has no order worth pinning, the kernel adds them in float64).  Returns a
    dict: R, c, t (float64 arrays rounded once from mpmath), s (singular values, descending), gap = (s2 + sign s3) / s1, sign,
    rank (numpy's matrix_rank rule on the float32 covariance: singular values above s1 * 3 * eps32), ok (procrustes: rank >= 2)."""
    mp = _mp()
    frm, to = np.asarray(frm), np.asarray(to)
    n = len(frm)

    def exact_mean(a, h):
        m = [sum(mp.mpf(float(v)) for v in a[:, d]) / n for d in range(3)]
        return store(np.array([float(v) for v in m]), h)          # float(mpf) rounds to nearest; then the dtype
    if numpy_means:
        dt = lambda h: np.float16 if h else f32
        mf, mt = frm.astype(dt(f16_from)).mean(axis=0).astype(f64), to.astype(dt(f16_to)).mean(axis=0).astype(f64)
    else:
        mf, mt = exact_mean(frm, f16_from), exact_mean(to, f16_to)
    fc, tc = store(frm.astype(f64) - mf, f16_from), store(to.astype(f64) - mt, f16_to)
    H = mp.matrix(3, 3)
    for i in range(3):
        for j in range(3):
            H[i, j] = sum(mp.mpf(float(tc[k, i])) * mp.mpf(float(fc[k, j])) for k in range(n))
    sig = sum(mp.mpf(float(v)) ** 2 for v in fc.reshape(-1))
    return fit_mp_H(H, mf, mt, sig, typ)


def fit_mp_H(H, mf, mt, sig, typ):
    mp = _mp()
    H = mp.matrix(H)
    zero = all(H[i, j] == 0 for i in range(3) for j in range(3))
    if zero:
        U, s, Vt = mp.eye(3), [mp.mpf(0)] * 3, mp.eye(3)
    else:
        U, s, Vt = mp.svd_r(H)
        s = [s[i] for i in range(3)]
    sign = 1 if mp.det(U * Vt) >= 0 else -1
    D = mp.diag([1, 1, sign])
    R = U * D * Vt
    s1 = s[0]
    gap = (s[1] + sign * s[2]) / s1 if s1 > 0 else mp.mpf(0)
    rank = sum(1 for v in s if v > s1 * 3 * mp.mpf(EPS32)) if s1 > 0 else 0
    mfm, mtm = mp.matrix([float(v) for v in mf]), mp.matrix([float(v) for v in mt])
    if typ == 1:
        c = (s[0] + s[1] + sign * s[2]) / sig if sig != 0 else mp.mpf(0)
        t = mtm - c * (R * mfm)
        ok = rank >= 2
    else:
        c = mp.mpf(1)
        t = R * (mtm - mfm) - R * mtm + mtm
        ok = True
    # how far s2 is from the rank rule's threshold and c from 3, relative (the margins of the crafted cases)
    return dict(R=np.array([[float(R[i, j]) for j in range(3)] for i in range(3)]), c=float(c), t=np.array([float(t[i]) for i in range(3)]),
                s=[float(v) for v in s], gap=float(gap), sign=sign, rank=rank, ok=ok,
                rank_margin=float((s[1] - s1 * 3 * mp.mpf(EPS32)) / s1) if s1 > 0 else 0.0, c_mp=c, R_mp=R, t_mp=t)


def row_mp(fit):
    """the float32 row [rot*scale | tra] the reference forms from a fit: the float64 product R c and t, each stored to float32 once"""
    return hyp_row(fit["R"], fit["c"], fit["t"])


K_WORST = 14.2         # measured: tests/test_pose_refs_cpu.py::test_restatement_within_the_bound_of_the_independent_reference prints it
K_FIT = 4 * K_WORST    # the bound's K: 4 times the worst a CPU emulation of the kernel's arithmetic shows (profiles/pose_tests_notes.md)


def tscale(c, mf, mt):
    """the size of what the translation is made of: t = mt - c R mf (resp. R (mt - mf) - R mt + mt), so an error e of R or c moves t by
    about e * max(1, |c|) * max(1, |mf|, |mt|)"""
    return max(1.0, abs(float(c))) * max(1.0, float(np.abs(mf).max()), float(np.abs(mt).max()))


def fit_err(R, c, t, fit):
    """the float64 error of a fit against reference (a), each part in its own unit: |R - R_a|, |c - c_a| / max(1, |c_a|), |t - t_a| / tscale"""
    return max(float(np.abs(np.asarray(R, f64) - fit["R"]).max()), abs(float(c) - fit["c"]) / max(1.0, abs(fit["c"])),
               float(np.abs(np.asarray(t, f64) - fit["t"]).max()) / fit["tscale"])


def row_exact(fit):
    """[c R | t] of reference (a), each entry rounded once to float64"""
    r = np.empty(12, f64)
    for i in range(3):
        for j in range(3):
            r[i * 4 + j] = float(fit["c_mp"] * fit["R_mp"][i, j])
        r[i * 4 + 3] = float(fit["t_mp"][i])
    return r


def row_bound(fit, K):
    """the float32 row against row_exact: 2 u32 |R c| resp. u32 |t| for the roundings to float32, plus the float64 term K u64 / gap in the
    unit of fit_err"""
    b = np.empty(12, f64)
    c = abs(fit["c"])
    cond = K * U64 / fit["gap"]
    for i in range(3):
        for j in range(3):
            b[i * 4 + j] = 2 * U32 * abs(fit["R"][i][j]) * c + cond * max(c, 1.0)
        b[i * 4 + 3] = U32 * abs(fit["t"][i]) + cond * fit["tscale"]
    return b


def final_bound(fit, K):
    """rot [9], tra [3], scale of a final fit against (a): u32 |value| plus the same float64 term"""
    cond = K * U64 / fit["gap"]
    return U32 * np.abs(fit["R"]).reshape(9) + cond, U32 * np.abs(fit["t"]) + cond * fit["tscale"], U32 * abs(fit["c"]) + cond * max(1.0, abs(fit["c"]))


def colour_nn_brute(mc, sc):
    """float64 brute force: (index, distance, tie) with tie[p] true when two model colours are at exactly the smallest distance"""
    d = sc.astype(f64)[:, None, :] - mc.astype(f64)[None, :, :]
    d2 = np.einsum("pmk,pmk->pm", d, d)
    idx = np.argmin(d2, 1)
    best = d2[np.arange(len(sc)), idx]
    return idx, np.sqrt(best), (d2 == best[:, None]).sum(1) > 1


def score_brute(row, mp_, mc, sp, sc, metric_thr, nocs_thr):
    """inlier decisions of one hypothesis row by brute force in float64: (inlier, margin) where margin is the smallest distance of a decision
    variable to its threshold or of the nearest neighbour to its runner-up, relative; decisions with a tiny margin are not the reference's
    to make"""
    tp = transform(row, sp).astype(f64)
    d2 = ((tp[:, None, :] - mp_.astype(f64)[None, :, :]) ** 2).sum(2)
    nn = np.argmin(d2, 1)
    d = np.sqrt(d2[np.arange(len(sp)), nn])
    dc = np.sqrt(((sc.astype(f64) - mc.astype(f64)[nn]) ** 2).sum(1))
    if mp_.shape[0] > 1:
        part = np.partition(d2, 1, 1)
        runner = np.sqrt(part[:, 1]) - np.sqrt(part[:, 0])
    else:
        runner = np.full(len(sp), np.inf)
    margin = np.minimum(np.minimum(np.abs(d - metric_thr), np.abs(dc - nocs_thr)), runner)
    return (d < metric_thr) & (dc < nocs_thr), margin
