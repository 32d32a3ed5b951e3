"""References of the band-selection / candidate-reuse bookkeeping (csrc/surface.hip) and of the parameter glue and the fused backward tail
(csrc/params.hip).  TEST INFRASTRUCTURE ONLY: plain numpy, no device code, written from the header comments of the kernels.

Two families:

  * SELECTION: integer results and float32 results of a single rounding, so every function here returns what the kernel must return BIT FOR BIT.
    Each takes the output arrays as they were before the call (`prev`, sentinel-filled by the tests) and returns updated copies, so that one
    array comparison also proves that nothing outside the documented extent was written.
  * PARAMETERS: float64 arithmetic on the float32 inputs, each result with its MASS (the sum of the absolute values of its terms), judged in
    units of eps32 * mass like tests/_splat_ref.py.

tests/test_surface_refs_cpu.py ties them to the oracle, to torch.nonzero and to torch float64 autograd."""
import numpy as np

from tests import _splat_ref as SR

F = np.float32


def _n(cnt, b, cap):
    return int(min(int(cnt[b]), cap))


# ---- selection family -------------------------------------------------------------------------------------------------------------------------

def band_ref(sdf, thr, thr_extra=None, skip=None, prev=None, cap=None, bit=0):
    """Band selection of B crops: rows with |sdf| < float32(thr) + thr_extra[b] (ONE float32 addition), ascending.
    prev: dict idx (B, cap), cnt (B,), slot (B, G) or None, over (B,) or None -- the arrays before the call.  Returns the same dict after it:
    idx[b, :min(total, cap)] the rows, cnt[b] the TRUE total, slot = rank where rank < cap else -1 on every row of the crop, over[b] |= bit only
    when total > cap (never cleared); a crop with skip[b] != 0 keeps everything."""
    sdf = np.asarray(sdf, F)
    B, G = sdf.shape
    out = {k: (None if v is None else np.array(v, copy=True)) for k, v in prev.items()}
    for b in range(B):
        if skip is not None and skip[b]:
            continue
        t = F(thr) if thr_extra is None else F(F(thr) + F(thr_extra[b]))
        with np.errstate(invalid="ignore"):
            rows = np.nonzero(np.abs(sdf[b]) < t)[0]
        total = rows.size
        k = min(total, cap)
        out["idx"][b, :k] = rows[:k]
        out["cnt"][b] = total
        if out.get("slot") is not None:
            out["slot"][b] = -1
            out["slot"][b, rows[:k]] = np.arange(k)
        if out.get("over") is not None and total > cap:
            out["over"][b] |= bit
    return out


def scatter_values_ref(dst, src, idx, cap, cnt):
    """dst[b, idx[b, s]] = src[b, s] for s < min(cnt[b], cap)"""
    dst = np.array(dst, copy=True)
    for b in range(dst.shape[0]):
        n = _n(cnt, b, cap)
        dst[b, idx[b, :n]] = src[b, :n]
    return dst


def candidate_rows_ref(inputs, cidx, stride, ccnt, prev):
    """rows[b, s] = inputs[b, cidx[b, s]] for s < n = min(ccnt[b], stride); rows n .. min(stride, n rounded up to 128) are the crop's grid row 0"""
    rows = np.array(prev, copy=True)
    for b in range(rows.shape[0]):
        n = _n(ccnt, b, stride)
        pad = min(stride, (n + 127) // 128 * 128)
        rows[b, :n] = inputs[b, cidx[b, :n]]
        rows[b, n:pad] = inputs[b, 0]
    return rows


def candidate_band_map_ref(idx, cap, cnt, cslot, stride, prev_pos, violations):
    """pos[b, e] = cslot[b, idx[b, e]] for e < min(cnt[b], cap); a band row that is no candidate (slot < 0 or >= stride) maps to position 0 and
    counts one hard violation (violations[b, 1]; violations may be None)"""
    pos = np.array(prev_pos, copy=True)
    vio = None if violations is None else np.array(violations, copy=True)
    for b in range(pos.shape[0]):
        n = _n(cnt, b, cap)
        sl = cslot[b, idx[b, :n]].copy()
        bad = (sl < 0) | (sl >= stride)
        sl[bad] = 0
        pos[b, :n] = sl
        if vio is not None:
            vio[b, 1] += int(bad.sum())
    return pos, vio


def candidate_band_ref(sdf_grid, csdf, cidx, stride, ccnt, thr, cap, prev):
    """The candidates' values written into the grid array, and the band as the order-preserving compaction of the candidates with |value| < thr:
    idx = their grid rows, pos = their positions in the candidate array, cnt the true total; over |= 1 if the band exceeds cap, |= 2 if the
    candidates exceeded their stride (then the first `stride` are used)."""
    grid = np.array(sdf_grid, copy=True)
    out = {k: np.array(v, copy=True) for k, v in prev.items()}
    for b in range(grid.shape[0]):
        n = _n(ccnt, b, stride)
        v = np.asarray(csdf[b, :n], F)
        grid[b, cidx[b, :n]] = v
        with np.errstate(invalid="ignore"):
            p = np.nonzero(np.abs(v) < F(thr))[0]
        k = min(p.size, cap)
        out["idx"][b, :k] = cidx[b, p[:k]]
        out["pos"][b, :k] = p[:k]
        out["cnt"][b] = p.size
        out["over"][b] |= (1 if p.size > cap else 0) | (2 if int(ccnt[b]) > stride else 0)
    return grid, out


def gather_rows_ref(src, idx, slot, cap, cnt, prev):
    """out[b, e] = src[b, slot[b, idx[b, e]]] for e < min(cnt[b], cap); a zero row where the slot is negative or >= src_cap"""
    out = np.array(prev, copy=True)
    src_cap = src.shape[1]
    for b in range(out.shape[0]):
        n = _n(cnt, b, cap)
        sl = slot[b, idx[b, :n]]
        ok = (sl >= 0) & (sl < src_cap)
        out[b, :n] = np.where(ok[:, None], src[b, np.where(ok, sl, 0)], F(0))
    return out


def gather_rows3_ref(src, idx, cnt):
    """out[b, j] = src[b, idx[b, j]] for j < min(cnt[b], cap), zero beyond"""
    B, cap = idx.shape
    out = np.zeros((B, cap, 3), F)
    for b in range(B):
        n = _n(cnt, b, cap)
        out[b, :n] = src[b, idx[b, :n]]
    return out


def scatter_add_rows3_ref(dst, src, idx, cnt):
    """dst[b, idx[b, j]] += src[b, j] for j < min(cnt[b], cap) (distinct idx within a crop: one float32 addition per element)"""
    out = np.array(dst, F, copy=True)
    B, cap = idx.shape
    for b in range(B):
        n = _n(cnt, b, cap)
        assert np.unique(idx[b, :n]).size == n
        out[b, idx[b, :n]] = out[b, idx[b, :n]] + np.asarray(src[b, :n], F)
    return out


def sdf_input_grad_ref(g_sdf, slot, J):
    """g_inputs[b, g] = g_sdf[b, g] * J[b, slot[b, g]] (float32 product: one rounding), zero rows where slot < 0; n_uncached = rows with slot < 0
    and a non-zero gradient"""
    g = np.asarray(g_sdf, F)
    hit = slot >= 0
    Jr = np.take_along_axis(np.asarray(J, F), np.where(hit, slot, 0)[:, :, None], axis=1)
    with np.errstate(invalid="ignore", over="ignore"):
        out = np.where(hit[:, :, None], g[:, :, None] * Jr, F(0)).astype(F)
    return out, int((~hit & (g != 0)).sum())


def audit_select_ref(cslot, stride, phase):
    """the non-candidate rows (cslot < 0) of slice ph = phase mod stride of every crop, slices of ceil(G / stride) contiguous rows: the flat
    rows b * G + g as a sorted array (the kernel's order is unspecified), n_audit their number"""
    B, G = cslot.shape
    ph = int(phase) % stride
    per = (G + stride - 1) // stride
    g = np.arange(ph * per, min((ph + 1) * per, G))
    rows = [b * G + g[cslot[b, g] < 0] for b in range(B)]
    rows = np.sort(np.concatenate(rows)) if rows else np.zeros(0, np.int64)
    return rows, rows.size


def audit_check_ref(sdf_grid, sdf_exact, src, n_audit, cap_rows, G, thr, reused, audit_dev, violations, phase):
    """per audited row i < min(n_audit, cap_rows), crop b = src[i] // G: |exact| < thr or NaN -> violations[b, 1] += 1; for crops that are not
    reused audit_dev[b] = max(audit_dev[b], |grid - exact|) (a float32 difference: one rounding; a NaN deviation never enters the maximum);
    phase + 1"""
    dev = np.array(audit_dev, F, copy=True)
    vio = np.array(violations, copy=True)
    flat = np.asarray(sdf_grid, F).reshape(-1)
    for i in range(min(int(n_audit), cap_rows)):
        r = int(src[i]); b = r // G
        ex = F(sdf_exact[i])
        if not (np.abs(ex) >= F(thr)):
            vio[b, 1] += 1
        if reused is None or not reused[b]:
            with np.errstate(invalid="ignore"):
                d = np.abs(F(flat[r] - ex))
            if d > dev[b]:
                dev[b] = d
    return dev, vio, int(phase) + 1


def guard_ref(sdf_grid, sdf_exact, idx, cap, cnt, margin, max_dev, violations, reused=None):
    """The guard's state machine, per crop: the candidates' exact values are patched into the grid array; for a crop that is not reused
    dev = max |old - exact| over its n = min(cnt, cap) candidates (0 for none; NaN if any difference is NaN), max_dev = dev,
      not (dev <= margin / 2): violations[b, 0] += 1 and margin = max(margin, 4 dev)  (a NaN dev leaves the margin: fmax returns the number)
      not (dev <  margin):     violations[b, 1] += 1 as well."""
    grid = np.array(sdf_grid, F, copy=True)
    margin = np.array(margin, F, copy=True); max_dev = np.array(max_dev, F, copy=True); vio = np.array(violations, copy=True)
    for b in range(grid.shape[0]):
        n = _n(cnt, b, cap)
        rows = idx[b, :n]
        with np.errstate(invalid="ignore", over="ignore"):
            d = np.abs(grid[b, rows] - np.asarray(sdf_exact[b, :n], F)).astype(F)
        grid[b, rows] = sdf_exact[b, :n]
        if reused is not None and reused[b]:
            continue
        dev = F(0) if n == 0 else (F(np.nan) if np.isnan(d).any() else d.max())
        m = margin[b]
        max_dev[b] = dev
        if not (dev <= F(0.5) * m):
            vio[b, 0] += 1
            if not (dev < m):
                vio[b, 1] += 1
            with np.errstate(over="ignore"):
                margin[b] = np.fmax(m, F(4) * dev)
    return grid, margin, max_dev, vio


def plan_ref(z, lip, margin, max_dev, lat_ref, age, max_reuse, n_full=None):
    """The plan's state machine: crop b reuses its candidate set while 0 < age <= max_reuse, lip |z - lat_ref| <= margin / 4 and
    max_dev <= margin / 2; then age += 1, else age = 1, lat_ref = z and n_full += 1.
    Returns reuse, lat_ref, age, n_full and `decisive` (B,): the smallest relative distance |lhs - rhs| / max(|lhs|, |rhs|) of the crop's two
    float inequalities from equality (float64) -- the float32 kernel is only pinned where this is large against eps32."""
    z = np.asarray(z, F); B = z.shape[0]
    lat_ref = np.array(lat_ref, F, copy=True); age = np.array(age, copy=True)
    n_full = None if n_full is None else np.array(n_full, copy=True)
    reuse = np.zeros(B, np.int32); decisive = np.zeros(B)
    for b in range(B):
        d = float(lip) * np.sqrt(((z[b].astype(np.float64) - lat_ref[b].astype(np.float64)) ** 2).sum())
        m, dv = float(margin[b]), float(max_dev[b])
        rel = lambda a, c: abs(a - c) / max(abs(a), abs(c), 1e-300)
        decisive[b] = min(rel(d, 0.25 * m), rel(dv, 0.5 * m))
        ok = age[b] > 0 and age[b] <= max_reuse and d <= 0.25 * m and dv <= 0.5 * m
        reuse[b] = 1 if ok else 0
        if ok:
            age[b] += 1
        else:
            age[b] = 1
            lat_ref[b] = z[b]
            if n_full is not None:
                n_full[b] += 1
    return reuse, lat_ref, age, n_full, decisive


# ---- parameter family ---------------------------------------------------------------------------------------------------------------------------

def params_forward_ref(yaw, trans, latent):
    """float64 on the float32 parameters: latnorm = max(||latent||, 1e-12) (B,), rows = latent / latnorm (B, L), pose (B, 4, 4) =
    [R_y(yaw) | t] with row 1 of the rotation negated"""
    yaw = np.asarray(yaw, np.float64).reshape(-1); trans = np.asarray(trans, np.float64).reshape(-1, 3)
    lat = np.asarray(latent, np.float64); B = yaw.shape[0]
    latnorm = np.maximum(np.sqrt((lat * lat).sum(1)), 1e-12)
    rows = lat / latnorm[:, None]
    c, s = np.cos(yaw), np.sin(yaw)
    pose = np.zeros((B, 4, 4))
    pose[:, 0, 0] = c; pose[:, 0, 2] = s; pose[:, 1, 1] = -1.0; pose[:, 2, 0] = -s; pose[:, 2, 2] = c
    pose[:, :3, 3] = trans
    pose[:, 3, 3] = 1.0
    return latnorm, rows, pose


def params_backward_ref(yaw_c, yaw_s, latent, latnorm, g_pose, g_latn, m_pose=None, m_latn=None):
    """float64: g_yaw = <dR/dyaw, g_pose>, dR/dyaw = [[-s, 0, c], [0, 0, 0], [-c, 0, -s]]; g_trans = g_pose[:, :3, 3];
    g_latent = (g_latn - z <z, g_latn>) / latnorm with z = latent / latnorm (F.normalize's backward, also where the clamp holds: then z = 0 for a
    zero latent).  c, s, latnorm are INPUTS (the kernel's own float32 values in the GPU tests).  m_pose / m_latn: the masses of the incoming
    gradients (default: their absolute values).  Returns g_yaw, g_trans, g_latent and a dict of their masses."""
    c = np.asarray(yaw_c, np.float64).reshape(-1); s = np.asarray(yaw_s, np.float64).reshape(-1)
    lat = np.asarray(latent, np.float64); nrm = np.asarray(latnorm, np.float64).reshape(-1, 1)
    gp = np.asarray(g_pose, np.float64).reshape(-1, 4, 4)[:, :3]; gl = np.asarray(g_latn, np.float64)
    mp = np.abs(gp) if m_pose is None else np.asarray(m_pose, np.float64).reshape(-1, 3, 4)
    ml = np.abs(gl) if m_latn is None else np.asarray(m_latn, np.float64)
    g_yaw = -s * gp[:, 0, 0] + c * gp[:, 0, 2] - c * gp[:, 2, 0] - s * gp[:, 2, 2]
    m_yaw = np.abs(s) * mp[:, 0, 0] + np.abs(c) * mp[:, 0, 2] + np.abs(c) * mp[:, 2, 0] + np.abs(s) * mp[:, 2, 2]
    z = lat / nrm
    dot = (z * gl).sum(1, keepdims=True)
    g_latent = (gl - z * dot) / nrm
    m_latent = (ml + np.abs(z) * (np.abs(z) * ml).sum(1, keepdims=True)) / nrm
    return g_yaw, gp[:, :, 3].copy(), g_latent, dict(g_yaw=m_yaw, g_trans=mp[:, :, 3].copy(), g_latent=m_latent)


def tail_ref(pose, points, normals, g_pc, g_nc, g_col, mode, g_xyzf, fslot, J_lat, latent, latnorm):
    """The fused backward tail of ONE crop in float64, the composition of _splat_ref.project_bwd_ref (g_points, the 12 pose sums),
    the iso-projection's g_sdf = -<g_points, n_hat> (surface_project_bwd_ref), the latent contraction g_latn = sum g_sdf J[:, :L]
    (surface_latent_grad_ref; without the float32 roundings those take between the stages) and params_backward_ref with c = pose[0, 0],
    s = pose[0, 2].  J_lat None: pose only, g_latn = g_latent = 0.  g_xyzf: the rows as the kernel adds them (with SOLVE the float32 products
    g_xyzf * kscale[2 b + 1]).  Returns a dict of values and `mass_*`."""
    pose = np.asarray(pose, F).reshape(4, 4)
    L = np.asarray(latent).shape[-1]
    pb = SR.project_bwd_ref(pose, points, normals, g_pc, g_nc, g_col, mode, g_xyzf=g_xyzf, fslot=fslot)
    nh = np.asarray(normals, F).astype(np.float64).reshape(-1, 3)
    gs = -(pb["g_points"] * nh).sum(1)
    ms = (pb["mass_g_points"] * np.abs(nh)).sum(1)
    if J_lat is not None:
        Jl = np.asarray(J_lat, F).astype(np.float64)
        g_latn = (gs[:, None] * Jl).sum(0); m_latn = (ms[:, None] * np.abs(Jl)).sum(0)
    else:
        g_latn = np.zeros(L); m_latn = np.zeros(L)
    g_pose = np.zeros((4, 4)); g_pose[:3] = pb["g_pose"]
    gy, gt, gl, m = params_backward_ref(pose[0, 0], pose[0, 2], np.asarray(latent, F).reshape(1, L), np.asarray(latnorm, F).reshape(1),
                                        g_pose[None], g_latn[None], pb["mass_g_pose"][None], m_latn[None])
    if J_lat is None:
        gl = np.zeros((1, L)); m["g_latent"] = np.zeros((1, L))
    return dict(g_points=pb["g_points"], mass_g_points=pb["mass_g_points"], g_pose=pb["g_pose"], mass_g_pose=pb["mass_g_pose"], g_sdf=gs,
                mass_g_sdf=ms, g_latn=g_latn, mass_g_latn=m_latn, g_yaw=gy[0], mass_g_yaw=m["g_yaw"][0], g_trans=gt[0], mass_g_trans=m["g_trans"][0],
                g_latent=gl[0], mass_g_latent=m["g_latent"][0])
