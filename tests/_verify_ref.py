"""Float64 numpy restatement of the verification kernels (csrc/verify_cells.h, csrc/verify.hip; DESIGN.md "Verification"), written in the
same operation order: every product, quotient, sum and difference below is one rounded float64 operation, as in the header compiled with
-ffp-contract=off.  The tests compare masks, depth bits, triangle indices, flags, rows and counts for equality."""
import numpy as np

NO_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)
FLAG_BEHIND, FLAG_INVALID = 1, 2
F32_MAX = np.float32(3.4028234663852886e38)


def project(f, c, X, Z):
    """f (X / Z) + c in float64 from float32 X, Z"""
    with np.errstate(all="ignore"):
        q = np.asarray(X, np.float32).astype(np.float64) / np.asarray(Z, np.float32).astype(np.float64)
        m = np.float64(f) * q
        return m + np.float64(c)


def tri_setup(p, K, z_min, window):
    """one triangle p float32 [3][3] -> (status, dict): status 0 ok, 1 skipped, 2 skipped behind z_min"""
    l, t, r, b = (int(x) for x in window)
    p = np.asarray(p, np.float32)
    if not np.isfinite(p).all():
        return 1, None
    if (p[:, 2] <= np.float32(z_min)).any():
        return 2, None
    u = project(K[0], K[2], p[:, 0], p[:, 2])
    v = project(K[1], K[3], p[:, 1], p[:, 2])
    z = p[:, 2].astype(np.float64)
    if not (np.isfinite(u).all() and np.isfinite(v).all()):
        return 1, None
    with np.errstate(all="ignore"):
        a = (u[1] - u[0]) * (v[2] - v[0])
        c = (v[1] - v[0]) * (u[2] - u[0])
        A2 = a - c
    if not (A2 != 0.0) or not np.isfinite(A2):
        return 1, None
    sgn = 1.0 if A2 > 0.0 else -1.0
    if r <= l or b <= t:
        return 1, None
    ulo, uhi = max(np.ceil(u.min()), float(l)), min(np.floor(u.max()), float(r - 1))
    vlo, vhi = max(np.ceil(v.min()), float(t)), min(np.floor(v.max()), float(b - 1))
    if not (ulo <= uhi and vlo <= vhi):
        return 1, None
    return 0, dict(u=u, v=v, z=z, sgn=sgn, box=(int(ulo), int(vlo), int(uhi), int(vhi)))


def pixel_keys(T, xs, ys, tri):
    """keys (uint64) of triangle T at the pixels (xs, ys) (integer arrays of one shape); NO_KEY where it does not cover"""
    px, py = xs.astype(np.float64), ys.astype(np.float64)
    with np.errstate(all="ignore"):
        du = [T["u"][i] - px for i in range(3)]
        dv = [T["v"][i] - py for i in range(3)]
        E, ok = [], np.ones(px.shape, bool)
        for i in range(3):
            a, b = (i + 1) % 3, (i + 2) % 3
            m0, m1 = du[a] * dv[b], dv[a] * du[b]
            e = m0 - m1
            E.append(e)
            ok &= (e * T["sgn"] >= 0.0)
        S = (E[0] + E[1]) + E[2]
        D = (E[0] / T["z"][0] + E[1] / T["z"][1]) + E[2] / T["z"][2]
        depth = (S / D).astype(np.float32)
        ok &= (depth > np.float32(0)) & (depth <= F32_MAX)
    key = depth.view(np.uint32).astype(np.uint64) << np.uint64(32) | np.uint64(tri)
    return np.where(ok, key, NO_KEY)


def raster(vertices, faces, K, window, z_min=0.1):
    """one mesh into one window: (mask uint8 [h][w], depth float32 [h][w], triangle int32 [h][w], flags int)"""
    l, t, r, b = (int(x) for x in window)
    w, h = max(r - l, 0), max(b - t, 0)
    keys = np.full((h, w), NO_KEY, np.uint64)
    flags = 0
    vertices = np.asarray(vertices, np.float32).reshape(-1, 3)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    K = [np.float64(k) for k in K]
    for ti, f in enumerate(faces):
        if (f < 0).any() or (f >= len(vertices)).any():
            flags |= FLAG_INVALID
            continue
        st, T = tri_setup(vertices[f], K, z_min, window)
        if st == 2:
            flags |= FLAG_BEHIND
        if st != 0:
            continue
        x0, y0, x1, y1 = T["box"]
        ys, xs = np.meshgrid(np.arange(y0, y1 + 1), np.arange(x0, x1 + 1), indexing="ij")
        k = pixel_keys(T, xs, ys, ti)
        sub = keys[y0 - t:y1 + 1 - t, x0 - l:x1 + 1 - l]
        np.minimum(sub, k, out=sub)
    return resolve(keys) + (flags,)


def resolve(keys):
    cov = keys != NO_KEY
    depth = np.where(cov, (keys >> np.uint64(32)).astype(np.uint32), np.uint32(0)).astype(np.uint32).view(np.float32)
    tri = np.where(cov, (keys & np.uint64(0xFFFFFFFF)).astype(np.int64), -1).astype(np.int32)
    return cov.astype(np.uint8), depth, tri


def mask_counts(mask, window, label=None):
    """int32 [8]: area, tight half-open box l t r b of the covered pixels (zeros for none), label area, intersection, 0"""
    l, t = int(window[0]), int(window[1])
    m = np.asarray(mask) != 0
    out = np.zeros(8, np.int32)
    out[0] = int(m.sum())
    if out[0]:
        ys, xs = np.nonzero(m)
        out[1:5] = [l + xs.min(), t + ys.min(), l + xs.max() + 1, t + ys.max() + 1]
    if label is not None:
        g = np.asarray(label) != 0
        out[5], out[6] = int(g.sum()), int((m & g).sum())
    return out


def pose_row(c, s, trans, scale):
    return np.array([c, s, trans[0], trans[1], trans[2], scale], np.float32)


def point_x(points, pose):
    """x float32 [n][3] and the in-cube byte of camera-frame points float32 [n][3] for pose = cos, sin, trans, scale (float32)"""
    p = np.asarray(points, np.float32).reshape(-1, 3).astype(np.float64)
    pose = np.asarray(pose, np.float32).astype(np.float64)
    c, s, sc = pose[0], pose[1], pose[5]
    with np.errstate(all="ignore"):
        q0, q1, q2 = p[:, 0] / sc - pose[2], p[:, 1] / sc - pose[3], p[:, 2] / sc - pose[4]
        a0, a1, b0, b1 = c * q0, s * q2, s * q0, c * q2
        x = np.stack([(a0 - a1).astype(np.float32), (-q1).astype(np.float32), (b0 + b1).astype(np.float32)], 1)
        inside = (np.abs(x) <= np.float32(1)).all(1).astype(np.uint8)
    return x, inside


def point_rows(points, ptoff, poses, latents):
    """rows float32 [N][L + 3] = latent || x, in_cube uint8 [N] for a ragged batch"""
    rows, ins = [], []
    lat = np.asarray(latents, np.float32)
    for b in range(len(ptoff) - 1):
        x, i = point_x(points[ptoff[b]:ptoff[b + 1]], poses[b])
        rows.append(np.concatenate([np.broadcast_to(lat[b], (len(x), lat.shape[1])), x], 1).astype(np.float32))
        ins.append(i)
    L = lat.shape[1]
    return (np.concatenate(rows) if rows else np.zeros((0, L + 3), np.float32)), (np.concatenate(ins) if ins else np.zeros(0, np.uint8))


def band_counts(sdf, in_cube, ptoff, poses, band):
    """int32 [B][3]: n_pts, n_cube, n_band; in the band: in the cube and fabsf(sdf) * scale < band in float32"""
    sdf, in_cube = np.asarray(sdf, np.float32), np.asarray(in_cube) != 0
    out = np.zeros((len(ptoff) - 1, 3), np.int32)
    for b in range(len(ptoff) - 1):
        s, i = sdf[ptoff[b]:ptoff[b + 1]], in_cube[ptoff[b]:ptoff[b + 1]]
        with np.errstate(all="ignore"):
            d = np.abs(s) * np.float32(poses[b][5])
            out[b] = [len(s), int(i.sum()), int((i & (d < np.float32(band))).sum())]
    return out


def roundtrip_bound(scale, trans):
    """Bound on |x' - x| per coordinate for a lattice point x in [-1, 1]^3 taken to the camera frame by Mesh.to_camera and back by point_x.
    With e = 2^-24 (half a float32 ulp, relative): the camera point p is rounded to float32, each coordinate by at most e |p_k| with
    |p_k| / scale <= sqrt(3) + |trans|, and the inverse rotation mixes two coordinates: 2 e (sqrt(3) + |trans|) after the division by scale;
    the label's translation is float32(trans * scale), off by at most e |trans_k| scale, likewise mixed: 2 e max|trans_k|; the cosine and
    sine are float32 values, so rot^T rot differs from the identity by at most about 2 e per entry, times |x| <= sqrt(3) twice over: 6 e;
    the result is rounded once: e.  The float64 operations in between contribute nothing at this scale."""
    t = np.abs(np.asarray(trans, np.float64))
    return 2.0 ** -24 * (2.0 * (np.sqrt(3.0) + np.linalg.norm(t)) + 2.0 * t.max() + 6.0 + 1.0)
