"""A numpy restatement of the signed distance to triangle meshes and of the surface sampler ("Signed distances to meshes").

It follows the rules literally: float64 on the float32 values, every operation on its own (numpy never fuses), the component order of
csrc/mesh_sdf_cells.h, triangles in index order, chunks of 4096 folded in chunk order.  It is vectorised over the query points and loops
over the triangles, so its output is compared with the header's and the kernels' bit for bit -- except the winding number, whose atan2 is
the one operation that differs between libraries.
"""
import numpy as np

CHUNK = 4096
AREA_CHUNK = 256
FLAG_NONFINITE, FLAG_INVALID = 1, 2
TWO_PI = 6.283185307179586


def dot(u, v):
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def cross(u, v):
    return np.stack(np.broadcast_arrays(u[..., 1] * v[..., 2] - u[..., 2] * v[..., 1], u[..., 2] * v[..., 0] - u[..., 0] * v[..., 2],
                                        u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]), -1)


def seg(p, a, b):
    ab, ap = b - a, p - a
    l2 = dot(ab, ab)
    t = dot(ap, ab) / l2 if l2 > 0 else np.zeros(len(p))
    t = np.where(t < 0, 0.0, np.where(t > 1, 1.0, t))
    d = ap - t[:, None] * ab
    return dot(d, d)


def tri_d2(p, a, b, c):
    """squared distance of the points p [n][3] (float64) to one triangle"""
    m = seg(p, a, b)
    s = seg(p, b, c)
    m = np.where(s < m, s, m)
    s = seg(p, c, a)
    m = np.where(s < m, s, m)
    e1, e2 = b - a, c - a
    n = cross(e1, e2)
    nn = dot(n, n)
    if not nn > 0:
        return m
    pa = p - a
    ok = (dot(cross(e1, pa), n) >= 0) & (dot(cross(c - b, p - b), n) >= 0) & (dot(cross(a - c, p - c), n) >= 0)
    h = dot(pa, n)
    s = (h * h) / nn
    return np.where(ok & (s < m), s, m)


def omega(p, a, b, c):
    A, B, C = a - p, b - p, c - p
    la, lb, lc = np.sqrt(dot(A, A)), np.sqrt(dot(B, B)), np.sqrt(dot(C, C))
    det = dot(A, cross(B, C))
    den = (((la * lb) * lc + dot(A, B) * lc) + dot(A, C) * lb) + dot(B, C) * la
    return np.where(det == 0, 0.0, np.arctan2(det, den) / TWO_PI)


def triangles(vertices, faces):
    """(tri float64 [T][3][3], status int [T]) of one mesh: status 0, or the flag bit of the reason the triangle is skipped"""
    v = np.asarray(vertices, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    bad = ((f < 0) | (f >= len(v))).any(1)
    tri = np.zeros((len(f), 3, 3))
    tri[~bad] = v[f[~bad]]
    status = np.where(bad, FLAG_INVALID, np.where(~np.isfinite(tri).all((1, 2)), FLAG_NONFINITE, 0))
    return tri, status


def mesh_sdf(vertices, faces, points, want_sign=True):
    """One mesh, its query points float32 [n][3] -> dict of sdf float32, dist float32, d2 float64, nearest int32, winding float64 (each [n]),
    flags (int), and abs_winding float64 [n], the sum of |omega| (the size of the winding sum's rounding error; no kernel computes it)."""
    tri, status = triangles(vertices, faces)
    p32 = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    n = len(p32)
    live = np.isfinite(p32).all(1)
    p = np.where(live[:, None], p32, 0).astype(np.float64)
    best, idx, w, aw = np.full(n, np.inf), np.full(n, -1, np.int32), np.zeros(n), np.zeros(n)
    for c0 in range(0, len(tri), CHUNK):
        cd2, cidx, cs = np.full(n, np.inf), np.full(n, -1, np.int32), np.zeros(n)
        for t in range(c0, min(c0 + CHUNK, len(tri))):
            if status[t]:
                continue
            a, b, c = tri[t]
            d = tri_d2(p, a, b, c)
            less = d < cd2
            cd2, cidx = np.where(less, d, cd2), np.where(less, np.int32(t), cidx)
            if want_sign:
                o = omega(p, a, b, c)
                cs = cs + o
                aw = aw + np.abs(o)
        less = cd2 < best
        best, idx = np.where(less, cd2, best), np.where(less, cidx, idx)
        w = w + cs
    best, idx, w = np.where(live, best, np.inf), np.where(live, idx, -1).astype(np.int32), np.where(live, w, 0.0)
    dist = np.sqrt(best).astype(np.float32)
    inside = (np.abs(w) >= 0.5) if want_sign else np.zeros(n, bool)
    return dict(sdf=np.where(inside, -dist, dist).astype(np.float32), dist=dist, d2=best, nearest=idx, winding=w if want_sign else np.zeros(n),
                flags=int(np.bitwise_or.reduce(status)) if len(status) else 0, abs_winding=aw)


def cumulative_area(vertices, faces):
    """(cum float64 [T], flags) in the defined order: sequential inside chunks of 256, sequential over the chunk totals"""
    tri, status = triangles(vertices, faces)
    with np.errstate(invalid="ignore", over="ignore"):
        e1, e2 = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
        n = cross(e1, e2)
        area = np.where(status == 0, np.sqrt(dot(n, n)) / 2.0, 0.0)
    cum = np.zeros(len(tri))
    base = 0.0
    for c0 in range(0, len(tri), AREA_CHUNK):
        local = np.cumsum(area[c0:c0 + AREA_CHUNK])                 # sequential
        cum[c0:c0 + AREA_CHUNK] = base + local
        base = base + local[-1]
    flags = int(np.bitwise_or.reduce(status)) if len(status) else 0
    if not (len(cum) and cum[-1] > 0):
        flags |= FLAG_INVALID
    return cum, flags


def surface_points(vertices, faces, uniforms):
    """uniforms float32 [s][3] -> (points float32 [s][3], triangle int32 [s], flags)"""
    u = np.asarray(uniforms, dtype=np.float32).reshape(-1, 3)
    tri, _ = triangles(vertices, faces)
    cum, flags = cumulative_area(vertices, faces)
    pts, pick = np.zeros((len(u), 3), np.float32), np.full(len(u), -1, np.int32)
    if len(cum) == 0 or not cum[-1] > 0 or len(u) == 0:
        return pts, pick, flags
    ok = ((u >= 0) & (u < 1)).all(1)
    target = u[:, 0].astype(np.float64) * cum[-1]
    t = np.searchsorted(cum, target, side="right")                  # the first t with cum[t] > target
    ok &= t < len(cum)
    t = np.where(ok, t, 0)
    s = np.sqrt(np.where(ok, u[:, 1], 0).astype(np.float64))
    u2 = u[:, 2].astype(np.float64)
    w0, w1, w2 = 1.0 - s, s * (1.0 - u2), s * u2
    x = (w0[:, None] * tri[t, 0] + w1[:, None] * tri[t, 1]) + w2[:, None] * tri[t, 2]
    return np.where(ok[:, None], x, 0).astype(np.float32), np.where(ok, t, -1).astype(np.int32), flags
