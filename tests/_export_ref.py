"""Float64 numpy restatement of the training-crop export (csrc/crop_cells.h, csrc/crops.hip; DESIGN.md "Training crops"), built on the
rasteriser's restatement tests/_verify_ref.py and written in the header's operation order: every product, quotient, sum and difference
below is one rounded float64 operation, as in the header compiled with -ffp-contract=off.  The tests compare bytes for equality."""
import numpy as np

from tests import _verify_ref as VR

FLAG_INVALID = VR.FLAG_INVALID


def byte(val):
    """0 for val <= 0 or NaN, 255 for val >= 255, else rint(val) (ties to even)"""
    val = np.asarray(val, np.float64)
    with np.errstate(all="ignore"):
        r = np.rint(np.where((val > 0.0) & (val < 255.0), val, 0.0))
    return np.where(val >= 255.0, 255, np.where(val > 0.0, r, 0)).astype(np.uint8)


def shade_values(T, xs, ys, attrs):
    """val float64 [n][3] of triangles T (lists of tri_setup dicts' u, v, z as [n][3] arrays) at the pixels (xs, ys) with attributes [n][3][3]"""
    u, v, z = T
    px, py = xs.astype(np.float64), ys.astype(np.float64)
    with np.errstate(all="ignore"):
        du, dv = u - px[:, None], v - py[:, None]
        q = []
        for i in range(3):
            a, b = (i + 1) % 3, (i + 2) % 3
            m0, m1 = du[:, a] * dv[:, b], dv[:, a] * du[:, b]
            q.append((m0 - m1) / z[:, i])
        D = (q[0] + q[1]) + q[2]
        A = np.asarray(attrs, np.float32).astype(np.float64)
        n = (q[0][:, None] * A[:, 0] + q[1][:, None] * A[:, 1]) + q[2][:, None] * A[:, 2]
        c = n / D[:, None]
        return (c + 1.0) * 127.5, c


def shade(vertices, faces, attrs, K, window, z_min, tri_img, visible=None):
    """The NOCS bytes uint8 [h][w][3] of a whole window from the raster's triangle image, and the flag word.  visible: bool [h][w], the
    pixels the annotation owns (None: occlusion off).  A triangle index outside the mesh other than -1, a face index outside the mesh or a
    triangle the rasteriser would have skipped raises FLAG_INVALID and the whole image is zeroed."""
    l, t, r, b = (int(x) for x in window)
    vertices = np.asarray(vertices, np.float32).reshape(-1, 3)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    attrs = np.asarray(attrs, np.float32).reshape(-1, 3)
    tri_img = np.asarray(tri_img, np.int64)
    out = np.zeros(tri_img.shape + (3,), np.uint8)
    Kd = [np.float64(k) for k in K]
    flags = 0
    ys, xs = np.nonzero(tri_img != -1)
    tr = tri_img[ys, xs]
    # as crop_export_pixel: an index outside the mesh is found before the owner is looked at, a triangle that cannot be set up only where
    # the annotation is visible
    idx_bad = (tr < 0) | (tr >= len(faces))
    for i in np.nonzero(~idx_bad)[0]:
        f = faces[tr[i]]
        idx_bad[i] = (f < 0).any() or (f >= len(vertices)).any()
    vis = np.ones(len(tr), bool) if visible is None else np.asarray(visible, bool)[ys, xs]
    setups = {}
    for ti in np.unique(tr[~idx_bad & vis]):
        st, T = VR.tri_setup(vertices[faces[ti]], Kd, z_min, window)
        setups[ti] = T if st == 0 else None
    bad = idx_bad.copy()
    for i in np.nonzero(~idx_bad & vis)[0]:
        bad[i] = setups[tr[i]] is None
    if bad.any():
        return out, FLAG_INVALID
    sel = vis & ~bad
    ys, xs, tr = ys[sel], xs[sel], tr[sel]
    if len(tr):
        u = np.stack([setups[ti]["u"] for ti in tr])
        v = np.stack([setups[ti]["v"] for ti in tr])
        z = np.stack([setups[ti]["z"] for ti in tr])
        val, _ = shade_values((u, v, z), xs + l, ys + t, attrs[faces[tr]])
        by = byte(val)
        by[(by == 0).all(1), 2] = 1
        out[ys, xs] = by
    return out, flags


def rgb_bytes(colors):
    """float32 BGR [..][3] -> uint8 RGB: rintf(255 v) in float32, clamped to 0 ... 255, NaN -> 0"""
    c = np.asarray(colors, np.float32)
    with np.errstate(all="ignore"):
        m = np.float32(255.0) * c
        assert m.dtype == np.float32
        r = np.rint(np.where((m > 0) & (m < 255), m, np.float32(0)))
    out = np.where(m >= 255, 255, np.where(m > 0, r, 0)).astype(np.uint8)
    return np.ascontiguousarray(out[..., ::-1])


def owner(masks, depths, windows):
    """per annotation int32 [h][w]: -1 where its own mask does not cover, else the annotation with the minimum key
    (bits(depth) << 32) | index among those whose window contains the pixel and whose mask covers it there"""
    B = len(masks)
    out = []
    for b in range(B):
        l, t, r, bt = (int(x) for x in windows[b])
        key = np.asarray(depths[b], np.float32).view(np.uint32).astype(np.uint64) << np.uint64(32) | np.uint64(b)
        best = np.where(np.asarray(masks[b]) != 0, key, VR.NO_KEY)
        for c in range(B):
            if c == b:
                continue
            cl, ct, cr, cb = (int(x) for x in windows[c])
            x0, y0, x1, y1 = max(l, cl), max(t, ct), min(r, cr), min(bt, cb)
            if x1 <= x0 or y1 <= y0:
                continue
            kc = np.asarray(depths[c], np.float32).view(np.uint32).astype(np.uint64) << np.uint64(32) | np.uint64(c)
            kc = np.where(np.asarray(masks[c]) != 0, kc, VR.NO_KEY)[y0 - ct:y1 - ct, x0 - cl:x1 - cl]
            sub = best[y0 - t:y1 - t, x0 - l:x1 - l]
            np.minimum(sub, kc, out=sub)
        own = (best & np.uint64(0xFFFFFFFF)).astype(np.int64)
        out.append(np.where(np.asarray(masks[b]) != 0, own, -1).astype(np.int32))
    return out


def export(meshes, attrs, K, windows, boxes, z_min=0.1, occlusion=True, colors=None, triangles=None):
    """The whole export of a ragged batch.  meshes: [(vertices, faces)], attrs: per mesh float32 [V][3], boxes inside the windows, colors:
    per annotation float32 BGR of the box's shape or None, triangles: per annotation a triangle image to use instead of the raster's.
    Returns per annotation a dict: uvw, rgb (or None), counts int32 [4] (box pixels, covered, visible, flag word incl. the raster's flags),
    owner, mask, depth, triangle."""
    B = len(meshes)
    ras = [VR.raster(meshes[b][0], meshes[b][1], K, windows[b], z_min) for b in range(B)]
    own = owner([r[0] for r in ras], [r[1] for r in ras], windows) if occlusion else [None] * B
    out = []
    for b in range(B):
        l, t, r, bt = (int(x) for x in windows[b])
        bl, btop, br, bb = (int(x) for x in boxes[b])
        mask, depth, tri, rflags = ras[b]
        if not (l <= bl <= br <= r and t <= btop <= bb <= bt):                  # a box outside its window: the flag, zeros
            shape = (max(bb - btop, 0), max(br - bl, 0), 3)
            out.append(dict(uvw=np.zeros(shape, np.uint8), rgb=None if colors is None else np.zeros(shape, np.uint8),
                            counts=np.array([0, 0, 0, FLAG_INVALID], np.int32), flags=FLAG_INVALID | int(rflags), owner=own[b], mask=mask,
                            depth=depth, triangle=tri))
            continue
        tri_img = tri if triangles is None or triangles[b] is None else np.asarray(triangles[b], np.int32)
        vis = None if own[b] is None else own[b] == b
        sy, sx = slice(btop - t, bb - t), slice(bl - l, br - l)
        # only the box's pixels are looked at
        boxed = np.full(tri_img.shape, -1, np.int64)
        boxed[sy, sx] = tri_img[sy, sx]
        img, flags = shade(meshes[b][0], meshes[b][1], attrs[b], K, windows[b], z_min, boxed, vis)
        uvw = np.ascontiguousarray(img[sy, sx])
        rgb = None if colors is None else rgb_bytes(colors[b])
        n = (bb - btop) * (br - bl)
        cov = mask[sy, sx] != 0
        seen = cov if vis is None else cov & vis[sy, sx]
        if flags & FLAG_INVALID:
            rgb = None if rgb is None else np.zeros_like(rgb)
            counts = np.array([0, 0, 0, flags], np.int32)
        else:
            counts = np.array([n, int(cov.sum()), int(seen.sum()), flags], np.int32)
        out.append(dict(uvw=uvw, rgb=rgb, counts=counts, flags=int(flags) | int(rflags), owner=own[b], mask=mask, depth=depth, triangle=tri_img))
    return out


def shade_bound(scale, trans):
    """Bound on |c - x| per coordinate, c the interpolated attribute (before quantisation) at a covered pixel and x = point_x of the pixel
    unprojected at the raster's float32 depth and rounded to float32, for a mesh whose attributes are its lattice vertices in [-1, 1]^3.

    With e = 2^-24 (half a float32 ulp, relative) and m = sqrt(3) + |trans|, the bound on |p_k| / scale of a camera point of the shape:
      * the pixel's ray meets the winning triangle of the ROUNDED camera vertices p_i at X = sum w_i p_i with perspective-correct weights
        w_i >= 0, sum w_i = 1, and c = sum w_i a_i with the same weights.  The map back to the lattice is affine, so it takes X to
        sum w_i (a_i + d_i), d_i the image of the rounding of p_i: each coordinate of p_i is off by at most e |p_ik|, divided by scale and
        mixed pairwise by the inverse rotation: |d_ik| <= 2 e m.                                                   (vertices rounded once)
      * the depth is rounded to float32: X moves along its ray by at most e |X|, which is e |x + trans| <= e m per lattice coordinate.
                                                                                                                    (depth rounded once)
      * the unprojected point is rounded to float32 and taken back by point_x with the label's float32 cosine, sine, translation and
        scale: that is roundtrip_bound(scale, trans) of tests/_verify_ref.py, which has the same 2 e m for the point, 2 e max|trans_k| for
        the translation, 6 e for the rotation and e for the result.
    The float64 operations in between contribute nothing at this scale."""
    t = np.abs(np.asarray(trans, np.float64))
    m = np.sqrt(3.0) + np.linalg.norm(t)
    return VR.roundtrip_bound(scale, trans) + 2.0 ** -24 * (2.0 * m + m)
