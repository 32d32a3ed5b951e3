"""Float64 numpy restatement of the synthetic bootstrap crops (csrc/synth_cells.h, csrc/synth.hip; DESIGN.md "Synthetic crops"), built on
the rasteriser's restatement tests/_verify_ref.py and the export's tests/_export_ref.py and written in the header's operation order: every
product, quotient, sum, difference and square root below is one rounded float64 operation, as in the header compiled with
-ffp-contract=off.  The tests compare bytes for equality."""
import numpy as np

from tests import _export_ref as ER
from tests import _verify_ref as VR

FLAG_INVALID = VR.FLAG_INVALID
U = np.uint64


def owner(masks, depths, windows, scene=None):
    """ER.owner among the annotations of each annotation's own scene; scene None: ER.owner itself"""
    if scene is None:
        return ER.owner(masks, depths, windows)
    scene = [int(s) for s in scene]
    out = [None] * len(masks)
    for s in sorted(set(scene)):
        idx = [b for b in range(len(masks)) if scene[b] == s]
        own = ER.owner([masks[b] for b in idx], [depths[b] for b in idx], [windows[b] for b in idx])
        # ER.owner's key holds the position in `idx`: idx is increasing, so the order of the keys is that of the batch's indices
        lut = np.asarray(idx + [-1], np.int32)
        for k, b in enumerate(idx):
            out[b] = lut[own[k]]
    return out


def mix64(z):
    with np.errstate(over="ignore"):
        z = (z ^ (z >> U(30))) * U(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U(27))) * U(0x94D049BB133111EB)
        return z ^ (z >> U(31))


def hash32(seed, x, y, k):
    """uint64 array holding the 32-bit noise word of channel k at the image pixels (x, y)"""
    with np.errstate(over="ignore"):
        key = (np.asarray(x).astype(U) << U(33)) | (np.asarray(y).astype(U) << U(2)) | U(k)
        return mix64(U(int(seed) & 0xFFFFFFFF) ^ mix64(key * U(0x9E3779B97F4A7C15) + U(1))) >> U(32)


def ramp_bytes(ramp, H, xs, ys):
    """the procedural background uint8 [n][3] at the image pixels (xs, ys): integers only, C division"""
    r = [int(v) for v in ramp]
    cl = lambda v: min(max(v, 0), 255)
    amp = cl(r[6])
    den = max(H - 1, 1)
    out = np.zeros((len(xs), 3), np.uint8)
    y = np.asarray(ys, np.int64)
    for k in range(3):
        top, bot = cl(r[k]), cl(r[3 + k])
        num = (bot - top) * y
        base = top + np.sign(num) * (np.abs(num) // den)                    # towards zero
        noise = ((hash32(r[7], xs, ys, k) >> U(24)) * U(amp) >> U(8)).astype(np.int64) - (amp >> 1)
        out[:, k] = np.clip(base + noise, 0, 255)
    return out


def background(s, W, H, xs, ys, ramp, bg_index=None, bgs=None):
    at = -1 if bg_index is None else int(bg_index[s])
    if bgs is not None and 0 <= at < len(bgs):
        return np.asarray(bgs[at], np.uint8)[ys, xs]
    return ramp_bytes(ramp[s], H, xs, ys)


def pos(v):
    with np.errstate(all="ignore"):
        return np.where(v > 0.0, v, 0.0)


def dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def unit(v):
    """v / sqrt(|v|^2), 0 where the squared length is not positive (zero or NaN)"""
    with np.errstate(all="ignore"):
        l2 = dot(v, v)
        ok = l2 > 0.0
        return np.where(ok[:, None], v / np.sqrt(np.where(ok, l2, 1.0))[:, None], 0.0)


def shade_values(T, xs, ys, nrm, K, paint, light):
    """val float64 [n][3] (before the factor 255) and the unit normal [n][3] at pixels (xs, ys) of triangles T = (u, v, z) with vertex normals
    nrm [n][3][3], paint [5] (albedo, ks, shin) and light [5] (l, ambient, kd)"""
    with np.errstate(all="ignore"):
        _, n = ER.shade_values(T, xs, ys, nrm)                             # ((q0 n0 + q1 n1) + q2 n2) / D
        n = unit(n)
        K = [np.float64(k) for k in K]
        px, py = (xs.astype(np.float64) - K[2]) / K[0], (ys.astype(np.float64) - K[3]) / K[1]
        pl = np.sqrt((px * px + py * py) + 1.0)
        v = np.stack([-(px / pl), -(py / pl), -(1.0 / pl)], 1)
        l = np.broadcast_to(np.asarray(light[:3], np.float64), v.shape)
        d = pos(dot(n, l))
        h = unit(l + v)
        s = pos(dot(n, h))
        sh = float(paint[4])
        for _ in range(0 if not sh > 0.0 else 7 if sh >= 7.0 else int(sh)):
            s = s * s
        diffuse = np.float64(light[3]) + np.float64(light[4]) * d
        spec = np.float64(paint[3]) * s
        val = np.stack([np.float64(paint[k]) * diffuse + spec for k in range(3)], 1)
    return val, n


def render(meshes, normals, K, windows, boxes, size, paint, light, ramp, scene=None, bg_index=None, bgs=None, z_min=0.1, triangles=None):
    """The whole of sdfr_synth_owner / sdfr_synth_shade (and sdfr_crop_export / sdfr_crop_counts fed the scene-aware owner) for a ragged
    batch.  meshes: [(vertices, faces)] in the camera frame, normals: per mesh float32 [V][3], size: (W, H), paint [B][5], light [S][5], ramp
    [S][8], scene [B] or None, bgs: list of uint8 [H][W][3] with bg_index [S], triangles: per annotation a triangle image to use instead of
    the raster's.  Returns per annotation a dict: rgb, flag (the shading's flag word), owner, mask, depth, triangle, val (float64 [h][w][3],
    NaN where the background shows), normal."""
    B = len(meshes)
    W, H = size
    sc = [0] * B if scene is None else [int(s) for s in scene]
    ras = [VR.raster(meshes[b][0], meshes[b][1], K, windows[b], z_min) for b in range(B)]
    own = owner([r[0] for r in ras], [r[1] for r in ras], windows, scene)
    tris = [ras[b][2] if triangles is None or triangles[b] is None else np.asarray(triangles[b], np.int32) for b in range(B)]
    Kd = [np.float64(k) for k in K]
    out = []
    for b in range(B):
        l, t, r, bt = (int(x) for x in windows[b])
        bl, btop, br, bb = (int(x) for x in boxes[b])
        h, w = max(bb - btop, 0), max(br - bl, 0)
        rgb = np.zeros((h, w, 3), np.uint8)
        val = np.full((h, w, 3), np.nan)
        nrm = np.full((h, w, 3), np.nan)
        res = dict(rgb=rgb, flag=0, owner=own[b], mask=ras[b][0], depth=ras[b][1], triangle=tris[b], val=val, normal=nrm)
        out.append(res)
        if not (l <= bl <= br <= r and t <= btop <= bb <= bt) or not 0 <= sc[b] < len(light):
            res["flag"] = FLAG_INVALID
            continue
        if h * w == 0:
            continue
        ys, xs = (a.reshape(-1) for a in np.mgrid[btop:bb, bl:br])
        c_at = own[b][ys - t, xs - l].astype(np.int64)
        flat = rgb.reshape(-1, 3)
        shaded = np.zeros(len(xs), bool)
        bad = False
        for c in np.unique(c_at[c_at >= 0]):
            if c >= B or sc[c] != sc[b]:
                continue
            cl, ct, cr, cb = (int(x) for x in windows[c])
            sel = np.nonzero((c_at == c) & (cl <= xs) & (xs < cr) & (ct <= ys) & (ys < cb))[0]
            tr = tris[c][ys[sel] - ct, xs[sel] - cl].astype(np.int64)
            sel, tr = sel[tr != -1], tr[tr != -1]
            vc = np.asarray(meshes[c][0], np.float32).reshape(-1, 3)
            fc = np.asarray(meshes[c][1], np.int64).reshape(-1, 3)
            nc = np.asarray(normals[c], np.float32).reshape(-1, 3)
            setups = {}
            for ti in np.unique(tr):
                if ti < 0 or ti >= len(fc) or (fc[ti] < 0).any() or (fc[ti] >= len(vc)).any():
                    bad = True
                    continue
                st, T = VR.tri_setup(vc[fc[ti]], Kd, z_min, windows[c])
                if st != 0:
                    bad = True
                    continue
                setups[ti] = T
            if bad:
                break
            if len(tr):
                T = tuple(np.stack([setups[ti][k] for ti in tr]) for k in ("u", "v", "z"))
                vv, nn = shade_values(T, xs[sel], ys[sel], nc[fc[tr]], K, paint[c], light[sc[b]])
                with np.errstate(all="ignore"):
                    flat[sel] = ER.byte(255.0 * vv)
                val.reshape(-1, 3)[sel], nrm.reshape(-1, 3)[sel] = vv, nn
                shaded[sel] = True
        if bad:
            res["flag"] = FLAG_INVALID
            rgb[:] = 0
            continue
        rest = np.nonzero(~shaded)[0]
        flat[rest] = background(sc[b], W, H, xs[rest], ys[rest], ramp, bg_index, bgs)
    return out


def nocs(meshes, attrs, K, windows, boxes, res, z_min=0.1):
    """sdfr_crop_export (colors NULL) and sdfr_crop_counts fed render()'s scene-aware owner: per annotation (uvw, counts int32 [4])"""
    out = []
    for b, r in enumerate(res):
        l, t, _, _ = (int(x) for x in windows[b])
        bl, btop, br, bb = (int(x) for x in boxes[b])
        sy, sx = slice(btop - t, bb - t), slice(bl - l, br - l)
        boxed = np.full(r["triangle"].shape, -1, np.int64)
        boxed[sy, sx] = r["triangle"][sy, sx]
        vis = r["owner"] == b
        img, flags = ER.shade(meshes[b][0], meshes[b][1], attrs[b], K, windows[b], z_min, boxed, vis)
        cov = r["mask"][sy, sx] != 0
        n = (bb - btop) * (br - bl)
        counts = np.array([0, 0, 0, flags] if flags & FLAG_INVALID else [n, int(cov.sum()), int((cov & vis[sy, sx]).sum()), flags], np.int32)
        out.append((np.ascontiguousarray(img[sy, sx]), counts))
    return out
