"""Input generators of tests/test_gpu_losses.py, shared with tests/test_loss_refs_cpu.py, which checks on the float64 references alone that the
inputs are fit to judge a float32 kernel with (few ambiguous rows, no row at the pairing threshold, both threshold branches taken)."""
import numpy as np

DIAMS = (5.0, 3.2, 7.0, 9.0, 10.5)        # <true,4>; <true,0> with radius 3 and 6; the largest LDS radius (8); <false,0>
SHAPES = ((1, 40), (40, 1), (16, 16), (17, 15), (31, 33), (24, 20), (37, 53), (64, 48))          # (H, W)
DENSE_SHAPES = ((6, 6), (7, 7), (12, 12))
THRESHOLDS_2D = (1.0, 0.3)

CLOUDS = (          # (ne, nl, ecap, lcap, scale)
    (300, 150, 512, 256, 2.0),
    (1000, 1025, 1000, 1025, 1.7),
    (3000, 2500, 3008, 4096, 2.3),
    (4100, 4096, 4160, 4096, 0.9),
    (64, 3, 64, 4, 1.0),
)
THRESHOLD_3D = 0.2


def _rng(*k):
    return np.random.default_rng([int(round(10 * x)) for x in k])


def image_2d(H, W, seed=0):
    """a uniform random rendering on a 60 % dense uniform random target.  Rendered pixels: the first and last row and column (every second
    pixel), both sides of every 16-pixel tile boundary, 15 % of the rest; one whole 16x16 tile next to a rendered one is left unrendered
    where the image has more than one tile."""
    rng = _rng(H, W, seed)
    tgt = (rng.random((3, H, W)) * (rng.random((1, H, W)) < 0.6)).astype(np.float32)
    mask = rng.random((H, W)) < 0.15
    mask[0, ::2] = mask[H - 1, 1::2] = True
    mask[::2, 0] = mask[1::2, W - 1] = True
    for k in range(16, H, 16):
        mask[k - 1, ::3] = mask[k, 1::3] = True
    for k in range(16, W, 16):
        mask[::3, k - 1] = mask[1::3, k] = True
    if W > 16:
        mask[0:16, 16:32] = False
    elif H > 16:
        mask[16:32, 0:16] = False
    rend = (rng.random((3, H, W)) * mask[None]).astype(np.float32)
    return rend, tgt


def dense_2d(H, W, seed=0):
    """a small crop with a dense target in [0.5, 1] and a dim rendering in [0.02, 0.08] on the interior pixels: for the pixels whose farthest
    image corner is closer than diam, no pixel of the image has weight 0, so "the rendered colour's own norm" is not a candidate"""
    rng = _rng(H, W, seed, 7)
    tgt = rng.uniform(0.5, 1.0, (3, H, W)).astype(np.float32)
    rend = np.zeros((3, H, W), np.float32)
    rend[:, 1:-1, 1:-1] = rng.uniform(0.02, 0.08, (3, H - 2, W - 2))
    return rend, tgt


def near_2d(H, W, diam, seed=0):
    """a crop where half of the rendered pixels lie 0.02 from the weighted target of their own pixel (target * diam), the others anywhere:
    minima on both sides of a threshold as small as 0.05"""
    rng = _rng(H, W, diam, seed, 11)
    rend, tgt = image_2d(H, W, seed + 1)
    for y, x in zip(*np.nonzero(rend.sum(0))):
        if rng.random() < 0.5 and tgt[:, y, x].sum() > 0:
            d = rng.standard_normal(3)
            rend[:, y, x] = (tgt[:, y, x].astype(np.float64) * diam + 0.02 * d / np.linalg.norm(d)).astype(np.float32)
    return rend, tgt


BATCH_SHAPES = ((6, 6), (12, 12))
BATCH_THRESHOLDS = (1.0, 0.3, 0.05)


def batch_2d(H, W, diam):
    """six crops of one size for one batched call: (name, rend, target)"""
    n_r, n_t = near_2d(H, W, diam)
    z_r = np.zeros((3, H, W), np.float32)
    o_r = z_r.copy(); o_r[:, 0, 0] = (0.3, 0.5, 0.2)                   # only pixel (0, 0): the index sum is 0, the reference returns 0
    _, t1 = image_2d(H, W, 3)
    far_r, _ = image_2d(H, W, 4)
    far_r = (-(far_r + (far_r.sum(0, keepdims=True) > 0))).astype(np.float32)       # rendered pixels in [-2, -1]: >= 1.7 from every weighted target (>= 0)
    s_r, s_t = image_2d(H, W, 5)
    ys, xs = np.nonzero(s_r.sum(0))
    for y, x in list(zip(ys, xs))[::2]:
        s_r[:, y, x] = (0.5, -0.5, 0.0)                                 # non-zero, channel sum exactly 0: counts as unrendered
    d_r, d_t = dense_2d(H, W)
    return [("near", n_r, n_t), ("zero", z_r, t1), ("origin", o_r, t1), ("far", far_r, t1), ("zerosum", s_r, s_t), ("dense", d_r, d_t)]


RAGGED_PIX_STRIDE = 1056
RAGGED_TILES_CAP = 7


def ragged_2d():
    """five slots of RAGGED_PIX_STRIDE pixels per channel: (name, rend, target), each with its own (H_b, W_b); the last lies outside the
    contract (W_b * H_b > pix_stride)"""
    out = [("17x15",) + image_2d(17, 15, 2), ("31x33",) + image_2d(31, 33, 2)]
    out.append(("1x1", np.full((3, 1, 1), 0.4, np.float32), np.full((3, 1, 1), 0.3, np.float32)))
    out.append(("dense6x6",) + dense_2d(6, 6, 1))
    out.append(("64x48",) + image_2d(64, 48, 2))
    return out


def cloud_3d(ne, nl, scale, seed=0):
    """uniform clouds (frustum units): the estimated points fill a box, the lidar its first 55 % in x, at a density of ~2.4 points per
    (threshold / scale)^3 -- an estimated point inside the lidar's part finds a partner at ~0.4 of the pairing distance, one outside
    finds none unless it is near the border"""
    rng = _rng(ne, nl, scale, seed)
    side = THRESHOLD_3D / scale * max(nl, 8) ** (1.0 / 3.0) * 0.75
    est = (rng.random((ne, 3)) * np.array([side / 0.55, side, side])).astype(np.float32)
    lid = (rng.random((nl, 3)) * side * scale).astype(np.float32)
    return est, lid


def batch_3d(ecap=1000, lcap=1025):
    """five crops for one call with per-crop counts: (name, est rows, lidar rows, ecnt, lcnt, scale).  'over' announces more estimated points
    than the capacity: the count is clamped to the capacity."""
    out = []
    e, l = cloud_3d(900, lcap, 1.7, 1); out.append(("normal", e, l, 900, lcap, 1.7))
    e, l = cloud_3d(500, 300, 2.0, 2); out.append(("nolidar", e, l, 500, 0, 2.0))
    e, l = cloud_3d(500, 300, 0.9, 3); out.append(("noest", e, l, 0, 300, 0.9))
    e, l = cloud_3d(ecap, 700, 1.3, 4); out.append(("over", e, l, ecap + 200, 700, 1.3))
    e, l = cloud_3d(1, lcap, 2.3, 5)
    e[0] = l[3] / np.float32(2.3) + np.float32(0.01)                    # the single point has a partner
    out.append(("one", e, l, 1, lcap, 2.3))
    return out


def single_2d(H, W):
    return dense_2d(H, W) if (H, W) in DENSE_SHAPES else image_2d(H, W)


def all_2d_inputs():
    """every generated 2-D input: (name, rend, target, diam, thresholds, one_sided) -- one_sided: built to sit far on one side of every threshold"""
    for diam in DIAMS:
        for H, W in SHAPES + DENSE_SHAPES:
            yield ("single %dx%d diam %g" % (H, W, diam),) + single_2d(H, W) + (diam, THRESHOLDS_2D, False)
        for H, W in BATCH_SHAPES:
            for name, r, t in batch_2d(H, W, diam):
                yield "batch %dx%d %s diam %g" % (H, W, name, diam), r, t, diam, BATCH_THRESHOLDS, name in ("zero", "origin", "far")
        for name, r, t in ragged_2d():
            yield "ragged %s diam %g" % (name, diam), r, t, diam, THRESHOLDS_2D, name == "1x1"


def all_3d_inputs():
    """every generated random 3-D input, as the kernel sees it after the counts are applied: (name, est, lidar, scale)"""
    for ne, nl, _, _, scale in CLOUDS:
        yield ("cloud %dx%d" % (ne, nl),) + cloud_3d(ne, nl, scale) + (scale,)
    for name, e, l, ec, lc, scale in batch_3d():
        yield "batch " + name, e[:min(ec, e.shape[0])], l[:lc], scale


# ---- tie rule: a 13^3 lattice of spacing 1/8 (frustum units) in shuffled order ----------------------------------------------------------
LATTICE_N = 13
TIE_THRESHOLD = 0.5                     # threshold / scale >= 0.25 > sqrt(3) / 16: every midpoint is paired
TIE_PER_KIND = 1300
TIE_SCALES = (1.0, 2.0)


def lattice_3d(scale, seed=0):
    """lidar = lattice * scale in shuffled order (coordinates multiples of scale / 8: exact for scale 1 and 2, and lidar / scale is the
    lattice again); estimated points = midpoints of edges (the 2 nearest lattice points at the same exact distance), of faces (4) and of
    cells (8), TIE_PER_KIND of each.
    Returns est, lidar, winner (the first lidar index among the nearest, over the exact float32 squared distances) and tied[j] (all of them)."""
    rng = _rng(LATTICE_N, scale, seed, 3)
    g = np.arange(LATTICE_N, dtype=np.float64) / 8.0
    lat = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    lat = lat[rng.permutation(lat.shape[0])]
    h = 1.0 / 16.0
    c = np.stack(np.meshgrid(g[:-1], g[:-1], g[:-1], indexing="ij"), -1).reshape(-1, 3)
    kinds = []
    for offs in ([(h, 0, 0), (0, h, 0), (0, 0, h)], [(h, h, 0), (h, 0, h), (0, h, h)], [(h, h, h)]):
        p = np.concatenate([c + np.array(o) for o in offs])
        kinds.append(p[rng.permutation(p.shape[0])[:TIE_PER_KIND]])
    est = np.concatenate(kinds).astype(np.float32)
    lidar = (lat * scale).astype(np.float32)
    fr = lidar / np.float32(scale)
    assert np.array_equal(fr.astype(np.float64), lat) and np.array_equal(est.astype(np.float64), np.concatenate(kinds))
    winner = np.zeros(est.shape[0], np.int64)
    tied = []
    for j0 in range(0, est.shape[0], 512):
        df = fr[None] - est[j0:j0 + 512, None, :]                       # float32, exact
        d2 = (df[..., 0] * df[..., 0] + df[..., 1] * df[..., 1]) + df[..., 2] * df[..., 2]
        winner[j0:j0 + 512] = d2.argmin(1)
        tied += [np.nonzero(r)[0] for r in d2 == d2.min(1, keepdims=True)]
    return est, lidar, winner, tied


def scan_slot(i, nl, tile=1024, waves=4):
    """(tile, wave) that scans lidar index i in the kernel's layout: tiles of 1024 points, a tile split evenly over the four waves"""
    tl, m = divmod(int(i), tile)
    mn = min(tile, nl - tl * tile)
    return tl, m // ((mn + waves - 1) // waves)


# ---- solver -------------------------------------------------------------------------------------------------------------------------------
SOLVER_SIZES = tuple((B, L) for B in (1, 64, 130) for L in (1, 3, 16))
SOLVER_STEPS = 200
SOLVER_MAGS = (0.0, 1e-8, 1e-7, 1e-4, 1.0, 1e3)
LR_ADAM, LR_SCALE, LR_LATENT = 0.01, 0.01, 3e-5
W2, W3 = 0.3, 0.5


def solver_inputs(B, L, steps=SOLVER_STEPS, seed=0):
    """params0 (5B + BL,), the crops' gradient magnitudes, and per step (grads, loss2d, loss3d, npairs).  Crop b's gradients have the
    magnitude SOLVER_MAGS[(b + L) % 6] times a random factor in [0.5, 1.5] and the element's sign; in a random quarter of its iterations a crop is skipped
    through npairs = -1, loss2d = NaN, or both losses 0."""
    rng = _rng(B, L, steps, seed)
    n = 5 * B + B * L
    p0 = rng.uniform(-1.0, 1.0, n).astype(np.float32)
    mag = np.asarray(SOLVER_MAGS)[(np.arange(B) + L) % 6]
    crop = np.concatenate([np.arange(B), np.repeat(np.arange(B), 3), np.arange(B), np.repeat(np.arange(B), L)])
    sign = rng.choice([-1.0, 1.0], n)          # one sign per element for the whole run: the first moment never cancels, so a relative bound on it means something
    seq = []
    for _ in range(steps):
        g = (mag[crop] * rng.uniform(0.5, 1.5, n) * sign).astype(np.float32)
        l2 = rng.uniform(0.1, 1.0, B).astype(np.float32)
        l3 = rng.uniform(0.01, 0.2, B).astype(np.float32)
        npairs = rng.integers(0, 500, B).astype(np.int32)
        kind = np.where(rng.random(B) < 0.25, rng.integers(1, 4, B), 0)
        npairs[kind == 1] = -1
        l2[kind == 2] = np.nan
        l2[kind == 3] = 0
        l3[kind == 3] = 0
        seq.append((g, l2, l3, npairs))
    return p0, mag, seq
