"""A float64 numpy restatement of the road-plane removal's semantics (include/sdfr.h, sdfr_lidar_normals; sdflabel_amd/frame.py lidar_normals,
remove_road, kitti_frame), brute force: per query the distances to all frustum points, a lexsort by (d2, index), the mean and the centred
covariance summed in neighbour order, numpy's eigh.  It shares no code with the product (the frustum planes come from tests/_ingest_ref.py,
which test_ingest_cpu.py pins to the reference's own output).  The semantics are the project's own statement of Open3D's hybrid search and
covariance normals; Open3D is installed nowhere this could run, so nothing here says anything about Open3D itself.

Besides the results it returns two values per point that tests use as EXCLUSION rules only: gap = (l1 - l0) / l2 of the covariance's
ascending eigenvalues (the conditioning of the normal: by Davis-Kahan a relative perturbation e of the covariance turns it by about e / gap)
and cut_tie, whether the max_nn cut fell between two candidates of exactly equal d2.

`street`, `blob` and `lattice` generate the test scenes from a seed; all coordinates are float32 values, so dx*dx is exact in float64 and d2
has the same bits with or without FMA contraction: neighbour sets can be compared for equality."""
import numpy as np

from tests import _ingest_ref as R

KITTI_K = np.array([[721.5377, 0, 609.5593], [0, 721.5377, 172.854], [0, 0, 1]], np.float64)
KITTI_WH = (1242, 375)


def in_frustum(P, K, w, h):
    pl = R.frustum_planes(K, 0, 0, w, h).astype(np.float64)
    P = np.asarray(P, np.float64).reshape(-1, 3)
    inside = np.ones(len(P), bool)
    for k in range(4):
        inside &= (pl[k, 0] * P[:, 0] + pl[k, 1] * P[:, 1]) + pl[k, 2] * P[:, 2] > 0
    return inside


def normals(P, K=None, w=None, h=None, radius=1.0, max_nn=30, cos_thresh=0.9):
    """rules 1-4.  Returns a dict of arrays over the N input points: normals [N][3], nn_count, nn_idx [N][max_nn] (-1 padded), in_frustum,
    road, keep, gap (inf where the normal is a default), cut_tie."""
    P = np.asarray(P).astype(np.float64).reshape(-1, 3)
    N = len(P)
    inside = in_frustum(P, K, w, h) if K is not None else np.ones(N, bool)
    r = float(np.float32(radius))
    r2 = r * r
    idx = np.nonzero(inside)[0]
    Q = P[idx]
    out = {"normals": np.tile([0.0, 0.0, 1.0], (N, 1)), "nn_count": np.zeros(N, np.int32), "nn_idx": np.full((N, max_nn), -1, np.int32),
           "in_frustum": inside, "gap": np.full(N, np.inf), "cut_tie": np.zeros(N, bool)}
    for a, i in enumerate(idx):
        d = Q - Q[a]
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        cand = np.nonzero(d2 < r2)[0]
        order = cand[np.lexsort((idx[cand], d2[cand]))]
        sel = order[:max_nn]
        k = len(sel)
        out["nn_count"][i] = k
        out["nn_idx"][i, :k] = idx[sel]
        out["cut_tie"][i] = len(order) > max_nn and d2[order[max_nn - 1]] == d2[order[max_nn]]
        if k < 3:
            continue
        nb = Q[sel]
        m = np.cumsum(nb, 0)[-1] / k                                   # cumsum: a sequential sum, in neighbour order
        e = nb - m
        C = np.cumsum(e[:, :, None] * e[:, None, :], 0)[-1] / k
        if not C.any():
            continue
        lam, V = np.linalg.eigh(C)
        n = V[:, 0] / np.linalg.norm(V[:, 0])
        if (n[0] * Q[a, 0] + n[1] * Q[a, 1]) + n[2] * Q[a, 2] > 0:
            n = -n
        out["normals"][i] = n
        out["gap"][i] = (lam[1] - lam[0]) / lam[2] if lam[2] > 0 else 0.0
    out["road"] = inside & (np.abs(out["normals"][:, 1]) > cos_thresh)
    out["keep"] = inside & ~out["road"]
    return out


def excluded(ref, cos_thresh=0.9):
    """the points whose road flag a correct implementation may decide either way: an ill-conditioned normal, |n_y| at the cut, a cut tie"""
    return ref["in_frustum"] & ((ref["gap"] < 1e-3) | (np.abs(np.abs(ref["normals"][:, 1]) - cos_thresh) < 1e-9) | ref["cut_tie"])


def f32(P):
    return np.asarray(P, np.float64).astype(np.float32).astype(np.float64)


def street(seed, K=KITTI_K, wh=KITTI_WH):
    """About 2 400 points in the camera frame (x right, y down, z forward): a tilted ground fan of lidar rings at y ~ 1.65 -- dense near the
    camera (neighbourhoods at the cap of 30), thinning out, and beyond 30 m rings whose points have no neighbour within 1 m --, six car-sized
    boxes standing on it and 60 stray points; some of it lies outside the KITTI frustum.  Shuffled, float32 values."""
    rng = np.random.default_rng(seed)
    tilt, slope = rng.uniform(-0.03, 0.03), rng.uniform(-0.02, 0.02)
    ground = lambda x, z: 1.65 + tilt * x + slope * (z - 10.0)         # noqa: E731
    pts = []
    for k in range(26):                                                # rings 0.8 m apart: every neighbourhood spans several rings
        rad = 5.0 + 0.8 * k + rng.uniform(-0.05, 0.05)
        az = np.deg2rad(np.arange(-44.0, 44.0, 1.6) + rng.uniform(0, 1.6))
        x, z = rad * np.sin(az), rad * np.cos(az)
        pts.append(np.stack([x, ground(x, z) + rng.normal(0, 0.01, len(az)), z], 1))
    for k in range(4):                                                 # far rings: 3 m apart and the points of a ring further than 1 m apart
        rad = 31.0 + 3.0 * k
        az = np.deg2rad(np.arange(-40.0, 40.0, 3.0) + rng.uniform(0, 3.0))
        x, z = rad * np.sin(az), rad * np.cos(az)
        pts.append(np.stack([x, ground(x, z), z], 1))
    for _ in range(6):                                                 # the two faces of a car the camera sees, 0.2 m grid with jitter
        cx, cz = rng.uniform(-7, 7), rng.uniform(9, 24)
        wd, ht, ln = 1.8, 1.5, 4.2
        side = cx - np.sign(cx) * wd / 2
        yy = np.arange(0.1, ht, 0.2)
        u, v = np.meshgrid(np.arange(-wd / 2, wd / 2, 0.2), yy)
        front = np.stack([cx + u.ravel(), ground(cx, cz) - v.ravel(), np.full(u.size, cz - ln / 2)], 1)
        u, v = np.meshgrid(np.arange(-ln / 2, ln / 2, 0.3), yy)
        flank = np.stack([np.full(u.size, side), ground(cx, cz) - v.ravel(), cz + u.ravel()], 1)
        both = np.concatenate([front, flank])
        pts.append(both + rng.normal(0, 0.01, both.shape))
    pts.append(np.stack([rng.uniform(-15, 15, 60), rng.uniform(-2, 1.5, 60), rng.uniform(4, 45, 60)], 1))
    P = np.concatenate(pts)
    return f32(P[rng.permutation(len(P))])


def blob(seed=0, n=3000):
    """n points, sigma = 0.1 m around (0, 1, 10): every neighbourhood holds the whole cloud"""
    rng = np.random.default_rng(seed)
    return f32(np.array([0.0, 1.0, 10.0]) + rng.normal(0, 0.1, (n, 3)))


def lattice(seed=0, n=7, step=0.25):
    """n^3 points of a cubic lattice of spacing `step` (exact in float32) around (0, 0, 10), shuffled: the cut at 30 falls on exact d2 ties"""
    rng = np.random.default_rng(seed)
    g = (np.arange(n) - n // 2) * step
    P = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3) + [0.0, 0.0, 10.0]
    return f32(P[rng.permutation(len(P))])


def small_camera(w=96, h=32):
    """a pinhole whose w x h image covers about the KITTI field of view"""
    s = w / KITTI_WH[0]
    return np.array([[KITTI_K[0, 0] * s, 0, KITTI_K[0, 2] * s], [0, KITTI_K[1, 1] * s, KITTI_K[1, 2] * s], [0, 0, 1]], np.float64), w, h
