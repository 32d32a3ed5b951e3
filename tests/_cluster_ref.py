"""Numpy restatement of the lidar clusters and rough boxes (csrc/cluster.hip, csrc/cluster_cells.h), and the cases the tests
run.  Nothing here looks at a hash grid: neighbours are found by brute force over all pairs, with the stated rounding
d2 = (dx*dx + dy*dy) + dz*dz < eps*eps in float64; components by the restatement's own union (minimum-label propagation with pointer
jumping, which ends with every point labelled by the smallest index of its component); then the numbering, the gates, the cap, the stable
member lists and the rectangles over a given direction table.  tests/test_cluster_cpu.py pins it to scipy's connected_components over
cKDTree pairs; the host build of cluster_cells.h and the GPU kernels must equal it bit for bit.

The cases are chosen for where the kernels can go wrong, not for a workload.
"""
import functools

import numpy as np

CAPPED, NONFINITE = 1, 2
RECT = 8


def f32(P):
    return np.asarray(P, np.float64).astype(np.float32).astype(np.float64)


def takes_part(P, mask=None):
    P = np.asarray(P).reshape(-1, 3).astype(np.float64)
    m = np.ones(len(P), bool) if mask is None else np.asarray(mask).reshape(-1) != 0
    fin = np.isfinite(P).all(1)
    return m & fin, bool((m & ~fin).any())


def pairs(P, part, eps):
    """(i, j) arrays, j < i, of the neighbouring participating points: brute force, d2 = (dx*dx + dy*dy) + dz*dz < eps*eps in float64"""
    idx = np.nonzero(part)[0]
    Q = np.asarray(P).reshape(-1, 3).astype(np.float64)[idx]
    e = float(np.float32(eps))
    e2 = e * e
    I, J = [], []
    for a0 in range(0, len(Q), 256):
        d = Q[a0:a0 + 256, None, :] - Q[None, :, :]
        d2 = (d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1]) + d[:, :, 2] * d[:, :, 2]
        a, b = np.nonzero(d2 < e2)
        a = a + a0
        lower = b < a
        I.append(idx[a[lower]]); J.append(idx[b[lower]])
    if not I:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    return np.concatenate(I), np.concatenate(J)


def roots(N, part, I, J):
    """root int64 [N]: the smallest index of every participating point's component, -1 for the others"""
    lab = np.arange(N, dtype=np.int64)
    while True:
        m = np.minimum(lab[I], lab[J])
        new = lab.copy()
        np.minimum.at(new, I, m)
        np.minimum.at(new, J, m)
        while True:                                                      # pointer jumping
            nxt = new[new]
            if np.array_equal(nxt, new):
                break
            new = nxt
        if np.array_equal(new, lab):
            break
        lab = new
    return np.where(part, lab, -1)


def clusters(P, mask=None, eps=0.5, min_points=10, max_points=None, max_clusters=512):
    """dict: label int32 [N], members int32 [total], off int32 [max_clusters + 1], counts int32 [4], root int64 [N], kept"""
    P = np.asarray(P).reshape(-1, 3)
    N = len(P)
    part, bad = takes_part(P, mask)
    I, J = pairs(P, part, eps)
    root = roots(N, part, I, J)
    size = np.bincount(root[root >= 0], minlength=N) if N else np.zeros(0, np.int64)
    is_root = root == np.arange(N)
    mp = 0 if max_points is None else int(max_points)
    is_cluster = is_root & (size >= int(min_points)) & ((size <= mp) if mp > 0 else True)
    cid = np.cumsum(is_cluster) - is_cluster                             # exclusive: ascending smallest member index
    found = int(is_cluster.sum())
    kept = min(found, int(max_clusters))
    label = np.full(N, -1, np.int32)
    ok = root >= 0
    r = np.where(ok, root, 0)
    ok &= is_cluster[r] & (cid[r] < max_clusters) if N else ok
    label[ok] = cid[r[ok]]
    off = np.zeros(max_clusters + 1, np.int32)
    members = []
    for c in range(kept):
        m = np.nonzero(label == c)[0]                                    # ascending input index
        members.append(m)
        off[c + 1] = off[c] + len(m)
    off[kept + 1:] = off[kept]
    flags = (CAPPED if found > max_clusters else 0) | (NONFINITE if bad else 0)
    counts = np.array([int(part.sum()), int(is_root.sum()), found, flags], np.int32)
    return {"label": label, "members": np.concatenate(members).astype(np.int32) if members else np.zeros(0, np.int32), "off": off, "counts": counts,
            "root": root, "kept": kept}


def directions(n_angles):
    """the table cluster.boxes forms: (cos, sin) of theta_k = k (pi / 2) / n_angles, float64, by numpy on the host"""
    th = np.arange(int(n_angles), dtype=np.float64) * (np.pi / 2) / int(n_angles)
    return np.ascontiguousarray(np.stack([np.cos(th), np.sin(th)], 1))


def rectangles(P, cl, dirs):
    """rect float64 [kept][8] = k, u_min, u_max, v_min, v_max, y_min, y_max, area of the first direction of the smallest area"""
    P = np.asarray(P).reshape(-1, 3).astype(np.float64)
    dirs = np.asarray(dirs, np.float64).reshape(-1, 2)
    out = np.zeros((cl["kept"], RECT))
    for c in range(cl["kept"]):
        Q = P[cl["members"][cl["off"][c]:cl["off"][c + 1]]]
        x, y, z = Q[:, 0:1], Q[:, 1], Q[:, 2:3]
        cs, sn = dirs[None, :, 0], dirs[None, :, 1]
        a = x * cs; b = z * sn; u = a + b
        a = z * cs; b = x * sn; v = a - b
        ulo, uhi, vlo, vhi = u.min(0) + 0.0, u.max(0) + 0.0, v.min(0) + 0.0, v.max(0) + 0.0
        area = (uhi - ulo) * (vhi - vlo)
        k = 0
        for j in range(1, len(dirs)):                                    # the first of the smallest, as the kernel walks the table
            if area[j] < area[k]:
                k = j
        out[c] = [k, ulo[k], uhi[k], vlo[k], vhi[k], y.min() + 0.0, y.max() + 0.0, area[k]]
    return out


# ---- cases ------------------------------------------------------------------------------------------------------------------------------
EPS = 0.5


def _blobs(rng, n, centres, sigma=0.08):
    c = np.asarray(centres, np.float64)
    return f32(c[rng.integers(0, len(c), n)] + rng.normal(0, sigma, (n, 3)))


def _case(P, mask=None, f64=False, **kw):
    P = np.asarray(P, np.float64).reshape(-1, 3)
    P = P if f64 else P.astype(np.float32)
    kw = dict(dict(eps=EPS, min_points=3, max_points=None, max_clusters=16), **kw)
    return {"points": P, "mask": None if mask is None else np.asarray(mask, np.uint8), "kw": kw}


@functools.lru_cache(maxsize=None)
def cluster_cases():
    """name -> {'points' float32 or float64 [N][3], 'mask' uint8 [N] or None, 'kw'}; never modified"""
    rng = np.random.default_rng(11)
    out = {}
    centres = [[0, 0, 8], [3, 0.5, 9], [-4, 1, 12], [6, -1, 15], [0.2, 0, 20]]
    # (4095 ... 8193: the scan over N runs 4096 elements per round, so these cross one and two rounds and carry between them)
    for n in (0, 1, 2, 63, 64, 65, 1023, 1024, 1025, 2049, 4095, 4096, 4097, 8193):
        out["n%d" % n] = _case(_blobs(rng, n, centres), min_points=1 if n < 63 else 5)
    e = float(np.float32(EPS))
    out["exactly_eps_apart"] = _case([[0, 0, 8], [e, 0, 8]], f64=True, min_points=1)
    out["just_below_eps"] = _case([[0, 0, 8], [np.nextafter(e, 0.0), 0, 8]], f64=True, min_points=1)
    # a chain of 3000 points 0.9 eps apart on an outward spiral (its turns 1.5 m apart) crossing many cells, indices shuffled: one long
    # component, the worst case for the depth of the unions
    th, chain = 0.0, []
    for k in range(3000):
        r = 20.0 + 1.5 * th / (2 * np.pi)
        chain.append([r * np.sin(th), 0.2 * np.sin(0.05 * k), 60.0 + r * np.cos(th)])
        th += 0.9 * EPS / r
    chain = np.array(chain)
    step = np.linalg.norm(np.diff(f32(chain), axis=0), axis=1)
    assert 0.8 * EPS < step.min() and step.max() < 0.95 * EPS
    out["chain"] = _case(chain[rng.permutation(3000)], min_points=10)
    # points on exact cell boundaries -- multiples of the cell width, float64, where floor(p / cell) may round either way -- at negative
    # coordinates too, each with a companion 0.2 m along x
    cell = float(np.float32(EPS)) * (1.0 + 1.0 / 1048576.0)
    g = np.arange(-4, 5) * cell
    lat = np.stack(np.meshgrid(g, g[3:6], g, indexing="ij"), -1).reshape(-1, 3)
    out["cell_boundaries"] = _case(np.concatenate([lat, lat + [0.2, 0.0, 0.0], lat * [1, 1, -1] - [20.0, 3.0, 20.0]]), f64=True, min_points=1,
                                   max_clusters=512)
    out["identical"] = _case(np.tile([[1.25, -0.5, 7.0]], (300, 1)), min_points=300)
    far = rng.integers(-900, 900, (400, 3)) * 37.0                      # several hundred scattered far cells: bucket collisions
    out["far_cells"] = _case(np.repeat(far, 3, 0) + rng.normal(0, 0.05, (1200, 3)), min_points=3, max_clusters=512)
    a, b = _blobs(rng, 40, [[0, 0, 8]], 0.05), _blobs(rng, 40, [[0.8, 0, 8]], 0.05)
    bridge = np.array([[0.4, 0, 8]])
    out["masked_bridge"] = _case(np.concatenate([a, bridge, b]), mask=np.r_[np.ones(40), 0, np.ones(40)])
    out["open_bridge"] = _case(np.concatenate([a, bridge, b]), mask=np.ones(81))
    bad = np.concatenate([a, [[np.nan, 0, 8], [0, np.inf, 8], [0, 0, -np.inf]], b])
    out["nonfinite"] = _case(bad[rng.permutation(len(bad))], mask=np.ones(len(bad)))
    out["nonfinite_masked_out"] = _case(np.concatenate([a, [[np.nan, 0, 8]]]), mask=np.r_[np.ones(40), 0])
    tight = lambda n, c: np.asarray(c, np.float64) + np.stack([np.arange(n) * 0.13, np.zeros(n), np.zeros(n)], 1)       # noqa: E731
    out["min_points_edge"] = _case(np.concatenate([tight(10, [0, 0, 8]), tight(9, [0, 3, 8]), tight(11, [0, 6, 8])]), min_points=10)
    out["max_points_edge"] = _case(np.concatenate([tight(20, [0, 0, 8]), tight(21, [0, 3, 8]), tight(19, [0, 6, 8])]), min_points=3, max_points=20)
    sixteen = np.concatenate([tight(4, [0, 3.0 * k, 8]) for k in range(16)])
    out["exactly_max_clusters"] = _case(sixteen[rng.permutation(64)], min_points=4, max_clusters=16)
    seventeen = np.concatenate([tight(4, [0, 3.0 * k, 8]) for k in range(17)])
    out["one_over_max_clusters"] = _case(seventeen[rng.permutation(68)], min_points=4, max_clusters=16)
    out["float64_input"] = _case(_blobs(rng, 500, centres) + rng.normal(0, 1e-9, (500, 3)), f64=True, min_points=5)
    out["all_masked_out"] = _case(_blobs(rng, 70, centres), mask=np.zeros(70))
    for c in out.values():
        c["points"].setflags(write=False)
    return out


THRESHOLD_CASES = ("exactly_eps_apart", "just_below_eps")                # the two cases scipy's non-strict test may not be asked about


@functools.lru_cache(maxsize=None)
def cluster_refs():
    return {k: clusters(c["points"], c["mask"], **c["kw"]) for k, c in cluster_cases().items()}


def _rot(P, ang, centre):
    c, s = np.cos(ang), np.sin(ang)
    Q = np.asarray(P, np.float64) - centre
    return np.stack([c * Q[:, 0] - s * Q[:, 2], Q[:, 1], s * Q[:, 0] + c * Q[:, 2]], 1) + centre


@functools.lru_cache(maxsize=None)
def box_cases():
    """name -> {'points', 'kw', 'n_angles' or 'dirs'}: the clusters come from the restatement, the rectangles are what is compared"""
    rng = np.random.default_rng(12)
    out = {}
    slab = lambda n, c: np.asarray(c, np.float64) + rng.uniform(-1, 1, (n, 3)) * [2.1, 0.7, 0.9]       # noqa: E731
    axis = np.concatenate([slab(300, [0, 0, 10]), slab(200, [9, 0.5, 14])])
    out["axis_aligned"] = dict(_case(axis, eps=1.0, min_points=10), n_angles=90)
    rot = np.concatenate([_rot(slab(300, [0, 0, 10]), 0.4, [0, 0, 10]), _rot(slab(257, [9, 0, 14]), -1.1, [9, 0, 14]),
                          _rot(slab(64, [-9, 0, 20]), 1.3, [-9, 0, 20])])
    out["rotated"] = dict(_case(rot[rng.permutation(len(rot))], eps=1.0, min_points=10), n_angles=90)
    out["rotated_f64"] = dict(_case(rot + rng.normal(0, 1e-9, rot.shape), f64=True, eps=1.0, min_points=10), n_angles=45)
    out["single_point"] = dict(_case([[1.5, -0.25, 7.0], [30, 0, 9]], min_points=1), n_angles=90)
    # a square's corners, centred on the origin of (x, z): the directions 0 and pi / 4 ... give different areas, 0 and the table's repeat of it
    # (an explicit second (1, 0) row) tie, and the first wins
    sq = np.array([[-1, 0, 9], [1, 0, 9], [-1, 0, 11], [1, 0.5, 11]], np.float64)
    out["tie_first_wins"] = dict(_case(sq, eps=4.0, min_points=4), dirs=np.array([[np.cos(0.3), np.sin(0.3)], [1.0, 0.0], [np.cos(0.7), np.sin(0.7)], [1.0, 0.0],
                                                                                   [0.0, 1.0]]))
    out["one_direction"] = dict(_case(rot, eps=1.0, min_points=10), n_angles=1)
    out["k_not_multiple_of_64"] = dict(_case(rot, eps=1.0, min_points=10), n_angles=257 + 64)
    out["k_most"] = dict(_case(axis, eps=1.0, min_points=10), n_angles=1024)
    for c in out.values():
        c["points"].setflags(write=False)
        c["dirs"] = directions(c.pop("n_angles")) if "n_angles" in c else np.ascontiguousarray(c["dirs"], np.float64)
    return out


@functools.lru_cache(maxsize=None)
def box_refs():
    out = {}
    for k, c in box_cases().items():
        cl = clusters(c["points"], c["mask"], **c["kw"])
        out[k] = (cl, rectangles(c["points"], cl, c["dirs"]))
    return out


# ---- the planted scene ------------------------------------------------------------------------------------------------------------------
SCENE = dict(scale=2.0, poses=((0.5, (-4.0, 0.9, 12.0)), (-0.9, (2.5, 0.9, 17.0)), (1.9, (7.0, 0.9, 24.0))), eps=0.5, min_points=30, n_angles=90,
             gates={"length": (1.0, 8.0), "width": (0.5, 3.5), "height": (0.5, 3.5)})


@functools.lru_cache(maxsize=None)
def planted_scene():
    """The asset shape meshed at R = 24 (tests/_complete_traj.completion_case) seen at three poses some metres apart -- its camera-facing
    vertices --, a ground sheet that the mask removes, a wall that the gates reject and sparse strays under min_points.  dict: points float32
    [N][3] (shuffled), mask uint8 [N], truth: per object (yaw, centre [3] in the camera frame, metres), owner int32 [N] (object number, -1
    ground, -2 wall, -3 stray), z_true."""
    from tests import _complete_traj as CT
    case = CT.completion_case()
    v = case["vertices"].astype(np.float64)
    _, g = CT._values(case["z_true"][0], case["vertices"])
    n = g / np.linalg.norm(g, axis=1, keepdims=True)
    sc = SCENE["scale"]
    pts, owner, truth = [], [], []
    for k, (yaw, centre) in enumerate(SCENE["poses"]):
        cs, sn, t = np.cos(yaw), np.sin(yaw), np.asarray(centre, np.float64) / sc

        def rot(x):                                                      # rot_yaw diag(1, -1, 1) x, as _complete_traj poses its shape
            xs = x * np.array([1.0, -1.0, 1.0])
            return np.stack([cs * xs[:, 0] + sn * xs[:, 2], xs[:, 1], -sn * xs[:, 0] + cs * xs[:, 2]], 1)

        cam, ncam = sc * (rot(v) + t), rot(n)
        facing = (ncam * cam).sum(1) < 0
        pts.append(cam[facing]); owner.append(np.full(int(facing.sum()), k))
        truth.append((float(yaw), np.asarray(centre, np.float64)))
    rng = np.random.default_rng(13)
    gx, gz = np.meshgrid(np.arange(-12, 12, 0.4), np.arange(6, 32, 0.4))
    ground = np.stack([gx.ravel(), np.full(gx.size, 2.6), gz.ravel()], 1) + rng.normal(0, 0.01, (gx.size, 3))
    wx, wy = np.meshgrid(np.arange(-11, 1, 0.3), np.arange(-1.0, 2.0, 0.3))
    wall = np.stack([wx.ravel(), wy.ravel(), np.full(wx.size, 30.0)], 1) + rng.normal(0, 0.01, (wx.size, 3))
    strays = np.stack([rng.uniform(-12, 12, 40), rng.uniform(-3, -1.5, 40), rng.uniform(6, 28, 40)], 1)
    pts += [ground, wall, strays]
    owner += [np.full(len(ground), -1), np.full(len(wall), -2), np.full(len(strays), -3)]
    P, owner = np.concatenate(pts).astype(np.float32), np.concatenate(owner).astype(np.int32)
    perm = rng.permutation(len(P))
    P, owner = P[perm], owner[perm]
    mask = (owner != -1).astype(np.uint8)
    for a in (P, owner, mask):
        a.setflags(write=False)
    return {"points": P, "mask": mask, "owner": owner, "truth": truth, "z_true": case["z_true"][0]}
