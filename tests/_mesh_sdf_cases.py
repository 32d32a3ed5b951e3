"""Test meshes and query points of the signed distance to meshes.  Every case is (vertices float32 [V][3], faces int32 [T][3], points float32
[n][3], want_sign).  Small on purpose: the restatement loops over the triangles in Python.  references() computes the restatement once per
process; nobody modifies what it returns."""
import functools

import numpy as np

from tests import _mesh_ref as MR
from tests import _mesh_sdf_ref as SR

RADIUS = 0.7
SEED = 7                       # chosen so that no point of any signed case has | |w| - 0.5 | <= 1e-6 (tests/test_mesh_sdf_cpu.py asserts it)


def icosphere(level, radius=RADIUS):
    """the icosahedron subdivided `level` times, vertices on the sphere, wound outward: 20 * 4^level triangles"""
    g = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1), (-g, 0, -1), (-g, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4), (3, 4, 2),
         (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.asarray(x, np.float64) / np.linalg.norm(x) for x in v]
    for _ in range(level):
        mid, nf = {}, []

        def m(i, j):
            k = (min(i, j), max(i, j))
            if k not in mid:
                x = v[i] + v[j]
                v.append(x / np.linalg.norm(x))
                mid[k] = len(v) - 1
            return mid[k]

        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    v, f = np.asarray(v) * radius, np.asarray(f, np.int32)
    flip = np.einsum("ij,ij->i", v[f[:, 0]], np.cross(v[f[:, 1]], v[f[:, 2]])) < 0
    f[flip] = f[flip][:, [0, 2, 1]]
    return v.astype(np.float32), f


def unit_cube():
    """[0, 1]^3, two triangles per face split along the diagonal from the face's lowest corner, wound outward"""
    v = np.array([(x, y, z) for x in (0, 1) for y in (0, 1) for z in (0, 1)], np.float32)            # index 4 x + 2 y + z
    f = np.array([(0, 1, 3), (0, 3, 2), (4, 6, 7), (4, 7, 5), (0, 4, 5), (0, 5, 1), (2, 3, 7), (2, 7, 6), (0, 2, 6), (0, 6, 4), (1, 5, 7), (1, 7, 3)],
                 np.int32)
    return v, f


def cube_tie_points():
    """exactly on the vertices, on edge midpoints, on the face diagonals (shared by two triangles), at face centres and at the cube's centre"""
    v, _ = unit_cube()
    edges = [(a + b) / 2 for a in v for b in v if np.abs(a - b).sum() == 1 and tuple(a) < tuple(b)]
    diag = [np.array(p, np.float32) for p in ((0, .25, .25), (0, .5, .5), (1, .75, .75), (.25, 0, .25), (.5, 1, .5), (.25, .25, 0), (.75, .75, 1))]
    return np.concatenate([v, np.asarray(edges, np.float32), np.asarray(diag, np.float32), np.array([[.5, .5, .5]], np.float32)])


def lattice_mesh(name, R=16):
    v, f, _ = MR.extract(MR.shape_sdf(name, R))
    return v, f


def broken_mesh():
    """a closed icosphere of 80 triangles plus what the kernels must skip or cope with: zero-area triangles (a repeated vertex, three collinear
    vertices, three equal vertices), a triangle with a NaN vertex and one with an infinite one, face indices below 0 and beyond the mesh"""
    v, f = icosphere(1)
    nv = len(v)
    extra_v = np.array([[np.nan, 0, 0], [np.inf, 0, 0], [0.9, 0.9, 0.9], [0.8, 0.8, 0.8], [0.7, 0.7, 0.7]], np.float32)
    extra_f = np.array([(0, 0, 1), (nv + 2, nv + 3, nv + 4), (5, 5, 5), (0, 1, nv), (2, nv + 1, 3), (-1, 0, 1), (0, 1, nv + 5), (2, 3, 1 << 30)], np.int32)
    # in the middle of the list, so that the triangles behind them keep their indices' meaning
    return np.concatenate([v, extra_v]), np.concatenate([f[:40], extra_f, f[40:]]).astype(np.int32)


def uniform_points(rng, n, half=1.0):
    return rng.uniform(-half, half, (n, 3)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def cases():
    rng = np.random.default_rng(SEED)
    out = {}
    iv, if_ = icosphere(3)
    out["icosphere"] = (iv, if_, uniform_points(rng, 2000), True)
    for name in ("sphere", "torus"):
        v, f = lattice_mesh(name)
        out["lattice_" + name] = (v, f, uniform_points(rng, 400), True)
    cv, cf = unit_cube()
    out["cube_ties"] = (cv, cf, cube_tie_points(), False)                  # on the surface the sign is undefined: the unsigned distance
    out["cube"] = (cv, cf, uniform_points(rng, 200, 1.0) * np.float32(0.75) + np.float32(0.5), True)
    keep = np.ones(len(if_), bool)
    keep[rng.choice(len(if_), 40, replace=False)] = False
    out["open"] = (iv, if_[keep], uniform_points(rng, 300), True)
    out["reversed"] = (iv, np.ascontiguousarray(if_[:, [0, 2, 1]]), uniform_points(rng, 300), True)
    bv, bf = broken_mesh()
    out["broken"] = (bv, bf, uniform_points(rng, 300), True)
    out["empty_mesh"] = (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), uniform_points(rng, 5), True)
    out["empty_queries"] = (cv, cf, np.zeros((0, 3), np.float32), True)
    q = uniform_points(rng, 6)
    q[1, 0], q[3, 2], q[4, 1] = np.nan, np.inf, -np.inf
    out["nonfinite_query"] = (cv, cf, q, True)
    v4, f4 = icosphere(4)                                                  # 5120 triangles: two chunks
    big = uniform_points(rng, 3000)
    out["two_chunks"] = (v4, f4, big, True)
    out["two_chunks_few"] = (v4, f4, big[:3].copy(), True)
    out["one_chunk_exactly"] = (v4, f4[:4096].copy(), uniform_points(rng, 40), True)
    return out


CLOSED = ("icosphere", "lattice_sphere", "lattice_torus", "cube", "reversed", "broken", "two_chunks")
SMALL = ("cube_ties", "cube", "broken", "empty_mesh", "empty_queries", "nonfinite_query", "two_chunks_few", "one_chunk_exactly")


@functools.lru_cache(maxsize=None)
def references():
    """name -> the restatement's dict for the case's own want_sign"""
    out = {}
    for n, (v, f, p, ws) in cases().items():
        if n == "two_chunks_few":
            continue
        out[n] = SR.mesh_sdf(v, f, p, ws)
    out["two_chunks_few"] = {k: (x[:3] if isinstance(x, np.ndarray) else x) for k, x in out["two_chunks"].items()}
    return out


@functools.lru_cache(maxsize=None)
def unsigned_references():
    """the same with want_sign = 0: dist, d2 and nearest are those of references(), the winding is 0 and sdf = dist"""
    out = {}
    for n, r in references().items():
        out[n] = dict(r, sdf=r["dist"], winding=np.zeros(len(r["dist"])))
    return out


def uniforms(name, n=600):
    """the sampler's uniforms of a case: float32 [n][3] in [0, 1), with the corners of the range among them"""
    rng = np.random.default_rng(hash_name(name) + SEED)
    u = rng.random((n, 3), dtype=np.float32)
    if n >= 4:
        u[0], u[1], u[2] = 0.0, np.float32(1.0) - np.float32(2.0 ** -24), (0.0, 0.0, 0.5)
        u[3] = (0.5, np.float32(1.0) - np.float32(2.0 ** -24), 0.0)
    return u


def hash_name(name):
    return sum((i + 1) * ord(c) for i, c in enumerate(name))


def pack(names):
    """the ragged batch of the named cases: (vertices, faces, voff, toff, points, qoff)"""
    cs = cases()
    vs, fs, ps = [cs[n][0] for n in names], [cs[n][1] for n in names], [cs[n][2] for n in names]
    off = lambda xs: np.concatenate([[0], np.cumsum([len(x) for x in xs])]).astype(np.int64)
    cat = lambda xs, dt: np.ascontiguousarray(np.concatenate([np.asarray(x, dt).reshape(-1, 3) for x in xs])) if xs else np.zeros((0, 3), dt)
    return cat(vs, np.float32), cat(fs, np.int32), off(vs), off(fs), cat(ps, np.float32), off(ps)


# ---- bounds and comparisons shared by the host and the device tests ---------------------------------------------------------------------------

EPS64 = 2.0 ** -52


def winding_bound(ref, T):
    """rounding of a sequential sum of T terms, each atan2 and its division good to a few ulp: (T + 8) eps (1 + sum |omega_t|)"""
    return (T + 8) * EPS64 * (1.0 + ref["abs_winding"])


def lattice_bound(R=16, radius=0.6):
    """How far the marching-tetrahedra mesh of the sphere |x| - radius on the R-lattice can be from that sphere.  Spacing h = 2 / (R - 1); an
    edge of the Kuhn subdivision is at most L = sqrt(3) h long, and so is a triangle's diameter (it lies in one cell).
      a vertex is the zero of the linear interpolant of f = |x| - radius along an edge; |f''| <= 1 / |x| <= 1 / (radius - L) along it, so the
        interpolation error, which is the vertex's distance from the sphere because |grad f| = 1, is at most delta = L^2 / (8 (radius - L));
      a point x = sum l_i v_i of a triangle has |x|^2 = sum l_i |v_i|^2 - sum_{i<j} l_i l_j |v_i - v_j|^2 >= (radius - delta)^2 - L^2 / 3,
        and |x| <= radius + delta: the chord sag.
    The mesh lies in that shell and every ray from the origin meets it, so distances to the mesh and to the sphere differ by at most
    e = max(delta, radius - sqrt((radius - delta)^2 - L^2 / 3))."""
    h = 2.0 / (R - 1)
    L = 3.0 ** 0.5 * h
    delta = L * L / (8.0 * (radius - L))
    return max(delta, radius - ((radius - delta) ** 2 - L * L / 3.0) ** 0.5), h


def check_against(out, names, cases, refs, signed, what="host"):
    """bits for everything but the winding number, which is held to its rounding bound"""
    o = 0
    for b, n in enumerate(names):
        r, k = refs[n], len(cases[n][2])
        for key in ("sdf", "dist", "d2", "nearest"):
            assert out[key][o:o + k].tobytes() == r[key].tobytes(), (what, n, key)
        dev = np.abs(out["winding"][o:o + k] - r["winding"])
        if k and signed:
            bound = winding_bound(references()[n], len(cases[n][1]))
            print("%s %-18s max winding difference %.2e (bound %.2e)" % (what, n, dev.max(), bound.min()))
            assert (dev <= bound).all(), (what, n)
        else:
            assert not dev.any(), (what, n)
        assert out["flags"][b] == r["flags"], (what, n)
        o += k
    assert o == len(out["sdf"])


def check_surface(out, names, cases, us, soff):
    for b, n in enumerate(names):
        pts, tri, flags = SR.surface_points(cases[n][0], cases[n][1], us[b])
        s0, s1 = soff[b], soff[b + 1]
        assert out["spoints"][3 * s0:3 * s1].tobytes() == pts.tobytes() and out["striangle"][s0:s1].tobytes() == tri.tobytes(), n
        assert out["sflags"][b] == flags, n
