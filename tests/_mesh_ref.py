"""A numpy restatement of the mesh extraction ("Meshes": marching tetrahedra on the Kuhn subdivision, welded) and, below it,
invariant checkers that know nothing about how the mesh was made.

The restatement follows the rules literally and in float32 with the operation order of csrc/mesh_cells.h, so its output is compared with the
kernels' bit for bit.  It derives everything (tetrahedra, triangle templates, winding) from first principles; the header uses constant tables,
and the equality tests are what ties the two together.
"""
import itertools

import numpy as np

AXIS_BIT = (4, 2, 1)                                   # corner / edge-class codes: x is the high bit
PERMS = list(itertools.permutations((0, 1, 2)))
# the six tetrahedra of a cell: corner codes along the walk 000 -> 111, one axis at a time
TETS = [(0, AXIS_BIT[p[0]], AXIS_BIT[p[0]] | AXIS_BIT[p[1]], 7) for p in PERMS]


def code_offset(c):
    return np.array(((c >> 2) & 1, (c >> 1) & 1, c & 1), dtype=np.int64)


def lattice_coords(R):
    """x_i = float32(-1 + 2 i / (R - 1)), evaluated in float64"""
    return (-1.0 + 2.0 * np.arange(R, dtype=np.float64) / float(R - 1)).astype(np.float32)


def lattice_points(R):
    """[R^3][3] float32, z fastest"""
    c = lattice_coords(R)
    X, Y, Z = np.meshgrid(c, c, c, indexing="ij")
    return np.stack([X, Y, Z], -1).reshape(-1, 3)


def _templates(mask):
    """triangles of a tetrahedron whose corners i with bit i of `mask` are inside, before the winding is settled: a list of triangles, each
    three edges (inside corner, outside corner) given by their positions in the tetrahedron"""
    I = [i for i in range(4) if mask >> i & 1]
    O = [i for i in range(4) if not mask >> i & 1]
    if len(I) == 1:
        return [[(I[0], O[0]), (I[0], O[1]), (I[0], O[2])]]
    if len(I) == 3:
        return [[(I[0], O[0]), (I[1], O[0]), (I[2], O[0])]]
    if len(I) == 2:
        q = [(I[0], O[0]), (I[0], O[1]), (I[1], O[1]), (I[1], O[0])]
        return [[q[0], q[1], q[2]], [q[0], q[2], q[3]]]
    return []


def _flipped(tet, mask):
    """does the template's first triangle, with every crossing at the edge's midpoint, face from outside to inside?  Integer arithmetic on
    doubled lattice coordinates: the midpoint of corners a and b is a + b."""
    corners = [code_offset(c) for c in TETS[tet]]
    tri = _templates(mask)[0]
    q = [corners[i] + corners[o] for i, o in tri]
    n = np.cross(q[1] - q[0], q[2] - q[0])
    I = [i for i in range(4) if mask >> i & 1]
    O = [i for i in range(4) if not mask >> i & 1]
    out_dir = len(I) * sum(corners[o] for o in O) - len(O) * sum(corners[i] for i in I)
    d = int(np.dot(n, out_dir))
    assert d != 0
    return d < 0


def tet_triangles(tet, mask):
    """the triangles of tetrahedron `tet` for inside mask `mask`, wound so that the normal points from inside to outside; each vertex is an
    edge (lower corner position, higher corner position)"""
    tris = _templates(mask)
    if tris and _flipped(tet, mask):
        tris = [[t[0], t[2], t[1]] for t in tris]
    return [[(min(e), max(e)) for e in t] for t in tris]


def extract(sdf):
    """sdf [R][R][R] float32 -> (vertices float32 [V][3], faces int32 [T][3], aux) for one shape.  aux: 'mask' uint8 [R^3] (the crossing
    mask of each point's owned edges) and 'tcount' uint8 [R^3] (the triangle count of each point's cell)."""
    sdf = np.ascontiguousarray(sdf, dtype=np.float32)
    R = sdf.shape[0]
    assert sdf.shape == (R, R, R) and 2 <= R <= 256
    N = R ** 3
    s = sdf.reshape(-1)
    with np.errstate(invalid="ignore"):
        inside = (sdf < 0)                                        # an exact 0 and a NaN are outside
    coords = lattice_coords(R)
    ii = np.arange(R)
    IX, IY, IZ = np.meshgrid(ii, ii, ii, indexing="ij")
    rows = ((IX * R + IY) * R + IZ)
    # -- vertices: one per crossing edge, ordered by (owner row, class)
    cross = np.zeros((N, 7), dtype=bool)
    for c in range(1, 8):
        d = code_offset(c)
        ok = (IX + d[0] < R) & (IY + d[1] < R) & (IZ + d[2] < R)
        a = rows[ok]
        b = a + (d[0] * R + d[1]) * R + d[2]
        cross[a, c - 1] = inside.reshape(-1)[a] != inside.reshape(-1)[b]
    own, cls = np.nonzero(cross)                                  # row-major: (owner row, class)
    vid = np.full((N, 7), -1, dtype=np.int64)
    vid[own, cls] = np.arange(own.size)
    d = np.stack([(cls + 1) >> 2 & 1, (cls + 1) >> 1 & 1, (cls + 1) & 1], 1)
    ia = np.stack([own // (R * R), own // R % R, own % R], 1)
    pa, pb = coords[ia], coords[ia + d]
    sa, sb = s[own], s[own + (d[:, 0] * R + d[:, 1]) * R + d[:, 2]]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        t = sa / (sa - sb)
    t = np.where(np.isnan(t), np.float32(0.5), t).astype(np.float32)     # a NaN or infinite neighbour: the midpoint
    prod = (t[:, None] * (pb - pa)).astype(np.float32)
    verts = (pa + prod).astype(np.float32)
    # -- triangles: ordered by (cell row of the low corner, tetrahedron, triangle)
    cell = (IX < R - 1) & (IY < R - 1) & (IZ < R - 1)
    crow = rows[cell]
    fl = inside.reshape(-1)
    keys, tris = [], []
    tcount = np.zeros(N, dtype=np.uint8)
    for tet, codes in enumerate(TETS):
        corner_rows = [crow + int((code_offset(c)[0] * R + code_offset(c)[1]) * R + code_offset(c)[2]) for c in codes]
        m = sum(fl[r].astype(np.int64) << i for i, r in enumerate(corner_rows))
        for mask in range(1, 15):
            sel = np.nonzero(m == mask)[0]
            if sel.size == 0:
                continue
            for k, tri in enumerate(tet_triangles(tet, mask)):
                f = np.stack([vid[corner_rows[lo][sel], (codes[hi] ^ codes[lo]) - 1] for lo, hi in tri], 1)
                assert (f >= 0).all()
                tris.append(f)
                keys.append((crow[sel] * 6 + tet) * 2 + k)
                np.add.at(tcount, crow[sel], 1)
    if tris:
        keys, tris = np.concatenate(keys), np.concatenate(tris)
        faces = tris[np.argsort(keys, kind="stable")].astype(np.int32)
    else:
        faces = np.zeros((0, 3), dtype=np.int32)
    mask7 = (cross.astype(np.uint8) << np.arange(7, dtype=np.uint8)).sum(1).astype(np.uint8)
    return verts, faces, {"mask": mask7, "tcount": tcount}


# ---- test shapes -------------------------------------------------------------------------------------------------------------------------

def shape_sdf(name, R):
    """float32 [R][R][R] samples of an analytic shape on the lattice"""
    p = lattice_points(R).astype(np.float64)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    if name == "sphere":
        v = np.sqrt(x * x + y * y + z * z) - 0.6
    elif name == "ellipsoid":
        v = (np.sqrt((x / 0.8) ** 2 + (y / 0.45) ** 2 + (z / 0.6) ** 2) - 1.0) * 0.45
    elif name == "torus":
        v = np.sqrt((np.sqrt(x * x + y * y) - 0.55) ** 2 + z * z) - 0.27
    elif name == "octahedron":                      # zeros exactly at lattice points when 0.5 is a multiple of the spacing
        v = np.abs(x) + np.abs(y) + np.abs(z) - 0.5
    elif name == "cut_sphere":                      # leaves the cube through the face x = 1
        v = np.sqrt((x - 0.8) ** 2 + y * y + z * z) - 0.5
    else:
        raise KeyError(name)
    return v.astype(np.float32).reshape(R, R, R)


# ---- invariants (independent of the extraction) -------------------------------------------------------------------------------------------

def undirected_edge_counts(faces):
    """how many triangles use each undirected edge: the array of multiplicities"""
    f = np.asarray(faces, dtype=np.int64)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    e.sort(axis=1)
    _, cnt = np.unique(e, axis=0, return_counts=True)
    return cnt


def is_closed(faces):
    cnt = undirected_edge_counts(faces)
    return bool(cnt.size > 0 and (cnt == 2).all())


def directed_edges_paired(faces):
    """every directed edge appears exactly once, and so does its reverse"""
    f = np.asarray(faces, dtype=np.int64)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    n = int(f.max()) + 1 if f.size else 1
    key = e[:, 0] * n + e[:, 1]
    rev = e[:, 1] * n + e[:, 0]
    u, cnt = np.unique(key, return_counts=True)
    return bool((cnt == 1).all() and np.array_equal(u, np.unique(rev)))


def euler_characteristic(faces):
    f = np.asarray(faces, dtype=np.int64)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    e.sort(axis=1)
    return int(np.unique(f).size - np.unique(e, axis=0).shape[0] + f.shape[0])


def signed_volume(vertices, faces):
    v = np.asarray(vertices, dtype=np.float64)
    a, b, c = (v[np.asarray(faces)[:, k]] for k in range(3))
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)


def triangle_areas(vertices, faces):
    v = np.asarray(vertices, dtype=np.float64)
    a, b, c = (v[np.asarray(faces)[:, k]] for k in range(3))
    return 0.5 * np.linalg.norm(np.cross(b - a, c - a), axis=1)
