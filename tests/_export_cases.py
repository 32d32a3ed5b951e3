"""The export's test batches, shared by tests/test_export_cpu.py (restatement and host build of the header) and tests/test_gpu_export.py
(the kernels): the 64 x 48 meshes of tests/_verify_cases.py with per-vertex attributes, boxes and colour crops."""
import numpy as np

from tests import _verify_cases as VC

W, H = VC.W, VC.H


POSE_CUBE = dict(h=0.5, scale=2.0, trans=(2.5, -1.75, 4.0))


def posed_cube(h=0.5, scale=2.0, trans=(2.5, -1.75, 4.0)):
    """A cube [-h, h]^3 of the lattice frame seen off-axis, so that three of its faces are in sight: camera vertices
    diag(1, -1, 1) scale a + trans with dyadic numbers only, so they are exact in float32 and the analytic ray-box intersection speaks about
    the very same solid.  Returns (camera vertices, faces, lattice vertices)."""
    a = np.array([[x, y, z] for z in (-h, h) for y in (-h, h) for x in (-h, h)], np.float64)
    cam = a * np.array([1.0, -1.0, 1.0]) * scale + np.asarray(trans, np.float64)
    assert np.array_equal(cam.astype(np.float32).astype(np.float64), cam)
    f = VC.faces((0, 1, 3), (0, 3, 2), (4, 7, 5), (4, 6, 7), (0, 4, 5), (0, 5, 1), (2, 3, 7), (2, 7, 6), (0, 2, 6), (0, 6, 4), (1, 5, 7), (1, 7, 3))
    return cam.astype(np.float32), f, a.astype(np.float32)


K_POSED = (41.3, 40.7, -3.6, 44.2)          # nothing round: few analytic values sit on a rounding boundary of the bytes


def colour_crop(rng, box):
    """float32 BGR of the box's shape: k / 255 values, and NaN, negative values, values above 1 and infinities sprinkled in"""
    h, w = max(box[3] - box[1], 0), max(box[2] - box[0], 0)
    c = (rng.integers(0, 256, (h, w, 3)).astype(np.float32) / np.float32(255.0)).astype(np.float32)
    flat = c.reshape(-1)
    if flat.size >= 12:
        flat[[0, 1, 2, 3, 4, 5, 6, 7]] = [np.nan, -0.5, 1.5, np.inf, -np.inf, 0.5 / 255, 1.5 / 255, 2.5 / 255]
        flat[8:12] = rng.uniform(-0.2, 1.2, 4).astype(np.float32)
    return c


def batches():
    """name -> dict(K, meshes [(v, f)], attrs, windows, boxes, colors (or None), triangles (or None), occlusion)"""
    c = VC.cases()
    rng = np.random.default_rng(11)
    out = {}

    def attr_for(v):
        a = rng.uniform(-1, 1, (len(v), 3)).astype(np.float32)
        return a

    def add(name, K, meshes, attrs, windows, boxes, occlusion=True, colors=True, triangles=None):
        out[name] = dict(K=K, meshes=meshes, attrs=attrs, windows=[tuple(w) for w in windows], boxes=[tuple(b) for b in boxes],
                         colors=[colour_crop(rng, b) for b in boxes] if colors else None, triangles=triangles, occlusion=occlusion)

    v, f = c["edges_through_samples"][:2]
    add("single_triangle", VC.K8, [(v, f)], [attr_for(v)], [VC.FULL], [VC.FULL])
    v, f = c["cube"][:2]
    cube_attr = np.stack([v[:, 0], -v[:, 1], v[:, 2] - 3.0], 1).astype(np.float32)
    add("cube_box_inside_window", VC.K_CUBE, [(v, f)], [cube_attr], [VC.FULL], [(20, 12, 44, 30)])
    v, f, a = posed_cube()
    add("posed_cube", K_POSED, [(v, f)], [a], [VC.FULL], [VC.FULL], colors=False)
    # two meshes with an exact depth tie where they overlap (both at Z = 2); different windows
    v, f = c["coplanar_overlap"][:2]
    m0, m1 = (v[3:6], VC.faces((0, 1, 2))), (v[0:3], VC.faces((0, 1, 2)))
    add("depth_tie", VC.K8, [m0, m1], [attr_for(m0[0]), attr_for(m1[0])], [VC.FULL, (8, 8, 40, 36)], [(10, 8, 40, 40), (8, 8, 40, 36)])
    # near over far; the near triangle is rendered into a window that holds only a part of it: outside that window it occludes nothing
    v, f = c["near_over_far"][:2]
    far, near = (v[0:3], VC.faces((0, 1, 2))), (v[3:6], VC.faces((0, 1, 2)))
    add("near_over_far", VC.K8, [far, near], [attr_for(far[0]), attr_for(near[0])], [VC.FULL, VC.FULL], [VC.FULL, (18, 8, 44, 32)])
    add("occluder_window_short", VC.K8, [far, near], [attr_for(far[0]), attr_for(near[0])], [VC.FULL, (18, 8, 30, 20)], [VC.FULL, (20, 10, 30, 20)])
    add("occlusion_off", VC.K8, [far, near], [attr_for(far[0]), attr_for(near[0])], [VC.FULL, VC.FULL], [VC.FULL, (18, 8, 44, 32)], occlusion=False)
    v, f = c["partly_outside_image"][:2]
    add("box_at_the_image_border", VC.K8, [(v, f)], [attr_for(v)], [(0, 0, 40, 48)], [(0, 0, 30, 48)])
    v, f = c["empty_window"][:2]
    add("empty_window", VC.K8, [(v, f)], [attr_for(v)], [c["empty_window"][3]], [c["empty_window"][3]])
    v, f = c["empty_mesh"][:2]
    add("empty_mesh", VC.K8, [(v, f)], [np.zeros((0, 3), np.float32)], [c["empty_mesh"][3]], [(6, 6, 18, 20)])
    v, f = c["nan_vertex"][:2]
    a = attr_for(v)
    a[7, 0] = np.nan                                          # triangle 3 = (7, 8, 9) wins everywhere: a NaN value gives byte 0
    add("nan_vertex", VC.K8, [(v, f)], [a], [VC.FULL], [VC.FULL])
    # all three values at -1 along the edge (10, 10)-(20, 10), which passes through sample points: (0, 0, 0) becomes (0, 0, 1) there
    v, f = c["edges_through_samples"][:2]
    add("zero_bytes", VC.K8, [(v, f)], [np.array([[-1, -1, -1], [-1, -1, -1], [-1, -1, 1]], np.float32)], [VC.FULL], [VC.FULL])
    v, f = c["edges_through_samples"][:2]
    tri = np.full((H, W), -1, np.int32)
    tri[10:21, 10:21] = 0
    tri[12, 12], tri[13, 13] = 7, -3                          # outside the mesh of one triangle
    add("bad_triangle_index", VC.K8, [(v, f), (v, f)], [attr_for(v), attr_for(v)], [VC.FULL, VC.FULL], [VC.FULL, (5, 5, 30, 30)],
        triangles=[tri, None], occlusion=False)
    add("box_outside_window", VC.K8, [(v, f), (v, f)], [attr_for(v), attr_for(v)], [(8, 8, 30, 30), VC.FULL], [(4, 8, 20, 20), VC.FULL], occlusion=False)
    return out


def sphere_batch():
    """the marching-tetrahedra sphere of tests/_verify_cases.py with its lattice vertices as attributes: (batch, scale, yaw, trans)"""
    from tests import _mesh_ref as MR
    v0, f0, _ = MR.extract(MR.shape_sdf("sphere", 24))
    scale, yaw, trans = 1.7, 0.7, (0.05, -0.02, 3.0)
    vc, fc = VC.to_camera(v0, f0, scale, yaw, trans)
    b = dict(K=VC.K_SPHERE, meshes=[(vc, fc)], attrs=[np.asarray(v0, np.float32)], windows=[VC.FULL], boxes=[VC.FULL], colors=None, triangles=None,
             occlusion=True)
    return b, scale, yaw, trans
