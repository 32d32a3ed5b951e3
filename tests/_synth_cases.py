"""The synthetic crops' test batches, shared by tests/test_synth_cpu.py (restatement and host build of the header) and
tests/test_gpu_synth.py (the kernels): the small meshes of tests/_verify_cases.py with per-vertex normals, scenes, paints, lights and
backgrounds.  Images are at most 64 x 48."""
import numpy as np

from tests import _verify_cases as VC

W, H = VC.W, VC.H
K_ODD = (41.3, 40.7, 30.4, 22.2)            # nothing round


def light_row(x, y, z, ambient, kd):
    l = np.array([x, y, z], np.float64)
    l = l / np.sqrt((l * l).sum())
    return [l[0], l[1], l[2], ambient, kd]


def outward(v):
    """unit normals pointing away from the centroid, float32"""
    d = np.asarray(v, np.float64) - np.asarray(v, np.float64).mean(0)
    return (d / np.linalg.norm(d, axis=1)[:, None]).astype(np.float32)


def batches():
    """name -> dict(K, size, meshes [(v, f)], normals, windows, boxes, paint [B][5], light [S][5], ramp [S][8], scene (or None), bg_index, bgs
    (or None), triangles (or None))"""
    c = VC.cases()
    rng = np.random.default_rng(23)
    out = {}

    def nrm_for(v):
        return rng.uniform(-1, 1, (len(v), 3)).astype(np.float32)

    def paint_row(ks=0.4, shin=4):
        return list(rng.uniform(0.2, 0.9, 3)) + [ks, shin]

    def ramp_row():
        return [int(x) for x in rng.integers(0, 256, 6)] + [int(rng.integers(0, 120)), int(rng.integers(0, 2 ** 31))]

    def add(name, K, meshes, normals, windows, boxes, scene=None, paint=None, S=None, bg_index=None, bgs=None, triangles=None, size=(W, H), light=None):
        B = len(meshes)
        S = S if S is not None else (1 if scene is None else max(scene) + 1)
        out[name] = dict(K=K, size=size, meshes=meshes, normals=normals, windows=[tuple(w) for w in windows], boxes=[tuple(b) for b in boxes],
                         scene=scene, paint=np.asarray(paint if paint is not None else [paint_row() for _ in range(B)], np.float64).reshape(B, 5),
                         light=np.asarray(light if light is not None else
                                          [light_row(*rng.uniform(-1, 1, 2), -rng.uniform(0.3, 1), rng.uniform(0.1, 0.4), rng.uniform(0.4, 0.9))
                                           for _ in range(S)], np.float64).reshape(S, 5),
                         ramp=np.asarray([ramp_row() for _ in range(S)], np.int32).reshape(S, 8), bg_index=bg_index, bgs=bgs, triangles=triangles)

    tet = np.array([[0.0, -1.0, 4.0], [-1.0, 0.7, 4.6], [1.1, 0.6, 4.4], [0.1, 0.2, 3.1]], np.float32)
    add("tetrahedron", K_ODD, [(tet, VC.faces((0, 1, 2), (0, 3, 1), (1, 3, 2), (2, 3, 0)))], [outward(tet)], [(1, 0, 64, 47)], [(1, 0, 64, 47)])
    cv, cf = VC.cube_mesh()
    # a 1-pixel box and a box equal to its window; the same mesh twice in one scene: every depth ties and the lower index owns
    add("one_pixel_box_and_whole_window", VC.K_CUBE, [(cv, cf), (cv, cf)], [outward(cv), outward(cv)], [VC.FULL, (10, 4, 41, 33)],
        [(30, 20, 31, 21), (10, 4, 41, 33)])
    v, f = c["partly_outside_image"][:2]
    add("window_clipped_at_the_image_corner", VC.K8, [(v, f)], [nrm_for(v)], [(0, 0, 40, 48)], [(0, 0, 30, 48)])
    v, f = c["near_over_far"][:2]
    far, near = (v[0:3], VC.faces((0, 1, 2))), (v[3:6], VC.faces((0, 1, 2)))
    # the occluder's window starts elsewhere: the owner's window pixel is not the annotation's own
    add("occluder_at_another_offset", VC.K8, [far, near], [nrm_for(far[0]), nrm_for(near[0])], [VC.FULL, (18, 8, 44, 32)], [VC.FULL, (18, 8, 44, 32)])
    add("occluder_window_short", VC.K8, [far, near], [nrm_for(far[0]), nrm_for(near[0])], [VC.FULL, (18, 8, 30, 20)], [(3, 2, 62, 45), (20, 10, 30, 20)])
    v, f = c["coplanar_overlap"][:2]
    m0, m1 = (v[3:6], VC.faces((0, 1, 2))), (v[0:3], VC.faces((0, 1, 2)))
    add("depth_tie", VC.K8, [m0, m1], [nrm_for(m0[0]), nrm_for(m1[0])], [VC.FULL, (8, 8, 40, 36)], [(10, 8, 40, 40), (8, 8, 40, 36)])
    # two scenes that overlap in pixel space, a third annotation in scene 0; scene 1 shows an image, scene 0 the ramp (index outside the images)
    bgs = [rng.integers(0, 256, (H, W, 3)).astype(np.uint8), rng.integers(0, 256, (H, W, 3)).astype(np.uint8)]
    add("two_scenes", VC.K8, [far, near, near], [nrm_for(far[0]), nrm_for(near[0]), nrm_for(near[0])],
        [VC.FULL, (16, 6, 46, 34), (18, 8, 44, 32)], [(2, 2, 60, 46), (16, 6, 46, 34), (19, 9, 43, 31)], scene=[0, 1, 0], bg_index=[7, 1], bgs=bgs)
    add("image_background", VC.K8, [far], [nrm_for(far[0])], [VC.FULL], [(0, 3, 61, 48)], bg_index=[0], bgs=bgs)
    # a triangle whose three normals are zero, and one with a NaN normal: the normal is 0, the colour albedo * ambient
    v, f = c["near_over_far"][:2]
    n = nrm_for(v)
    n[0:3] = 0.0
    n[4, 1] = np.nan
    add("zero_and_nan_normal", VC.K8, [(v, f)], [n], [VC.FULL], [(1, 1, 63, 47)])
    # shin 0 and 7 and ks = 0: the cube three times, each in a scene of its own, under one light direction
    li = [light_row(0.3, -0.5, -0.8, 0.2, 0.7)] * 3
    add("shin_0_7_and_ks_0", VC.K_CUBE, [(cv, cf)] * 3, [outward(cv)] * 3, [(12, 4, 52, 44)] * 3, [(12, 4, 52, 44)] * 3, scene=[0, 1, 2],
        paint=[[0.8, 0.5, 0.3, 0.5, 0], [0.8, 0.5, 0.3, 0.5, 7], [0.8, 0.5, 0.3, 0.0, 3]], light=li)
    # an image of one row: the ramp's denominator is max(H - 1, 1)
    K1 = (8.0, 8.0, 32.0, 0.0)
    row = VC.at([(10, -5, 1), (50, -5, 1), (30, 5, 1)], K1)
    add("one_row_image", K1, [(row, VC.faces((0, 1, 2)))], [nrm_for(row)], [(0, 0, 64, 1)], [(3, 0, 61, 1)], size=(64, 1))
    v, f = c["empty_mesh"][:2]
    add("empty_mesh", VC.K8, [(v, f)], [np.zeros((0, 3), np.float32)], [c["empty_mesh"][3]], [(6, 6, 18, 20)])
    v, f = c["empty_window"][:2]
    add("empty_window", VC.K8, [(v, f)], [nrm_for(v)], [c["empty_window"][3]], [c["empty_window"][3]])
    add("empty_window_beside_another", VC.K8, [(v, f), far], [nrm_for(v), nrm_for(far[0])], [c["empty_window"][3], VC.FULL],
        [c["empty_window"][3], (5, 5, 50, 40)])
    # a triangle image that does not belong to the mesh (7 and -3 for a mesh of one triangle): flag bit 1, zeros; the scene beside it untouched
    v, f = c["edges_through_samples"][:2]
    tri = np.full((H, W), -1, np.int32)
    tri[10:21, 10:21] = 0
    tri[12, 12], tri[13, 13] = 7, -3
    add("triangles_of_another_mesh", VC.K8, [(v, f), (v, f)], [nrm_for(v), nrm_for(v)], [VC.FULL, VC.FULL], [VC.FULL, (5, 5, 30, 30)], scene=[0, 1],
        triangles=[tri, None])
    add("box_outside_window", VC.K8, [(v, f), (v, f)], [nrm_for(v), nrm_for(v)], [(8, 8, 30, 30), VC.FULL], [(4, 8, 20, 20), VC.FULL], scene=[0, 1])
    add("scene_outside_the_table", VC.K8, [(v, f), (v, f)], [nrm_for(v), nrm_for(v)], [VC.FULL, VC.FULL], [VC.FULL, (5, 5, 30, 30)], scene=[3, 0], S=1)
    return out


def sphere_batch(R=24):
    """the marching-tetrahedra sphere of tests/_mesh_ref.py, radius r = 0.6 lattice units, with the exact vertex normals
    v / |v|, posed at z = 10 r scale in front of the camera, ks = 0: (batch, centre, radius in camera units)"""
    from tests import _mesh_ref as MR
    v0, f0, _ = MR.extract(MR.shape_sdf("sphere", R))
    v0 = np.asarray(v0, np.float64)
    r = 0.6                                                                # shape_sdf's sphere
    scale = 1.5
    centre = np.array([0.2, -0.1, 10.0 * r * scale])
    vc, fc = VC.to_camera(v0, f0, scale, 0.0, tuple(centre / scale))
    vc = np.asarray(vc, np.float32)
    n = vc.astype(np.float64) - centre
    n = (n / np.linalg.norm(n, axis=1)[:, None]).astype(np.float32)
    K = (200.0, 200.0, 31.5, 23.7)                                         # the sphere is 40 pixels across
    b = dict(K=K, size=(W, H), meshes=[(vc, fc)], normals=[n], windows=[VC.FULL], boxes=[VC.FULL], scene=None,
             paint=np.array([[1.0, 1.0, 1.0, 0.0, 0]], np.float64), light=np.array([light_row(0.4, -0.5, -0.75, 0.15, 0.8)], np.float64),
             ramp=np.zeros((1, 8), np.int32), bg_index=None, bgs=None, triangles=None)
    return b, centre, r * scale
