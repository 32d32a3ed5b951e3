"""The rasteriser's test meshes, shared by tests/test_verify_cpu.py (restatement and host build of the header) and tests/test_gpu_verify.py
(the kernels).  Image 64 x 48.  With fx = fy = 8, integer cx, cy, Z = 1 or 2 and X, Y multiples of 1/8 (1/4 at Z = 2) every projection is
an exact integer, so edges pass exactly through sample points."""
import numpy as np

from tests._verify_ref import pose_row

W, H = 64, 48
K8 = (8.0, 8.0, 32.0, 24.0)
K_SPHERE = (100.0, 100.0, 31.5, 23.7)
FULL = (0, 0, W, H)


def at(uvz, K=K8):
    """camera-frame float32 vertices projecting to (u, v) at depth z"""
    uvz = np.asarray(uvz, np.float64).reshape(-1, 3)
    X = (uvz[:, 0] - K[2]) / K[0] * uvz[:, 2]
    Y = (uvz[:, 1] - K[3]) / K[1] * uvz[:, 2]
    out = np.stack([X, Y, uvz[:, 2]], 1).astype(np.float32)
    assert np.array_equal(out.astype(np.float64), np.stack([X, Y, uvz[:, 2]], 1))           # exactly representable
    return out


def faces(*f):
    return np.asarray(f, np.int32).reshape(-1, 3)


def cube_mesh():
    """a cube with its front face at Z = 2 and its back face at Z = 4, for fx = fy = 32: the front face projects to [16, 48] x [8, 40]"""
    v = np.array([[x, y, z] for z in (2.0, 4.0) for y in (-1.0, 1.0) for x in (-1.0, 1.0)], np.float32)
    f = faces((0, 1, 3), (0, 3, 2),                         # front (first: it wins exact ties on its border)
              (4, 7, 5), (4, 6, 7), (0, 4, 5), (0, 5, 1), (2, 3, 7), (2, 7, 6), (0, 2, 6), (0, 6, 4), (1, 5, 7), (1, 7, 3))
    return v, f


K_CUBE = (32.0, 32.0, 32.0, 24.0)


def sphere_mesh():
    """the marching-tetrahedra mesh of the analytic sphere at R = 24 (tests/_mesh_ref.py) in the camera frame: a few thousand triangles of a
    few pixels each"""
    from tests import _mesh_ref as MR
    v, f, _ = MR.extract(MR.shape_sdf("sphere", 24))
    return to_camera(v, f, 1.7, 0.7, (0.05, -0.02, 3.0))


def to_camera(v, f, scale, yaw, trans):
    import torch
    from sdflabel_amd.frame import assemble_labels
    from sdflabel_amd.mesh import Mesh
    _, cam_T = assemble_labels(np.zeros((1, 6), np.float32), np.array([yaw], np.float32), np.array([trans], np.float32),
                               np.array([scale], np.float32), np.eye(4), [None])
    m = Mesh(torch.from_numpy(np.ascontiguousarray(v, np.float32)), torch.from_numpy(np.ascontiguousarray(f, np.int32)), scale=scale,
             cam_T=cam_T[0]).to_camera()
    return m.vertices_numpy(), m.faces_numpy()


def cases():
    """name -> (vertices float32 [V][3], faces int32 [T][3], K, window, z_min)"""
    nan = np.float32(np.nan)
    one = at([(10, 10, 1), (20, 10, 1), (10, 20, 1)])
    c = {}
    c["edges_through_samples"] = (one, faces((0, 1, 2)), K8, FULL, 0.1)
    c["edges_through_samples_z2"] = (at([(30, 5, 2), (50, 15, 2), (40, 35, 2)]), faces((0, 2, 1)), K8, FULL, 0.1)
    c["shared_edge"] = (at([(10, 10, 1), (20, 10, 1), (20, 20, 1), (10, 20, 1)]), faces((0, 1, 2), (0, 2, 3)), K8, FULL, 0.1)
    c["coplanar_overlap"] = (at([(10, 10, 2), (30, 10, 2), (10, 30, 2), (14, 12, 2), (34, 14, 2), (16, 32, 2)]), faces((3, 4, 5), (0, 1, 2)), K8,
                             FULL, 0.1)
    c["near_over_far"] = (at([(4, 4, 2), (60, 6, 2), (8, 44, 2), (20, 10, 1), (40, 12, 1), (24, 30, 1)]), faces((0, 1, 2), (3, 4, 5)), K8, FULL, 0.1)
    c["partly_outside_window"] = (at([(10, 10, 1), (50, 14, 1), (20, 40, 1)]), faces((0, 1, 2)), K8, (12, 12, 30, 31), 0.1)
    c["partly_outside_image"] = (at([(-10, -5, 1), (40, 10, 1), (5, 60, 1)]), faces((0, 1, 2)), K8, FULL, 0.1)
    c["zero_area"] = (np.concatenate([at([(10, 10, 1), (20, 20, 1), (30, 30, 1)]), one]), faces((0, 1, 2), (3, 4, 5), (3, 3, 4)), K8, FULL, 0.1)
    behind = np.concatenate([one, np.array([[0.5, 0.5, 0.05], [1.0, 0.0, 1.0], [0.0, 1.0, 1.0], [0.0, 0.0, 0.1]], np.float32)])
    c["behind_z_min"] = (behind, faces((3, 4, 5), (0, 1, 2), (6, 4, 5)), K8, FULL, 0.1)
    wild = np.concatenate([one, np.array([[nan, 0, 1], [1, 0, 1], [0, 1, 1], [np.inf, 0, 1], [3e38, -3e38, 0.2], [-3e38, 3e38, 0.2],
                                          [3e38, 3e38, 0.2]], np.float32)])
    c["nan_vertex"] = (wild, faces((3, 4, 5), (0, 1, 2), (6, 4, 5), (7, 8, 9), (7, 1, 2)), K8, FULL, 0.1)
    c["bad_index"] = (one, faces((0, 1, 3), (0, 1, 2), (-1, 1, 2)), K8, FULL, 0.1)
    c["empty_mesh"] = (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), K8, (5, 5, 20, 20), 0.1)
    c["empty_window"] = (one, faces((0, 1, 2)), K8, (10, 10, 10, 20), 0.1)
    c["full_window"] = (at([(-100, -100, 1), (300, -100, 1), (-100, 300, 1)]), faces((0, 1, 2)), K8, (8, 8, 56, 40), 0.1)
    cv, cf = cube_mesh()
    c["cube"] = (cv, cf, K_CUBE, FULL, 0.1)
    sv, sf = sphere_mesh()
    c["sphere24"] = (sv, sf, K_SPHERE, (3, 1, 62, 47), 0.1)
    return c


def point_problem(seed=4, n=(300, 0, 150), L=3):
    """a ragged batch of camera-frame points with poses, latents and stand-in decoder values (some NaN, some outside the cube)"""
    rng = np.random.default_rng(seed)
    ptoff = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    poses = [pose_row(np.cos(np.float32(y)), np.sin(np.float32(y)), t, s) for y, t, s in
             ((0.7, (0.4, -0.2, 3.0), 1.7), (-2.0, (0.0, 0.0, 5.0), 2.0), (3.0, (-1.0, 0.3, 4.0), 0.9))]
    pts = []
    for b in range(len(n)):
        c = np.asarray(poses[b][2:5], np.float64) * float(poses[b][5])
        pts.append((c + rng.uniform(-1.3, 1.3, (n[b], 3)) * float(poses[b][5])).astype(np.float32))
    points = np.concatenate(pts)
    points[5] = np.nan
    points[7, 1] = np.inf
    lat = rng.standard_normal((len(n), L)).astype(np.float32)
    sdf = rng.uniform(-0.3, 0.3, ptoff[-1]).astype(np.float32)
    sdf[11] = np.nan
    return points, ptoff, np.stack(poses), lat, sdf, np.float32(0.2)
