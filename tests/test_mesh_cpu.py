"""Mesh extraction without a GPU: the invariants of the numpy restatement (tests/_mesh_ref.py), the per-point header csrc/mesh_cells.h
compiled for the host and compared with the restatement bit for bit, and the host side of sdflabel_amd.mesh (files, camera frame)."""
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import _mesh_ref as MR
from tests._util import build_host_program

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPHERE_VOLUME = 4.0 / 3.0 * np.pi * 0.6 ** 3


@pytest.mark.parametrize("R", [9, 13])
@pytest.mark.parametrize("name,chi", [("sphere", 2), ("ellipsoid", 2), ("torus", 0)])
def test_restatement_is_closed_oriented_and_has_the_right_genus(name, chi, R):
    v, f, aux = MR.extract(MR.shape_sdf(name, R))
    assert len(f) > 0 and int(aux["tcount"].sum()) == len(f) and int(sum(bin(m).count("1") for m in aux["mask"])) == len(v)
    assert (MR.undirected_edge_counts(f) == 2).all()
    assert MR.directed_edges_paired(f)
    assert MR.euler_characteristic(f) == chi
    assert MR.signed_volume(v, f) > 0
    assert (MR.triangle_areas(v, f) > 0).all()


def test_restatement_exact_zeros_give_degenerate_triangles_and_stay_closed():
    sdf = MR.shape_sdf("octahedron", 9)
    assert (sdf == 0).sum() > 0
    v, f, _ = MR.extract(sdf)
    n0 = int((MR.triangle_areas(v, f) == 0).sum())
    print("octahedron R = 9: %d triangles, %d of zero area" % (len(f), n0))
    assert n0 > 0
    assert MR.is_closed(f) and MR.directed_edges_paired(f) and MR.euler_characteristic(f) == 2
    assert abs(MR.signed_volume(v, f) - 4.0 / 3.0 * 0.5 ** 3) < 1e-6


def test_restatement_open_surface_and_nan():
    v, f, _ = MR.extract(MR.shape_sdf("cut_sphere", 9))
    cnt = MR.undirected_edge_counts(f)
    assert cnt.max() == 2 and cnt.min() == 1                    # open where it leaves the cube, never more than two triangles on an edge
    sdf = MR.shape_sdf("sphere", 9)
    sdf[4, 4, :] = np.nan
    v, f, _ = MR.extract(sdf)
    assert np.isfinite(v).all() and len(f) > 0


def test_sphere_volume_converges_monotonically():
    vols = []
    for R in (9, 13, 25, 41):
        v, f, _ = MR.extract(MR.shape_sdf("sphere", R))
        vols.append(MR.signed_volume(v, f))
    err = [abs(x - SPHERE_VOLUME) for x in vols]
    print("sphere volumes", vols, "exact", SPHERE_VOLUME)
    assert all(a > b for a, b in zip(err, err[1:]))
    assert err[-1] < 0.005 * SPHERE_VOLUME


# ---- the header on the host ----------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    return build_host_program(tmp_path_factory.mktemp("mesh_host"), "mesh_host/mesh_host.cpp", "mesh_host")


def run_host(exe, sdf, tmp):
    R = sdf.shape[0]
    src, dst = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(src, "wb") as fh:
        fh.write(np.int32(R).tobytes() + np.ascontiguousarray(sdf, np.float32).tobytes())
    r = subprocess.run([exe, src, dst], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    raw = open(dst, "rb").read()
    nv, nt = np.frombuffer(raw, np.int32, 2)
    o = 8
    v = np.frombuffer(raw, np.float32, 3 * nv, o).reshape(nv, 3); o += 12 * nv
    f = np.frombuffer(raw, np.int32, 3 * nt, o).reshape(nt, 3); o += 12 * nt
    mask = np.frombuffer(raw, np.uint8, R ** 3, o); o += R ** 3
    tc = np.frombuffer(raw, np.uint8, R ** 3, o)
    return v, f, mask, tc


def _cases():
    rng = np.random.default_rng(5)
    yield "sphere9", MR.shape_sdf("sphere", 9)
    yield "torus13", MR.shape_sdf("torus", 13)
    yield "octahedron9", MR.shape_sdf("octahedron", 9)
    yield "cut9", MR.shape_sdf("cut_sphere", 9)
    yield "noise7", rng.standard_normal((7, 7, 7)).astype(np.float32)             # every case of every tetrahedron, many times
    yield "single_cell", np.array([-1, 1, 1, -1, 1, -1, 0, 1], np.float32).reshape(2, 2, 2)
    s = MR.shape_sdf("sphere", 9)
    s[3, :, 5] = np.nan
    s[0, 0, 0] = -np.inf
    yield "nan9", s
    yield "all_inside5", -np.ones((5, 5, 5), np.float32)                            # nothing: the boundary is not capped
    yield "sphere21",MR.shape_sdf("sphere", 21)                                    # 37 blocks of 256 points


@pytest.mark.parametrize("name", [n for n, _ in _cases()])
def test_header_on_the_host_reproduces_the_restatement(host_program, tmp_path, name):
    sdf = dict(_cases())[name]
    v, f, mask, tc = run_host(host_program, sdf, str(tmp_path))
    rv, rf, aux = MR.extract(sdf)
    assert np.array_equal(mask, aux["mask"]) and np.array_equal(tc, aux["tcount"])
    assert f.shape == rf.shape and np.array_equal(f, rf)
    assert v.shape == rv.shape and v.tobytes() == rv.tobytes()
    assert np.isfinite(v).all()


# ---- sdflabel_amd.mesh on the host -----------------------------------------------------------------------------------------------------------

def _host_mesh(name="ellipsoid", R=13, normals=True):
    from sdflabel_amd.mesh import Mesh
    v, f, _ = MR.extract(MR.shape_sdf(name, R))
    n = None
    if normals:                                        # the ellipsoid's analytic outward normals
        g = v.astype(np.float64) / np.array([0.8, 0.45, 0.6]) ** 2
        n = (g / np.linalg.norm(g, axis=1, keepdims=True)).astype(np.float32)
    return Mesh(torch.from_numpy(v), torch.from_numpy(f), None if n is None else torch.from_numpy(n))


@pytest.mark.parametrize("normals", [True, False])
def test_ply_round_trip(tmp_path, normals):
    from sdflabel_amd.mesh import load_ply
    m = _host_mesh(normals=normals)
    p = str(tmp_path / "m.ply")
    m.save(p)
    v, n, f = load_ply(p)
    assert v.tobytes() == m.vertices_numpy().tobytes() and np.array_equal(f, m.faces_numpy())
    assert (n is None) == (not normals) and (n is None or n.tobytes() == m.normals_numpy().tobytes())
    head = open(p, "rb").read(64)
    assert head.startswith(b"ply\nformat binary_little_endian 1.0\n")


def test_obj_round_trip(tmp_path):
    m = _host_mesh()
    p = str(tmp_path / "m.obj")
    m.save(p)
    v, n, f = [], [], []
    for ln in open(p):
        w = ln.split()
        if w[:1] == ["v"]:
            v.append([float(x) for x in w[1:]])
        elif w[:1] == ["vn"]:
            n.append([float(x) for x in w[1:]])
        elif w[:1] == ["f"]:
            f.append([int(x.split("/")[0]) - 1 for x in w[1:]])
            assert all(x.split("/")[0] == x.split("/")[2] for x in w[1:])
    assert np.array_equal(np.asarray(v, np.float32), m.vertices_numpy()) and np.array_equal(np.asarray(n, np.float32), m.normals_numpy())
    assert np.array_equal(np.asarray(f, np.int32), m.faces_numpy())
    with pytest.raises(ValueError):
        m.save(str(tmp_path / "m.stl"))


def test_drop_degenerate_is_a_host_side_option(tmp_path):
    from sdflabel_amd.mesh import load_ply
    m = _host_mesh("octahedron", 9, normals=False)
    assert m.is_closed()
    kept = m.faces_numpy(drop_degenerate=True)
    assert 0 < len(kept) < len(m.faces_numpy()) == len(m)
    m.save(str(tmp_path / "d.ply"), drop_degenerate=True)
    assert len(load_ply(str(tmp_path / "d.ply"))[2]) == len(kept)


def test_to_camera_keeps_positive_volume_and_outward_normals():
    from sdflabel_amd.frame import assemble_labels
    m = _host_mesh()
    assert m.is_closed() and m.volume() > 0
    assert abs(m.volume() - MR.signed_volume(m.vertices_numpy(), m.faces_numpy())) < 1e-12
    with pytest.raises(ValueError):
        m.to_camera()
    scale = 1.7
    _, cam_T = assemble_labels(np.zeros((1, 6), np.float32), np.array([0.7], np.float32), np.array([[0.4, -0.2, 5.0]], np.float32),
                               np.array([scale], np.float32), np.eye(4), [None])
    assert np.linalg.det(cam_T[0][:3, :3]) < 0                                  # the matrix holds diag(1, -1, 1): a reflection
    m.scale, m.cam_T = scale, cam_T[0]
    c = m.to_camera()
    assert c.frame == "camera" and c.to_camera() is c and c.is_closed()
    assert abs(c.volume() - scale ** 3 * m.volume()) < 1e-4 * c.volume() and c.volume() > 0
    assert abs(c.area() - scale ** 2 * m.area()) < 1e-4 * c.area()
    # the geometric normal of every triangle agrees with the transformed vertex normals: outward in the camera frame too
    v, f, n = c.vertices_numpy().astype(np.float64), c.faces_numpy(), c.normals_numpy().astype(np.float64)
    g = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    assert (np.einsum("ij,ij->i", g, n[f].mean(1)) > 0).all()
    centre = v.mean(0)
    assert (np.einsum("ij,ij->i", n, v - centre) > 0).all()
    want = (m.vertices_numpy().astype(np.float64) * scale) @ cam_T[0][:3, :3].T + cam_T[0][:3, 3]
    assert np.abs(v - want).max() < 1e-5
