"""Verification without a GPU: the numpy restatement (tests/_verify_ref.py) against analytic silhouettes, the header csrc/verify_cells.h
compiled for the host and compared with the restatement bit for bit (once more under the address and undefined-behaviour sanitizers), and
the agreement of header, ctypes table and library on the new exports."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import _verify_cases as VC
from tests import _verify_ref as VR
from tests._util import build_host_program

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cases():
    return VC.cases()


@pytest.fixture(scope="module")
def refs(cases):
    """name -> (mask, depth, triangle, flags) of the restatement; computed once, never modified"""
    return {n: VR.raster(v, f, K, w, z) for n, (v, f, K, w, z) in cases.items()}


# ---- the restatement against what can be said without it -------------------------------------------------------------------------------------

def test_cube_equals_the_analytic_silhouette_and_the_front_faces_depth(refs):
    mask, depth, tri, flags = refs["cube"]
    ys, xs = np.mgrid[0:VC.H, 0:VC.W]
    want = (xs >= 16) & (xs <= 48) & (ys >= 8) & (ys <= 40)             # the front face's projection, borders included
    assert flags == 0 and np.array_equal(mask != 0, want)
    assert (depth[want] == np.float32(2.0)).all() and (depth[~want] == 0).all()
    assert np.isin(tri[want], (0, 1)).all() and (tri[~want] == -1).all()       # the front face wins the exact ties on its border


def test_inclusive_edges_pass_through_sample_points(refs):
    mask, depth, tri, _ = refs["edges_through_samples"]
    ys, xs = np.mgrid[0:VC.H, 0:VC.W]
    want = (xs >= 10) & (ys >= 10) & (xs + ys <= 30)                     # 66 lattice points, the three borders included
    assert np.array_equal(mask != 0, want) and int(mask.sum()) == 66
    assert mask[15, 15] == 1 and mask[10, 20] == 1 and mask[20, 10] == 1 and mask[16, 15] == 0
    assert (depth[want] == 1).all()
    m2 = refs["edges_through_samples_z2"][0]                            # the other winding, Z = 2
    u = np.array([30.0, 50, 40]); v = np.array([5.0, 15, 35])
    e = [(u[a] - xs) * (v[b] - ys) - (v[a] - ys) * (u[b] - xs) for a, b in ((1, 2), (2, 0), (0, 1))]
    s = np.sign((u[1] - u[0]) * (v[2] - v[0]) - (v[1] - v[0]) * (u[2] - u[0]))
    assert np.array_equal(m2 != 0, (e[0] * s >= 0) & (e[1] * s >= 0) & (e[2] * s >= 0))      # integer arithmetic in float64: exact
    assert m2[10, 40] == 1 and m2[20, 45] == 1                          # on the edges (30,5)-(50,15) and (50,15)-(40,35)


def test_shared_edges_ties_and_occlusion(refs):
    mask, depth, tri, _ = refs["shared_edge"]
    ys, xs = np.mgrid[0:VC.H, 0:VC.W]
    sq = (xs >= 10) & (xs <= 20) & (ys >= 10) & (ys <= 20)
    assert np.array_equal(mask != 0, sq)                                 # no gap along the diagonal
    assert (tri[sq & (xs >= ys)] == 0).all() and (tri[sq & (xs < ys)] == 1).all()       # the diagonal itself goes to the lower index
    mask, depth, tri, _ = refs["coplanar_overlap"]
    a = VR.raster(*_only(VC.cases()["coplanar_overlap"], 0))[0] != 0
    b = VR.raster(*_only(VC.cases()["coplanar_overlap"], 1))[0] != 0
    assert (a & b).sum() > 50 and np.array_equal(mask != 0, a | b)
    assert (tri[a] == 0).all() and (tri[b & ~a] == 1).all() and (depth[a | b] == 2).all()
    mask, depth, tri, _ = refs["near_over_far"]
    near = VR.raster(*_only(VC.cases()["near_over_far"], 1))[0] != 0
    assert near.sum() > 100 and (tri[near] == 1).all() and (depth[near] == 1).all() and (depth[(mask != 0) & ~near] == 2).all()


def _only(case, i):
    v, f, K, w, z = case
    return v, f[i:i + 1], K, w, z


def test_windows_skips_and_flags(refs, cases):
    full = VR.raster(cases["partly_outside_window"][0], cases["partly_outside_window"][1], VC.K8, VC.FULL)[0]
    l, t, r, b = cases["partly_outside_window"][3]
    assert np.array_equal(refs["partly_outside_window"][0], full[t:b, l:r]) and 0 < refs["partly_outside_window"][0].sum() < full.sum()
    assert refs["partly_outside_image"][0].sum() > 0
    one = refs["edges_through_samples"]
    for name, fl, idx in (("zero_area", 0, 1), ("behind_z_min", VR.FLAG_BEHIND, 1), ("bad_index", VR.FLAG_INVALID, 1)):
        m, d, tr, flags = refs[name]
        assert flags == fl and np.array_equal(m, one[0]) and d.tobytes() == one[1].tobytes() and (tr[m != 0] == idx).all(), name
    m, d, tr, flags = refs["nan_vertex"]
    assert flags == 0 and np.isin(tr, (1, 3, 4)).all() and np.isfinite(d).all()
    assert refs["empty_mesh"][0].shape == (15, 15) and refs["empty_mesh"][0].sum() == 0 and (refs["empty_mesh"][2] == -1).all()
    assert refs["empty_window"][0].shape == (10, 0)
    assert refs["full_window"][0].shape == (32, 48) and refs["full_window"][0].all() and (refs["full_window"][2] == 0).all()
    m, d, tr, _ = refs["sphere24"]
    print("sphere24: %d triangles, %d pixels covered, %d distinct winners" % (len(cases["sphere24"][1]), int(m.sum()), len(np.unique(tr[m != 0]))))
    assert 2000 <= len(cases["sphere24"][1]) <= 6000 and m.sum() > 500 and len(np.unique(tr[m != 0])) > 200


def test_mask_counts_and_point_frame_of_the_restatement(refs, cases):
    m = refs["edges_through_samples"][0]
    lab = np.zeros_like(m)
    lab[12:30, 8:16] = 1
    c = VR.mask_counts(m, VC.FULL, lab)
    assert c.tolist() == [66, 10, 10, 21, 21, 18 * 8, int((m[12:30, 8:16]).sum()), 0]
    assert VR.mask_counts(refs["empty_mesh"][0], cases["empty_mesh"][3]).tolist() == [0] * 8
    # the lattice frame is the inverse of the camera frame of the label
    rng = np.random.default_rng(2)
    x = rng.uniform(-1, 1, (200, 3)).astype(np.float32)
    scale, yaw, trans = 1.7, 0.7, (0.4, -0.2, 3.0)
    cam, _ = VC.to_camera(x, np.zeros((0, 3), np.int32), scale, yaw, trans)
    pose = VR.pose_row(np.cos(np.float32(yaw)), np.sin(np.float32(yaw)), trans, scale)
    back, inside = VR.point_x(cam, pose)
    bound = VR.roundtrip_bound(scale, trans)
    print("camera -> lattice round trip: max error %.3g, bound %.3g" % (np.abs(back - x).max(), bound))
    assert np.abs(back.astype(np.float64) - x).max() < bound and inside.sum() >= 195


# ---- the header on the host --------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    return build_host_program(tmp_path_factory.mktemp("verify_host"), "verify_host/verify_host.cpp", "verify_host")


def run_host(exe, names, cases, K, pp, tmp):
    """the cases `names` (all with intrinsics K) as one ragged batch plus the point problem -> what the host program wrote"""
    B = len(names)
    vs, fs, wins = [cases[n][0] for n in names], [cases[n][1] for n in names], np.asarray([cases[n][3] for n in names], np.int32)
    voff = np.concatenate([[0], np.cumsum([len(v) for v in vs])]).astype(np.int64)
    toff = np.concatenate([[0], np.cumsum([len(f) for f in fs])]).astype(np.int64)
    points, ptoff, poses, lat, sdf, band = pp
    NA, L = lat.shape
    src, dst = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(src, "wb") as fh:
        fh.write(np.array([B, VC.W, VC.H, NA, L], np.int32).tobytes() + np.array([0.1, band], np.float32).tobytes() + np.asarray(K, np.float64).tobytes())
        for a in (voff, toff, wins, ptoff, np.concatenate(vs).astype(np.float32), np.concatenate(fs).astype(np.int32), poses, lat, points, sdf):
            fh.write(np.ascontiguousarray(a).tobytes())
    r = subprocess.run([exe, src, dst], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    raw = open(dst, "rb").read()
    P = int(((wins[:, 2] - wins[:, 0]) * (wins[:, 3] - wins[:, 1])).sum())
    N = int(ptoff[-1])
    o = 0
    out = []
    for dt, n in ((np.uint8, P), (np.float32, P), (np.int32, P), (np.int32, B), (np.int32, 8 * B), (np.float32, N * (L + 3)), (np.uint8, N),
                  (np.int32, 3 * NA)):
        out.append(np.frombuffer(raw, dt, n, o))
        o += n * np.dtype(dt).itemsize
    assert o == len(raw)
    return out, wins


def check_host(out, wins, names, refs, pp):
    mask, depth, tri, flags, counts, rows, in_cube, band = out
    o = 0
    for b, n in enumerate(names):
        rm, rd, rt, rf = refs[n]
        k = rm.size
        assert mask[o:o + k].tobytes() == rm.tobytes() and depth[o:o + k].tobytes() == rd.tobytes() and tri[o:o + k].tobytes() == rt.tobytes(), n
        assert flags[b] == rf, n
        assert counts[8 * b:8 * b + 8].tolist() == VR.mask_counts(rm, wins[b]).tolist(), n
        o += k
    points, ptoff, poses, lat, sdf, bandw = pp
    rrows, rin = VR.point_rows(points, ptoff, poses, lat)
    assert rows.tobytes() == rrows.tobytes() and in_cube.tobytes() == rin.tobytes()
    assert 0 < rin.sum() < len(rin)
    want = VR.band_counts(sdf, rin, ptoff, poses, bandw)
    assert band.reshape(-1, 3).tolist() == want.tolist() and 0 < want[0, 2] < want[0, 1] < want[0, 0]


def k8_names(cases):
    return [n for n, c in cases.items() if c[2] == VC.K8]


def test_header_on_the_host_reproduces_the_restatement(host_program, tmp_path, cases, refs):
    pp = VC.point_problem()
    names = k8_names(cases)
    out, wins = run_host(host_program, names, cases, VC.K8, pp, str(tmp_path))
    check_host(out, wins, names, refs, pp)
    for name, K in (("cube", VC.K_CUBE), ("sphere24", VC.K_SPHERE)):
        out, wins = run_host(host_program, [name, "empty_mesh"], cases, K, pp, str(tmp_path))
        check_host(out, wins, [name, "empty_mesh"], refs, pp)


def test_header_on_the_host_under_the_sanitizers(tmp_path, cases, refs):
    """exact-size buffers: an index outside a window, a mesh or a cloud is an error here"""
    exe = build_host_program(tmp_path, "verify_host/verify_host.cpp", "verify_host_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    pp = VC.point_problem()
    names = k8_names(cases)
    out, wins = run_host(exe, names, cases, VC.K8, pp, str(tmp_path))
    check_host(out, wins, names, refs, pp)
    # the cases in which only the predicates the kernels share (verify_face_ok, verify_window_ok) keep the reads inside the buffers
    flags = dict(zip(names, out[3].tolist()))
    assert flags["bad_index"] == VR.FLAG_INVALID and flags["behind_z_min"] == VR.FLAG_BEHIND and flags["empty_mesh"] == flags["empty_window"] == 0
    v, f = cases["edges_through_samples"][:2]
    broken = dict(cases, window_outside_image=(v, f, VC.K8, (60, 40, 70, 50), 0.1))
    names = ["edges_through_samples", "window_outside_image", "bad_index"]
    (mask, _, tri, flags, counts, _, _, _), wins = run_host(exe, names, broken, VC.K8, pp, str(tmp_path))
    n0 = refs["edges_through_samples"][0].size
    assert mask[:n0].tobytes() == refs["edges_through_samples"][0].tobytes() and mask[n0 + 100:].tobytes() == refs["bad_index"][0].tobytes()
    assert not mask[n0:n0 + 100].any() and (tri[n0:n0 + 100] == -1).all()
    assert flags.tolist() == [0, VR.FLAG_INVALID, VR.FLAG_INVALID] and counts[8:16].tolist() == [0] * 7 + [VR.FLAG_INVALID]


# ---- header, ctypes table, library -------------------------------------------------------------------------------------------------------------

def test_abi_has_the_verification_entry_points():
    from sdflabel_amd import _lib
    header = open(os.path.join(ROOT, "include", "sdfr.h")).read()
    h = _lib.lib()
    for name in ("sdfr_mesh_raster", "sdfr_verify_mask_counts", "sdfr_verify_point_rows", "sdfr_verify_band_counts"):
        assert name in _lib.EXPORTS and hasattr(h, name) and re.search(r"\bint %s\(" % name, header), name
    assert int(re.search(r"#define SDFR_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION == h.sdfr_version() >= 412


def test_argument_checks_come_before_any_launch():
    import ctypes
    from sdflabel_amd import _lib
    h = _lib.lib()
    k = (ctypes.c_double * 4)(8, 8, 32, 24)
    assert h.sdfr_mesh_raster(None, 0, None, 0, None, None, None, None, 0, 1, 64, 48, k, 0.1, None, None, None, None, None, None) == -1
    assert b"NULL" in h.sdfr_last_error()
    assert h.sdfr_mesh_raster(None, 0, None, 0, None, None, None, None, 0, 0, 64, 48, k, 0.1, None, None, None, None, None, None) == 0
    assert h.sdfr_mesh_raster(None, 0, None, 0, None, None, None, None, 0, 1, 64, 48, None, 0.1, None, None, None, None, None, None) == -1
    assert h.sdfr_mesh_raster(None, 0, None, 0, None, None, None, None, 64 * 48 + 1, 1, 64, 48, k, 0.1, None, None, None, None, None, None) == -1
    assert h.sdfr_mesh_raster(None, 0, None, 0, None, None, None, None, 0, 1, 64, 48, k, -1.0, None, None, None, None, None, None) == -1
    assert h.sdfr_verify_mask_counts(None, None, None, None, 0, 2, 64, 48, None, None) == -1
    assert h.sdfr_verify_point_rows(None, 10, None, 1, None, None, 3, 5, 6, None, None, None) == -1 and b"outside" in h.sdfr_last_error()
    assert h.sdfr_verify_point_rows(None, 10, None, 1, None, None, 3, 0, 10, None, None, None) == -1 and b"NULL" in h.sdfr_last_error()
    assert h.sdfr_verify_band_counts(None, None, 10, None, 1, None, 0.2, None, None) == -1
    assert h.sdfr_verify_band_counts(None, None, 0, None, 0, None, 0.2, None, None) == 0


def test_python_side_without_a_gpu():
    import torch
    from sdflabel_amd import verify as V
    from sdflabel_amd.mesh import Mesh
    box, win = V.label_windows([[10.2, 5, 30, 20.5], [0, 0, 64, 48]], (64, 48), 0.25)
    assert box.tolist() == [[10, 5, 30, 21], [0, 0, 64, 48]] and win.tolist() == [[5, 1, 35, 25], [0, 0, 64, 48]]
    assert V._box_iou([0, 0, 10, 10], [5, 0, 15, 10]) == 50.0 / 150.0 and V._box_iou([0, 0, 0, 0], [0, 0, 0, 0]) == 0.0
    m = Mesh(torch.zeros((3, 3)), torch.zeros((1, 3), dtype=torch.int32))
    with pytest.raises(ValueError):
        V.raster_many([m], VC.K8, [VC.FULL], (VC.W, VC.H))                 # a lattice-frame mesh
    m.frame = "camera"
    with pytest.raises(V._lib.SdfrError):
        V.raster_many([m], VC.K8, [VC.FULL], (VC.W, VC.H))                 # no CPU fallback
