"""Signed distances to meshes without a GPU: the numpy restatement (tests/_mesh_sdf_ref.py) against analysis, the header
csrc/mesh_sdf_cells.h compiled for the host and compared with the restatement bit for bit (once more under the address and
undefined-behaviour sanitizers, as a stand-alone program), and the agreement of header, ctypes table and library on the new exports.
Every figure is printed before it is asserted."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import _mesh_ref as MR
from tests import _mesh_sdf_cases as C
from tests import _mesh_sdf_ref as SR
from tests._mesh_sdf_cases import check_against, check_surface, lattice_bound, winding_bound
from tests._util import build_host_program

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cases():
    return C.cases()


@pytest.fixture(scope="module")
def refs():
    return C.references()


# ---- the restatement against analysis ------------------------------------------------------------------------------------------------------------

def test_icosphere_distance_stays_within_the_sag_of_the_largest_triangle(cases, refs):
    v, f, p, _ = cases["icosphere"]
    a, b, c = (v[f[:, k]].astype(np.float64) for k in range(3))
    la, lb, lc = np.linalg.norm(b - c, axis=1), np.linalg.norm(c - a, axis=1), np.linalg.norm(a - b, axis=1)
    area = 0.5 * np.linalg.norm(np.cross(b - a, c - a), axis=1)
    rc = (la * lb * lc / (4.0 * area)).max()                               # the largest circumradius
    sag = C.RADIUS - (C.RADIUS ** 2 - rc ** 2) ** 0.5
    r = np.linalg.norm(p.astype(np.float64), axis=1)
    err = np.abs(refs["icosphere"]["dist"] - np.abs(r - C.RADIUS)).max()
    print("icosphere: circumradius %.4f, sag %.3e, max | dist - | |p| - r | | = %.3e" % (rc, sag, err))
    assert err <= sag + 1e-6                                               # 1e-6: the vertices and dist are float32
    far = np.abs(r - C.RADIUS) > sag + 1e-6
    assert far.sum() > 1900 and np.array_equal(refs["icosphere"]["sdf"][far] < 0, r[far] < C.RADIUS)
    # the reversed winding gives w = -1 inside and the same signs
    rr = np.linalg.norm(cases["reversed"][2].astype(np.float64), axis=1)
    far = np.abs(rr - C.RADIUS) > sag + 1e-6
    assert np.array_equal(refs["reversed"]["sdf"][far] < 0, rr[far] < C.RADIUS) and refs["reversed"]["winding"].min() < -0.99


def test_lattice_sphere_stays_within_the_derived_bound(cases, refs):
    e, h = lattice_bound()
    p = cases["lattice_sphere"][2].astype(np.float64)
    r = np.linalg.norm(p, axis=1)
    ref = refs["lattice_sphere"]
    err = np.abs(ref["dist"] - np.abs(r - 0.6)).max()
    print("lattice sphere R = 16: h = %.4f, e = %.4f = %.2f h^2, max error %.4f = %.2f h^2" % (h, e, e / h ** 2, err, err / h ** 2))
    assert err <= e + 1e-6
    far = np.abs(r - 0.6) > e + 1e-6
    assert far.sum() > 300 and np.array_equal(ref["sdf"][far] < 0, r[far] < 0.6)


def test_winding_numbers_of_closed_meshes_are_integers_within_rounding(cases, refs):
    for n in C.CLOSED:
        w, T = refs[n]["winding"], len(cases[n][1])
        dev = np.abs(w - np.round(w))
        bound = winding_bound(refs[n], T)
        print("%-16s T = %5d: max | w - round(w) | = %.2e, smallest bound %.2e" % (n, T, dev.max(), bound.min()))
        f = cases[n][1]
        assert MR.is_closed(np.concatenate([f[:40], f[48:]]) if n == "broken" else f), n       # (the broken mesh: its usable triangles)
        assert (dev <= bound).all() and np.isin(np.round(w), (-1, 0, 1)).all(), n
        assert (np.round(w) != 0).any() and (np.round(w) == 0).any(), n


def test_margin_condition_no_point_is_near_the_sign_threshold(cases, refs):
    """what lets every comparison below demand equal signs from libraries whose atan2 differs in the last bits"""
    for n, r in refs.items():
        if len(r["winding"]) == 0:
            continue
        m = np.abs(np.abs(r["winding"]) - 0.5).min()
        print("%-18s min | |w| - 0.5 | = %.4f" % (n, m))
        assert m > 1e-6, n
    assert refs["cube_ties"]["winding"].tolist() == [0.0] * len(cases["cube_ties"][2])      # unsigned: no winding pass at all


def test_cube_ties_go_to_the_lowest_index(cases, refs):
    v, f, p, _ = cases["cube_ties"]
    tri, _ = SR.triangles(v, f)
    d = np.stack([SR.tri_d2(p.astype(np.float64), *t) for t in tri], 1)        # [points][12]
    tied = (d == d.min(1, keepdims=True))
    print("cube: triangles at the minimum per point:", tied.sum(1).tolist())
    assert (tied.sum(1) >= 2).all() and tied.sum(1).max() == 12 and np.array_equal(refs["cube_ties"]["nearest"], tied.argmax(1))
    assert (refs["cube_ties"]["d2"][:-1] == 0).all() and refs["cube_ties"]["d2"][-1] == 0.25 and refs["cube_ties"]["sdf"][-1] == 0.5


def test_skips_flags_and_empty_inputs(cases, refs):
    r = refs["broken"]
    v, f, p, _ = cases["broken"]
    clean = SR.mesh_sdf(*C.icosphere(1), p)
    remap = np.concatenate([np.arange(40), np.arange(48, 88)]).astype(np.int32)    # index in the broken mesh of each clean triangle
    assert r["flags"] == SR.FLAG_NONFINITE | SR.FLAG_INVALID
    # the zero-area triangles at (0.7 .. 0.9)^3 act as a segment: some points are nearest to it, the others see the clean sphere
    seg = np.isin(r["nearest"], (40, 41, 42))                               # (40 and 42 repeat an edge and a vertex of the sphere: exact ties)
    print("broken mesh: %d of %d points are nearest to a zero-area triangle" % (seg.sum(), len(p)))
    assert 0 < seg.sum() < len(p) and not np.isin(r["nearest"], (43, 44, 45, 46, 47)).any()
    assert np.array_equal(r["nearest"][~seg], remap[clean["nearest"][~seg]]) and r["d2"][~seg].tobytes() == clean["d2"][~seg].tobytes()
    assert np.array_equal(np.round(r["winding"]), np.round(clean["winding"]))
    e = refs["empty_mesh"]
    assert np.isposinf(e["sdf"]).all() and np.isposinf(e["dist"]).all() and (e["nearest"] == -1).all() and (e["winding"] == 0).all() and e["flags"] == 0
    assert len(refs["empty_queries"]["sdf"]) == 0
    q = refs["nonfinite_query"]
    bad = ~np.isfinite(cases["nonfinite_query"][2]).all(1)
    assert bad.sum() == 3 and np.isposinf(q["sdf"][bad]).all() and (q["nearest"][bad] == -1).all() and (q["winding"][bad] == 0).all()
    assert np.isfinite(q["sdf"][~bad]).all()
    # the unsigned distance is the signed one's magnitude, and the open mesh has a usable one
    assert np.array_equal(C.unsigned_references()["icosphere"]["sdf"], np.abs(refs["icosphere"]["sdf"]))


def test_surface_points_of_the_restatement(cases):
    v, f, _, _ = cases["broken"]
    u = C.uniforms("broken", 4000)
    pts, tri, flags = SR.surface_points(v, f, u)
    tr, status = SR.triangles(v, f)
    assert flags == 3 and (tri >= 0).all() and (status[tri] == 0).all()
    area = MR.triangle_areas(np.nan_to_num(v), np.where(status[:, None] == 0, f, 0))
    assert (area[tri] > 0).all()                                            # a zero-area triangle is never chosen
    a, b, c = tr[tri, 0], tr[tri, 1], tr[tri, 2]
    n = np.cross(b - a, c - a)
    off = np.abs(np.einsum("ij,ij->i", pts - a, n)) / np.linalg.norm(n, axis=1)
    print("surface points: max distance from the chosen triangle's plane %.2e" % off.max())
    assert off.max() < 4 * 2.0 ** -24
    assert SR.surface_points(v, f[40:43], u[:5])[1].tolist() == [-1] * 5 and SR.surface_points(v, f[40:43], u[:5])[2] & SR.FLAG_INVALID
    bad = u[:4].copy()
    bad[0, 0], bad[1, 1], bad[2, 2], bad[3, 0] = 1.0, -0.5, np.nan, 2.0
    assert SR.surface_points(v, f, bad)[1].tolist() == [-1] * 4


# ---- the header on the host --------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    return build_host_program(tmp_path_factory.mktemp("mesh_sdf_host"), "mesh_sdf_host/mesh_sdf_host.cpp", "mesh_sdf_host")


def run_host(exe, packed, want_sign, uniforms, soff, tmp):
    v, f, voff, toff, p, qoff = packed
    B, N, S = len(voff) - 1, len(p), len(uniforms)
    src, dst = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(src, "wb") as fh:
        fh.write(np.array([B, int(want_sign)], np.int32).tobytes() + np.array([len(v), len(f), N, S], np.int64).tobytes())
        for a in (voff, toff, qoff, np.asarray(soff, np.int64), v, f, p, np.asarray(uniforms, np.float32)):
            fh.write(np.ascontiguousarray(a).tobytes())
    r = subprocess.run([exe, src, dst], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    raw = open(dst, "rb").read()
    out, o = {}, 0
    for name, dt, n in (("sdf", np.float32, N), ("dist", np.float32, N), ("d2", np.float64, N), ("nearest", np.int32, N), ("winding", np.float64, N),
                        ("flags", np.int32, B), ("spoints", np.float32, 3 * S), ("striangle", np.int32, S), ("sflags", np.int32, B)):
        out[name] = np.frombuffer(raw, dt, n, o)
        o += n * np.dtype(dt).itemsize
    assert o == len(raw)
    return out


def host_round(exe, names, cases, refs, signed, tmp):
    us = [C.uniforms(n, 50 if len(cases[n][1]) > 100 else 20) for n in names]
    soff = np.concatenate([[0], np.cumsum([len(u) for u in us])]).astype(np.int64)
    out = run_host(exe, C.pack(names), signed, np.concatenate(us), soff, tmp)
    check_against(out, names, cases, refs, signed)
    check_surface(out, names, cases, us, soff)
    return out


def test_header_on_the_host_reproduces_the_restatement(host_program, tmp_path, cases, refs):
    signed = [n for n in cases if n != "cube_ties"]
    host_round(host_program, signed, cases, refs, True, str(tmp_path))
    host_round(host_program, list(cases), cases, C.unsigned_references(), False, str(tmp_path))
    host_round(host_program, ["two_chunks_few"], cases, refs, True, str(tmp_path))         # alone: the same bits as in the batch


def test_header_on_the_host_under_the_sanitizers(tmp_path, cases, refs):
    """a stand-alone program with exact-size buffers: an index outside a mesh, a point run or a workspace is an error here"""
    exe = build_host_program(tmp_path, "mesh_sdf_host/mesh_sdf_host.cpp", "mesh_sdf_host_san",
                             ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    names = [n for n in C.SMALL if n != "cube_ties"]
    out = host_round(exe, names, cases, refs, True, str(tmp_path))
    host_round(exe, list(C.SMALL), cases, C.unsigned_references(), False, str(tmp_path))
    assert out["flags"][names.index("broken")] == 3 and out["flags"][names.index("empty_mesh")] == 0
    # offsets that do not fit together: the mesh is skipped whole, its points keep the defaults, the neighbours keep their bits
    names = ["cube", "broken", "nonfinite_query"]
    v, f, voff, toff, p, qoff = C.pack(names)
    us = np.concatenate([C.uniforms(n, 20) for n in names])
    soff = np.array([0, 20, 40, 60], np.int64)
    for which, bad in (("voff", np.array([0, 8, len(v) + 1, len(v)], np.int64)), ("toff", np.array([0, 12, -5, len(f)], np.int64))):
        o = run_host(exe, (v, f, bad if which == "voff" else voff, bad if which == "toff" else toff, p, qoff), True, us, soff, str(tmp_path))
        n0, n1 = qoff[1], qoff[2]
        assert o["sdf"][:n0].tobytes() == refs["cube"]["sdf"].tobytes(), which
        assert np.isposinf(o["sdf"][n0:n1]).all() and (o["nearest"][n0:n1] == -1).all() and o["flags"][1] == SR.FLAG_INVALID, which
        assert (o["striangle"][20:40] == -1).all() and o["sflags"][1] == SR.FLAG_INVALID and (o["striangle"][:20] >= 0).all(), which
    o = run_host(exe, (v, f, voff, toff, p, np.array([0, qoff[1], len(p) + 7, len(p)], np.int64)), True, us, soff, str(tmp_path))
    assert o["sdf"][:qoff[1]].tobytes() == refs["cube"]["sdf"].tobytes() and np.isposinf(o["sdf"][qoff[1]:]).all()
    assert o["flags"].tolist() == [0, 3, 0]                                 # the meshes themselves are fine: only their points are not served


# ---- header, ctypes table, library -------------------------------------------------------------------------------------------------------------

NEW = ("sdfr_mesh_sdf_ws_bytes", "sdfr_mesh_sdf", "sdfr_mesh_surface_ws_bytes", "sdfr_mesh_surface_points")


def test_abi_has_the_mesh_sdf_entry_points():
    from sdflabel_amd import _lib
    header = open(os.path.join(ROOT, "include", "sdfr.h")).read()
    h = _lib.lib()
    for name in NEW:
        assert name in _lib.EXPORTS and hasattr(h, name) and re.search(r"\bint(64_t)? %s\(" % name, header), name
    assert int(re.search(r"#define SDFR_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION == h.sdfr_version() >= 415
    sh = open(os.path.join(ROOT, "sdflabel_amd", "csrc", "build.sh")).read()
    assert re.search(r"-ffp-contract=off -c \"\$HERE/mesh_sdf\.hip\"", sh) and "synth,mesh_sdf}.o" in sh
    src = open(os.path.join(ROOT, "sdflabel_amd", "csrc", "mesh_sdf.hip")).read()
    assert "atomic" not in "\n".join(l.split("//")[0] for l in src.splitlines())          # no atomics: the same bits on every run


def test_argument_checks_come_before_any_launch():
    from sdflabel_amd import _lib
    h = _lib.lib()
    none20 = dict(vertices=None, V=0, faces=None, T=0, voff=None, toff=None, points=None, N=0, qoff=None)

    def sdf(B=1, want_sign=1, ws=None, ws_bytes=0, **kw):
        a = dict(none20, **kw)
        return h.sdfr_mesh_sdf(a["vertices"], a["V"], a["faces"], a["T"], a["voff"], a["toff"], a["points"], a["N"], a["qoff"], B, want_sign, ws,
                               ws_bytes, None, None, None, None, None, None, None)

    assert sdf(B=0) == 0                                                    # nothing to do
    assert sdf() == -1 and b"NULL" in h.sdfr_last_error()
    assert sdf(B=-1) == -1 and sdf(T=1 << 31) == -1 and sdf(N=-1) == -1 and b"out of range" in h.sdfr_last_error()
    assert sdf(want_sign=2) == -1 and b"want_sign" in h.sdfr_last_error()
    assert h.sdfr_mesh_sdf_ws_bytes(-1, 0, 0) == -1 and h.sdfr_mesh_sdf_ws_bytes(2, 1 << 31, 0) == -1
    assert h.sdfr_mesh_sdf_ws_bytes(2, 5000, 9000) == 24                    # many points: the block table alone
    assert h.sdfr_mesh_sdf_ws_bytes(2, 3, 9000) == 24 + 3 * 3 * 20 + 4      # few points, three chunks: the partials, rounded up to 8
    assert h.sdfr_mesh_sdf_ws_bytes(2, 3, 4096) == 24                       # one chunk: nothing to split
    assert h.sdfr_mesh_surface_ws_bytes(2, 1000) == 24 + 8000 + 6 * 20 and h.sdfr_mesh_surface_ws_bytes(-1, 0) == -1
    assert h.sdfr_mesh_surface_points(None, 0, None, 0, None, None, None, 0, None, 0, None, 0, None, None, None, None) == 0
    assert h.sdfr_mesh_surface_points(None, 0, None, 0, None, None, None, 5, None, 0, None, 0, None, None, None, None) == -1
    assert h.sdfr_mesh_surface_points(None, 0, None, 0, None, None, None, 0, None, 1, None, 0, None, None, None, None) == -1
    assert b"NULL" in h.sdfr_last_error()


# ---- the Python side without a GPU ---------------------------------------------------------------------------------------------------------------

def test_sdf_samples_npz_round_trip(tmp_path):
    import torch
    from sdflabel_amd.sdf_samples import SdfSamples, sample_counts
    rng = np.random.default_rng(0)
    rows = rng.normal(size=(50, 4)).astype(np.float32)
    rows[3, 3] = 0.0
    s = SdfSamples(torch.from_numpy(rows), None, (20, 20, 10))
    path = str(tmp_path / "shape.npz")
    s.save(path)
    z = np.load(path)
    assert sorted(z.files) == ["neg", "pos"] and (z["pos"][:, 3] >= 0).all() and (z["neg"][:, 3] < 0).all()
    assert z["pos"].dtype == np.float32 and z["pos"].shape[1] == 4 and len(z["pos"]) + len(z["neg"]) == 50
    back = SdfSamples.load(path)
    want = np.concatenate([rows[rows[:, 3] >= 0], rows[rows[:, 3] < 0]])
    assert len(back) == 50 and back.numpy().tobytes() == want.tobytes()
    assert sample_counts(500000, (0.47, 0.47)) == (235000, 235000, 30000) and sample_counts(10, (0.5, 0.5)) == (5, 5, 0)
    with pytest.raises(ValueError):
        sample_counts(10, (0.7, 0.7))


def test_load_obj_against_load_ply(tmp_path):
    import torch
    from sdflabel_amd.mesh import Mesh, load_obj, load_ply
    v, f = C.icosphere(1)
    n = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)
    for nrm in (None, n):
        m = Mesh(torch.from_numpy(v), torch.from_numpy(f), None if nrm is None else torch.from_numpy(nrm))
        m.save(str(tmp_path / "m.ply"))
        m.save(str(tmp_path / "m.obj"))
        pv, pn, pf = load_ply(str(tmp_path / "m.ply"))
        ov, on, of = load_obj(str(tmp_path / "m.obj"))
        assert ov.tobytes() == pv.tobytes() and of.tobytes() == pf.tobytes() and ov.dtype == np.float32 and of.dtype == np.int32
        assert (on is None) == (pn is None) and (on is None or on.tobytes() == pn.tobytes())
    # polygons are fanned, indices may be negative or of the a/b/c form, comments and other lines are ignored
    (tmp_path / "q.obj").write_text("# a square and a triangle\nmtllib x.mtl\nv 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nvt 0 0\nf 1/1 2/1 3/1 4/1\n"
                                    "v 0 0 1\nf -1 -5 -4\nf 1//1 2//1 5//1\n")
    qv, qn, qf = load_obj(str(tmp_path / "q.obj"))
    assert qv.shape == (5, 3) and qn is None and qf.tolist() == [[0, 1, 2], [0, 2, 3], [4, 0, 1], [0, 1, 4]]
    (tmp_path / "bad.obj").write_text("v 0 0 0\nf 1 2 3\n")
    with pytest.raises(ValueError):
        load_obj(str(tmp_path / "bad.obj"))


def test_fit_frame_and_normalize():
    from sdflabel_amd.sdf_samples import fit_frame, normalize
    v = np.array([[1, 2, 3], [5, 2, 3], [3, 4, 3], [3, 2, 9], [np.nan, 0, 0]], np.float32)
    c, s = fit_frame(v, "unit_sphere", buffer=1.03)
    assert c.tolist() == [3.0, 3.0, 6.0] and c.dtype == np.float64
    far = np.sqrt(((v[:4].astype(np.float64) - c) ** 2).sum(1)).max()
    assert s == 1.0 / (far * 1.03)
    x = normalize(v[:4], c, s)
    assert x.dtype == np.float32 and abs(np.linalg.norm(x.astype(np.float64), axis=1).max() - 1 / 1.03) < 1e-6
    c, s = fit_frame(v, "unit_cube", buffer=1.0)
    assert s == 1.0 / 3.0 and np.abs(normalize(v[:4], c, s)).max() == 1.0
    c, s = fit_frame(v, None)
    assert c.tolist() == [0, 0, 0] and s == 1.0 and normalize(v[:4], c, s).tobytes() == v[:4].tobytes()
    with pytest.raises(ValueError):
        fit_frame(v, "ball")
    with pytest.raises(ValueError):
        fit_frame(v[:1], "unit_sphere")


def test_python_side_refuses_host_tensors():
    import torch
    from sdflabel_amd import _lib
    from sdflabel_amd.mesh import Mesh
    from sdflabel_amd.sdf_samples import mesh_sdf_many
    v, f = C.unit_cube()
    m = Mesh(torch.from_numpy(v), torch.from_numpy(f))
    with pytest.raises(_lib.SdfrError):
        mesh_sdf_many([m], [torch.zeros((3, 3))])                           # no CPU fallback
    with pytest.raises(_lib.SdfrError):
        m.signed_distance(torch.zeros((3, 3)))
