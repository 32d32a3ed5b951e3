"""Mesh extraction on the device (csrc/mesh.hip, sdflabel_amd/mesh.py) against the numpy restatement tests/_mesh_ref.py: counts, faces and
vertex bits must be equal.  Every figure is printed before it is asserted."""
import ctypes

import numpy as np
import pytest
import torch

import sdflabel_amd
from sdflabel_amd import _lib
from sdflabel_amd import mesh as M
from sdflabel_amd.fixtures import ASSET, ASSET_ELLIPSOID, GT_LATENT
from sdflabel_amd.frame import BAND_THRESHOLD
from tests import _mesh_ref as MR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV)


def assert_equals_restatement(mesh, sdf):
    rv, rf, _ = MR.extract(sdf)
    v, f = mesh.vertices_numpy(), mesh.faces_numpy()
    assert v.shape == rv.shape and f.shape == rf.shape, (v.shape, rv.shape, f.shape, rf.shape)
    assert f.dtype == np.int32 and np.array_equal(f, rf)
    assert v.dtype == np.float32 and v.tobytes() == rv.tobytes()
    return rv, rf


def test_single_cell_every_mixed_pattern_of_a_tetrahedron_chain():
    rng = np.random.default_rng(0)
    chain = [(0, 0, 0), (1, 0, 0), (1, 1, 0), (1, 1, 1)]                     # the first tetrahedron: x, then y, then z
    cells = []
    for mask in range(1, 15):
        s = rng.uniform(0.1, 1.0, (2, 2, 2)).astype(np.float32)              # the other four corners stay outside
        for i, c in enumerate(chain):
            if mask >> i & 1:
                s[c] = -s[c]
        cells.append(s)
    sdf = np.stack(cells)
    meshes = M.mesh_from_sdf(dev(sdf))
    assert len(meshes) == 14
    for b, m in enumerate(meshes):
        rv, rf = assert_equals_restatement(m, sdf[b])
        assert len(rf) > 0


@pytest.mark.parametrize("R,name", [(3, "sphere"), (9, "torus"), (41, "sphere")])
def test_equals_restatement(R, name):
    """R = 9: 729 points, three scan blocks with a tail; R = 41: 68 921 points, 270 blocks, the second level of the scan"""
    sdf = MR.shape_sdf(name, R) if R > 3 else (MR.shape_sdf("sphere", 3) + np.float32(0.3))
    (m,) = M.mesh_from_sdf(dev(sdf))
    rv, rf = assert_equals_restatement(m, sdf)
    print("R = %d %s: %d vertices, %d triangles" % (R, name, len(rv), len(rf)))
    assert len(rf) > 0
    if R > 3:
        assert m.is_closed() and m.volume() > 0


def test_random_signs_cover_every_case():
    sdf = np.random.default_rng(3).standard_normal((2, 11, 11, 11)).astype(np.float32)
    for b, m in enumerate(M.mesh_from_sdf(dev(sdf))):
        assert_equals_restatement(m, sdf[b])


def test_ragged_batch_equals_solo_and_other_positions():
    R = 9
    sphere = MR.shape_sdf("sphere", R)
    empty, full = np.ones_like(sphere), -np.ones_like(sphere)
    a = M.mesh_from_sdf(dev(np.stack([sphere, empty, full])))
    b = M.mesh_from_sdf(dev(np.stack([full, empty, sphere])))
    (solo,) = M.mesh_from_sdf(dev(sphere))
    assert [len(m) for m in a] == [len(solo), 0, 0] and [len(m) for m in b] == [0, 0, len(solo)]
    assert a[1].vertices.shape == (0, 3) and a[2].vertices.shape == (0, 3)          # all inside: nothing, the boundary is not capped
    assert_equals_restatement(solo, sphere)
    for m in (a[0], b[2]):
        assert torch.equal(m.vertices, solo.vertices) and torch.equal(m.faces, solo.faces)
    assert not a[1].is_closed()


def test_open_surface_exact_zeros_and_nan():
    cut = MR.shape_sdf("cut_sphere", 9)
    octa = MR.shape_sdf("octahedron", 9)
    nan = MR.shape_sdf("sphere", 9)
    nan[3, :, 5] = np.nan
    nan[6, 6, :] = np.nan
    m_cut, m_oct, m_nan = M.mesh_from_sdf(dev(np.stack([cut, octa, nan])))
    assert_equals_restatement(m_cut, cut)
    cnt = MR.undirected_edge_counts(m_cut.faces_numpy())
    assert cnt.max() == 2 and cnt.min() == 1 and not m_cut.is_closed()
    rv, rf = assert_equals_restatement(m_oct, octa)
    assert (MR.triangle_areas(rv, rf) == 0).sum() > 0 and m_oct.is_closed() and MR.euler_characteristic(m_oct.faces_numpy()) == 2
    assert len(m_oct.faces_numpy(drop_degenerate=True)) < len(m_oct)
    assert_equals_restatement(m_nan, nan)
    assert np.isfinite(m_nan.vertices_numpy()).all() and len(m_nan) > 0


def test_two_runs_give_the_same_bits():
    sdf = dev(MR.shape_sdf("torus", 13))
    (a,), (b,) = M.mesh_from_sdf(sdf), M.mesh_from_sdf(sdf)
    assert torch.equal(a.vertices, b.vertices) and torch.equal(a.faces, b.faces)


def test_emit_refuses_an_undersized_capacity_and_bad_arguments():
    L = _lib.lib()
    R = 9
    sdf = dev(MR.shape_sdf("sphere", R)).view(-1)
    rv, rf, _ = MR.extract(MR.shape_sdf("sphere", R))
    nb = int(L.sdfr_mesh_ws_bytes(R, 1))
    assert nb > 0 and L.sdfr_mesh_ws_bytes(1, 1) == -1 and L.sdfr_mesh_ws_bytes(257, 1) == -1 and L.sdfr_mesh_ws_bytes(256, 128) == -1
    ws = torch.zeros(nb, dtype=torch.uint8, device=DEV)
    cnt = torch.zeros(2, dtype=torch.int32, device=DEV)
    st = _lib.stream_ptr()
    P = _lib.ptr
    assert L.sdfr_mesh_count(P(sdf), R, 1, P(cnt[0:]), P(cnt[1:]), P(ws), nb, st) == 0
    nv, nt = cnt.cpu().tolist()
    assert (nv, nt) == (len(rv), len(rf))
    voff, toff = (ctypes.c_int64 * 2)(0, nv), (ctypes.c_int64 * 2)(0, nt)
    verts = torch.full((nv, 3), 7.0, device=DEV)
    faces = torch.full((nt, 3), -5, dtype=torch.int32, device=DEV)
    for cap_v, cap_t in ((nv - 1, nt), (nv, nt - 1)):
        rc = L.sdfr_mesh_emit(P(sdf), R, 1, voff, toff, P(ws), nb, P(verts), cap_v, P(faces), cap_t, st)
        assert rc == -1 and b"room for" in L.sdfr_last_error()
    torch.cuda.synchronize()
    assert (verts == 7.0).all() and (faces == -5).all()                         # nothing was written
    # offsets that claim fewer elements than the shape has: the tail beyond them stays untouched
    voff2, toff2 = (ctypes.c_int64 * 2)(0, nv - 5), (ctypes.c_int64 * 2)(0, nt - 9)
    assert L.sdfr_mesh_emit(P(sdf), R, 1, voff2, toff2, P(ws), nb, P(verts), nv, P(faces), nt, st) == 0
    torch.cuda.synchronize()
    assert (verts[nv - 5:] == 7.0).all() and (faces[nt - 9:] == -5).all()
    assert verts[:nv - 5].cpu().numpy().tobytes() == rv[:nv - 5].tobytes() and np.array_equal(faces[:nt - 9].cpu().numpy(), rf[:nt - 9])
    # argument checks come before any launch
    assert L.sdfr_mesh_count(P(sdf), 1, 1, P(cnt[0:]), P(cnt[1:]), P(ws), nb, st) == -1
    assert L.sdfr_mesh_count(None, R, 1, P(cnt[0:]), P(cnt[1:]), P(ws), nb, st) == -1
    assert L.sdfr_mesh_count(P(sdf), R, 1, P(cnt[0:]), P(cnt[1:]), P(ws), nb - 1, st) == -1
    assert L.sdfr_mesh_count(P(sdf), 256, 128, P(cnt[0:]), P(cnt[1:]), P(ws), nb, st) == -1 and b"2^31" in L.sdfr_last_error()
    assert L.sdfr_mesh_emit(P(sdf), R, 1, None, toff, P(ws), nb, P(verts), nv, P(faces), nt, st) == -1
    assert L.sdfr_mesh_lattice_inputs(None, 3, R, 1, 0, 10, P(verts), st) == -1
    assert L.sdfr_mesh_lattice_inputs(P(verts), 3, R, 1, R ** 3 - 5, 10, P(verts), st) == -1
    with pytest.raises(_lib.SdfrError):
        M.mesh_from_sdf(torch.zeros(3, 3, 3))
    with pytest.raises(ValueError):
        M.mesh_from_sdf(torch.zeros(1, 1, 1, device=DEV))


def test_lattice_inputs_rows():
    L = _lib.lib()
    R, Ld = 5, 4
    lat = torch.arange(2 * Ld, dtype=torch.float32, device=DEV).view(2, Ld)
    out = torch.empty((2, 40, Ld + 3), device=DEV)
    _lib.check(L.sdfr_mesh_lattice_inputs(_lib.ptr(lat), Ld, R, 2, 50, 40, _lib.ptr(out), _lib.stream_ptr()), "sdfr_mesh_lattice_inputs")
    pts = MR.lattice_points(R)[50:90]
    for b in range(2):
        assert torch.equal(out[b, :, :Ld], lat[b].expand(40, Ld))
        assert out[b, :, Ld:].cpu().numpy().tobytes() == pts.tobytes()
    assert M.lattice_points(R).numpy().tobytes() == MR.lattice_points(R).tobytes()


# ---- the decoder's shapes ------------------------------------------------------------------------------------------------------------------

RES = 24
LATENTS = [GT_LATENT, (0.1, 0.2, -0.4)]


@pytest.fixture(scope="module", params=[ASSET, ASSET_ELLIPSOID], ids=["synth", "ellipsoid"])
def fit(request):
    dec = sdflabel_amd.setup_dsdf(request.param + ".pt", precision=torch.float32)[0].to(DEV)
    lat = torch.tensor(LATENTS, device=DEV)
    raw = M.meshes_many(dec, lat, resolution=RES, polish=False, normals=True, return_sdf=True)
    pol = M.meshes_many(dec, lat, resolution=RES, polish=True, normals=True)
    return dec, lat, raw, pol


def test_meshes_many_equals_the_restatement_on_the_devices_own_sdf(fit):
    dec, lat, raw, pol = fit
    for m, p in zip(raw, pol):
        sdf = m.sdf.cpu().numpy()
        assert sdf.shape == (RES, RES, RES)
        rv, rf = assert_equals_restatement(m, sdf)
        assert torch.equal(p.faces, m.faces) and p.vertices.shape == m.vertices.shape
        for x in (m, p):
            assert x.is_closed() and MR.euler_characteristic(x.faces_numpy()) == 2 and x.volume() > 0
        print("R = %d: %d vertices, %d triangles, volume %.5f (polished %.5f)" % (RES, len(rv), len(rf), m.volume(), p.volume()))
    # the latent went in raw: the samples are the decoder's at the lattice points with the latent as given
    pts = M.lattice_points(RES, DEV)
    want, _ = dec(torch.cat([lat[0].expand(pts.shape[0], -1), pts], 1))
    assert torch.equal(want.view(-1), raw[0].sdf.view(-1))


def test_meshes_many_normals_agree_with_the_winding(fit):
    _, _, raw, pol = fit
    for m in raw + pol:
        v, f, n = m.vertices_numpy().astype(np.float64), m.faces_numpy(), m.normals_numpy().astype(np.float64)
        assert np.abs(np.linalg.norm(n, axis=1) - 1).max() < 1e-5
        g = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
        ok = np.linalg.norm(g, axis=1) > 0
        d = np.einsum("ij,ij->i", g[ok], n[f[ok]].mean(1))
        print("triangles %d (zero area %d): min of normal . mean decoder normal / |normal| = %.3g" %
              (len(f), int((~ok).sum()), (d / np.linalg.norm(g[ok], axis=1)).min()))
        assert (d > 0).all()


def test_polish_brings_the_vertices_onto_the_surface(fit):
    dec, lat, raw, pol = fit
    for b, (m, p) in enumerate(zip(raw, pol)):
        def residual(x):
            inp = torch.cat([lat[b].expand(x.vertices.shape[0], -1), x.vertices], 1)
            return float(dec.forward_float64(inp).abs().max())
        e_raw, e_pol = residual(m), residual(p)
        print("shape %d: max |sdf| at the vertices %.3e unpolished, %.3e polished (band threshold %.2g)" % (b, e_raw, e_pol, BAND_THRESHOLD))
        assert e_pol < e_raw and e_pol < BAND_THRESHOLD


def test_chunked_staging_gives_the_bits_of_one_chunk(fit):
    dec, lat, raw, pol = fit
    small = 3000 * 4 * (lat.shape[1] + 3)                                    # about 3000 rows in flight: five chunks per shape
    a = M.meshes_many(dec, lat, resolution=RES, polish=True, return_sdf=True, staging_bytes=small)
    b = M.meshes_many(dec, lat, resolution=RES, polish=False, return_sdf=True, max_batch=1)
    for x, y, r, p in zip(a, b, raw, pol):
        assert torch.equal(x.sdf, r.sdf) and torch.equal(y.sdf, r.sdf)
        assert torch.equal(x.faces, p.faces) and torch.equal(x.vertices, p.vertices) and torch.equal(x.normals, p.normals)
        assert torch.equal(y.faces, r.faces) and torch.equal(y.vertices, r.vertices)


def test_float16_decoder_and_parameter_dicts():
    dec = sdflabel_amd.setup_dsdf(ASSET + ".pt", precision=torch.float16)[0].to(DEV)
    params = [{"latent": torch.tensor(GT_LATENT, device=DEV), "scale": torch.tensor([2.0]), "yaw": torch.tensor([0.6]),
               "trans": torch.tensor([0.1, 0.0, 3.5])}]
    (m,) = M.meshes_many(dec, params, resolution=RES, return_sdf=True)
    assert m.is_closed() and MR.euler_characteristic(m.faces_numpy()) == 2 and m.volume() > 0
    (r,) = M.mesh_from_sdf(m.sdf)
    assert torch.equal(r.faces, m.faces)
    c = m.to_camera()
    print("float16 decoder: %d triangles, volume %.5f, camera-frame volume %.5f" % (len(m), m.volume(), c.volume()))
    assert c.is_closed() and c.volume() > 0 and abs(c.volume() - 8.0 * m.volume()) < 1e-3 * c.volume()
    assert m.scale == 2.0 and m.cam_T.shape == (4, 4)


def test_layernorm_decoder_takes_the_recomputing_jacobian():
    from sdflabel_amd.fixtures import ASSET_ELLIPSOID_LN
    dec = sdflabel_amd.setup_dsdf(ASSET_ELLIPSOID_LN + ".pt", precision=torch.float32)[0].to(DEV)
    (m,) = M.meshes_many(dec, torch.tensor([GT_LATENT], device=DEV), resolution=16)
    assert m.is_closed() and m.volume() > 0 and np.isfinite(m.normals_numpy()).all()


# ---- the frame pipeline ----------------------------------------------------------------------------------------------------------------------

def test_refine_frame_meshes():
    from sdflabel_amd.pipelines import optimizer as OP
    from sdflabel_amd.pipelines.frame import refine_frame
    from tests.test_gpu_frame import _synthetic_frame
    dec32 = sdflabel_amd.setup_dsdf(ASSET + ".pt", precision=torch.float32)[0].to(DEV)
    dec16 = sdflabel_amd.setup_dsdf(ASSET + ".pt", precision=torch.float16)[0].to(DEV)
    annos, K_orig, latents = _synthetic_frame(dec32, n=4)
    grid = sdflabel_amd.Grid3D(40, DEV)
    p_WC = np.eye(4)
    p_WC[:3, 3] = [0.1, -0.2, 0.3]
    W8 = {"2d": 0.3, "3d": 0.5}
    R = 16
    with pytest.raises(ValueError):
        refine_frame(annos, dec16, grid, latents, K_orig, p_WC, 3, W8, seed=7, mesh_resolution=R)
    OP.clear_refiner_cache()
    est0, kept0 = refine_frame(annos, dec16, grid, latents, K_orig, p_WC, 3, W8, seed=7)
    OP.clear_refiner_cache()
    est, kept, st = refine_frame(annos, dec16, grid, latents, K_orig, p_WC, 3, W8, seed=7, return_stages=True, mesh_resolution=R)
    assert kept == kept0 and len(kept) >= 2
    for k in est0:
        assert (est[k] == est0[k]) if k == "name" else (est[k].dtype == est0[k].dtype and est[k].tobytes() == est0[k].tobytes()), k
    labels = [lab for lab in st["labels"] if lab is not None]
    assert len(st["meshes"]) == len(kept) == len(labels)
    for m, (lab, pts, cam_T) in zip(st["meshes"], labels):
        assert m.frame == "camera" and m.is_closed() and m.volume() > 0
        scale = float(m.scale)
        # the box of the camera-frame mesh along the label's own axes (the columns of cam_T's rotation): height, width, length
        v = (m.vertices_numpy().astype(np.float64) - cam_T[:3, 3]) @ cam_T[:3, :3]
        ext = v.max(0) - v.min(0)
        dims = np.asarray(lab["dimensions"], np.float64)
        tol = 2.0 * scale / (R - 1) + BAND_THRESHOLD * scale
        print("mesh box (h, w, l) %s, label dimensions %s, tolerance %.4f" % (ext[[1, 0, 2]], dims, tol))
        assert np.abs(ext[[1, 0, 2]] - dims).max() < tol
