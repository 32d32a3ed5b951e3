"""Signed distances to meshes on the device (csrc/mesh_sdf.hip, sdflabel_amd/sdf_samples.py) against the numpy restatement
tests/_mesh_sdf_ref.py: sdf, dist, d2, nearest, the surface points, their triangles and the flags must be EQUAL -- both sides do the same
float64 operations in the same order -- and the winding number, whose atan2 differs between libraries, stays within its rounding bound.
Every figure is printed before it is asserted."""
import warnings

import numpy as np
import pytest
import torch

import sdflabel_amd
from sdflabel_amd import _lib
from sdflabel_amd import mesh as M
from sdflabel_amd import sdf_samples as S
from sdflabel_amd.fixtures import ASSET, GT_LATENT
from tests import _mesh_ref as MR
from tests import _mesh_sdf_cases as C
from tests import _mesh_sdf_ref as SR
from tests._mesh_sdf_cases import check_against, check_surface, lattice_bound

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 256


def count_syncs(fn):
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            out = fn()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    return sum("synchroniz" in str(x.message).lower() for x in w), out


@pytest.fixture(scope="module")
def cases():
    return C.cases()


@pytest.fixture(scope="module")
def refs():
    return C.references()


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def guarded(n, dtype, fill):
    return torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)


def inner(t, n, fill):
    """the n values between the guard rows, after checking that the guards are untouched"""
    h = t.cpu().numpy()
    assert (h[:GUARD] == fill).all() and (h[GUARD + n:] == fill).all(), "a guard row was written"
    return h[GUARD:GUARD + n]


def raw_sdf(packed, want_sign):
    """sdfr_mesh_sdf on outputs that sit between guard rows -> the dict the host harness gives"""
    L = _lib.lib()
    v, f, voff, toff, p, qoff = packed
    B, N = len(voff) - 1, len(p)
    d = [up(x) for x in (v, f, voff, toff, p, qoff)]
    nbytes = int(L.sdfr_mesh_sdf_ws_bytes(B, N, len(f)))
    ws = guarded(nbytes // 8, torch.int64, 0x55)
    outs = dict(sdf=(torch.float32, 7.0), dist=(torch.float32, 7.0), d2=(torch.float64, 7.0), nearest=(torch.int32, -5), winding=(torch.float64, 7.0))
    t = {k: guarded(N, dt, fill) for k, (dt, fill) in outs.items()}
    flags = guarded(B, torch.int32, 99)
    P = _lib.ptr
    _lib.check(L.sdfr_mesh_sdf(P(d[0]) if len(v) else None, len(v), P(d[1]) if len(f) else None, len(f), P(d[2]), P(d[3]), P(d[4]) if N else None, N,
                               P(d[5]), B, int(want_sign), P(ws[GUARD:]), nbytes, P(t["sdf"][GUARD:]), P(t["dist"][GUARD:]), P(t["d2"][GUARD:]),
                               P(t["nearest"][GUARD:]), P(t["winding"][GUARD:]), P(flags[GUARD:]), _lib.stream_ptr()), "sdfr_mesh_sdf")
    out = {k: inner(t[k], N, fill) for k, (_, fill) in outs.items()}
    out["flags"] = inner(flags, B, 99)
    inner(ws, nbytes // 8, 0x55)
    return out


def raw_surface(packed, uniforms, soff):
    L = _lib.lib()
    v, f, voff, toff, _, _ = packed
    B, Sn = len(voff) - 1, len(uniforms)
    d = [up(x) for x in (v, f, voff, toff, np.asarray(uniforms, np.float32), np.asarray(soff, np.int64))]
    nbytes = int(L.sdfr_mesh_surface_ws_bytes(B, len(f)))
    ws = guarded(nbytes // 8, torch.int64, 0x55)
    pts, tri, flags = guarded(3 * Sn, torch.float32, 7.0), guarded(Sn, torch.int32, -5), guarded(B, torch.int32, 99)
    P = _lib.ptr
    _lib.check(L.sdfr_mesh_surface_points(P(d[0]) if len(v) else None, len(v), P(d[1]) if len(f) else None, len(f), P(d[2]), P(d[3]), P(d[4]), Sn,
                                          P(d[5]), B, P(ws[GUARD:]), nbytes, P(pts[GUARD:]), P(tri[GUARD:]), P(flags[GUARD:]), _lib.stream_ptr()),
               "sdfr_mesh_surface_points")
    inner(ws, nbytes // 8, 0x55)
    return dict(spoints=inner(pts, 3 * Sn, 7.0), striangle=inner(tri, Sn, -5), sflags=inner(flags, B, 99))


def piece(out, qoff, b):
    return {k: out[k][qoff[b]:qoff[b + 1]] for k in ("sdf", "dist", "d2", "nearest", "winding")}


def same_bits(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in a)


# ---- the kernels against the restatement ---------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def signed_batch(cases):
    names = [n for n in cases if n != "cube_ties"]
    packed = C.pack(names)
    return names, packed, raw_sdf(packed, True)


def test_signed_batch_equals_the_restatement(cases, refs, signed_batch):
    names, _, out = signed_batch
    check_against(out, names, cases, refs, True, "device")


def test_unsigned_batch_of_all_cases_equals_the_restatement(cases, refs, signed_batch):
    names = list(cases)
    out = raw_sdf(C.pack(names), False)
    check_against(out, names, cases, C.unsigned_references(), False, "device")
    # want_sign = 0 gives the same dist and nearest as the signed run
    snames, spacked, sout = signed_batch
    qoff, sq = C.pack(names)[5], spacked[5]
    for n in snames:
        a, b = piece(out, qoff, names.index(n)), piece(sout, sq, snames.index(n))
        assert all(a[k].tobytes() == b[k].tobytes() for k in ("dist", "d2", "nearest")), n


def test_alone_in_the_batch_and_at_another_position_give_the_same_bits(cases, signed_batch):
    names, packed, out = signed_batch
    moved = names[3:] + names[:3]
    out2, q2 = raw_sdf(C.pack(moved), True), C.pack(moved)[5]
    again = raw_sdf(packed, True)
    assert same_bits({k: out[k] for k in out}, {k: again[k] for k in again})            # two runs: the same bits, winding included
    for n in names:
        a = piece(out, packed[5], names.index(n))
        assert same_bits(a, piece(out2, q2, moved.index(n))), n
        if n in ("icosphere", "open", "broken", "cube", "nonfinite_query", "one_chunk_exactly"):
            alone = raw_sdf(C.pack([n]), True)
            assert same_bits(a, piece(alone, np.array([0, len(cases[n][2])]), 0)) and alone["flags"][0] == out["flags"][names.index(n)], n


def test_both_launch_shapes_give_the_same_bits(cases, refs, signed_batch):
    """3 points of the two-chunk mesh alone take the chunk-split shape (partials in the workspace, folded in chunk order), 3 000 the plain one"""
    L = _lib.lib()
    T = len(cases["two_chunks"][1])
    assert L.sdfr_mesh_sdf_ws_bytes(1, 3, T) > 16 and L.sdfr_mesh_sdf_ws_bytes(1, 3000, T) == 16 and T > SR.CHUNK
    few = raw_sdf(C.pack(["two_chunks_few"]), True)
    many = raw_sdf(C.pack(["two_chunks"]), True)
    check_against(few, ["two_chunks_few"], cases, refs, True, "device split")
    check_against(many, ["two_chunks"], cases, refs, True, "device plain")
    assert same_bits(piece(few, np.array([0, 3]), 0), {k: many[k][:3] for k in ("sdf", "dist", "d2", "nearest", "winding")})
    few0 = raw_sdf(C.pack(["two_chunks_few"]), False)
    assert few0["d2"].tobytes() == few["d2"].tobytes() and few0["nearest"].tobytes() == few["nearest"].tobytes() and not few0["winding"].any()
    # a small batch in the split shape: meshes of one and of two chunks, an empty one, non-finite queries
    names = ["cube", "two_chunks_few", "empty_mesh", "nonfinite_query", "one_chunk_exactly", "broken"]
    packed = C.pack(names)
    assert L.sdfr_mesh_sdf_ws_bytes(len(names), len(packed[4]), len(packed[1])) > 8 * (len(names) + 1)
    check_against(raw_sdf(packed, True), names, cases, refs, True, "device split batch")


def test_offsets_that_do_not_fit_skip_the_mesh(cases, refs):
    names = ["cube", "broken", "nonfinite_query"]
    v, f, voff, toff, p, qoff = C.pack(names)
    bad = voff.copy()
    bad[2] = len(v) + 1
    o = raw_sdf((v, f, bad, toff, p, qoff), True)
    assert o["sdf"][:qoff[1]].tobytes() == refs["cube"]["sdf"].tobytes() and np.isposinf(o["sdf"][qoff[1]:]).all()
    assert (o["nearest"][qoff[1]:] == -1).all() and o["flags"].tolist() == [0, 2, 2]
    o = raw_sdf((v, f, voff, toff, p, np.array([0, qoff[1], len(p) + 7, len(p)], np.int64)), True)
    assert o["sdf"][:qoff[1]].tobytes() == refs["cube"]["sdf"].tobytes() and np.isposinf(o["sdf"][qoff[1]:]).all() and o["flags"].tolist() == [0, 3, 0]


# ---- surface points ----------------------------------------------------------------------------------------------------------------------------

def test_surface_points_equal_the_restatement_and_lie_on_their_triangles(cases):
    names = ["icosphere", "broken", "cube", "empty_mesh", "two_chunks", "lattice_torus"]
    us = [C.uniforms(n, 300) for n in names]
    soff = np.concatenate([[0], np.cumsum([len(u) for u in us])]).astype(np.int64)
    packed = C.pack(names)
    out = raw_surface(packed, np.concatenate(us), soff)
    check_surface(out, names, cases, us, soff)
    assert same_bits(out, raw_surface(packed, np.concatenate(us), soff))
    for b, n in enumerate(names):
        tri = out["striangle"][soff[b]:soff[b + 1]]
        if n == "empty_mesh":
            assert (tri == -1).all() and out["sflags"][b] == SR.FLAG_INVALID
            continue
        tr, status = SR.triangles(cases[n][0], cases[n][1])
        x = out["spoints"].reshape(-1, 3)[soff[b]:soff[b + 1]].astype(np.float64)
        a, bb, c = tr[tri, 0], tr[tri, 1], tr[tri, 2]
        nrm = np.cross(bb - a, c - a)
        assert (tri >= 0).all() and (status[tri] == 0).all() and (np.linalg.norm(nrm, axis=1) > 0).all(), n      # never a zero-area triangle
        # on the triangle within the float32 rounding of the coordinates: each is off by at most 2^-24 of its size
        tol = 2.0 ** -24 * np.linalg.norm(x, axis=1) + 1e-15
        d = np.sqrt(np.stack([SR.tri_d2(x[i:i + 1], *t) for i, t in enumerate(tr[tri])]).ravel())
        print("%-14s max distance from the triangle %.2e (smallest tolerance %.2e)" % (n, d.max(), tol.min()))
        assert (d <= tol).all(), n


def test_triangle_histogram_follows_the_areas(cases):
    v, f, _, _ = cases["broken"]
    n = 20000
    u = np.random.default_rng(5).random((n, 3), dtype=np.float32)
    out = raw_surface(C.pack(["broken"]), u, np.array([0, n], np.int64))
    tr, status = SR.triangles(v, f)
    area = np.where(status == 0, MR.triangle_areas(np.nan_to_num(v), np.where(status[:, None] == 0, f, 0)), 0.0)
    share = area / area.sum()
    hist = np.bincount(out["striangle"], minlength=len(f)).astype(np.float64)
    sd = np.sqrt(n * share * (1 - share))
    z = np.abs(hist - n * share) / np.maximum(sd, 1e-300)
    print("histogram over %d triangles, %d draws: largest deviation %.2f standard deviations" % ((share > 0).sum(), n, z[share > 0].max()))
    assert (hist[share == 0] == 0).all() and (z[share > 0] <= 5).all()


# ---- against the extraction on the device, and end to end ------------------------------------------------------------------------------------------

def test_lattice_sphere_from_the_device_extraction_stays_within_the_derived_bound():
    e, h = lattice_bound()
    (m,) = M.mesh_from_sdf(up(MR.shape_sdf("sphere", 16)))
    p = up(np.random.default_rng(3).uniform(-1, 1, (4000, 3)).astype(np.float32))
    syncs, res = count_syncs(lambda: S.mesh_sdf_many([m], [p], return_nearest=True, return_winding=True))
    sdf = res.sdf.cpu().numpy().astype(np.float64)
    r = np.linalg.norm(p.cpu().numpy().astype(np.float64), axis=1)
    err = np.abs(sdf - (r - 0.6)).max()
    far = np.abs(r - 0.6) > e + 1e-6
    print("device sphere R = 16: %d triangles, max | sdf - (|p| - 0.6) | = %.4f = %.2f h^2, bound e = %.4f; %d host syncs"
          % (len(m), err, err / h ** 2, e, syncs))
    assert syncs == 0 and err <= e + 1e-6 and far.sum() > 3000 and np.array_equal(sdf[far] < 0, r[far] < 0.6)
    assert int(res.flags.cpu()[0]) == 0 and res.nearest.min() >= 0 and res.nearest.max() < len(m)
    assert torch.equal(m.signed_distance(p), res.sdf)
    # the camera-frame mesh is wound the other way round: the same distances and signs, up to the rigid motion's rounding
    m.scale, m.cam_T = 1.0, np.diag([1.0, -1.0, 1.0, 1.0])
    cam = m.to_camera()
    q = p * torch.tensor([1.0, -1.0, 1.0], device=DEV)
    assert torch.allclose(cam.signed_distance(q), res.sdf, rtol=0, atol=1e-6)           # (the edges are walked in another order: float32 rounding)


def test_draw_sdf_samples_end_to_end(tmp_path):
    dec = sdflabel_amd.setup_dsdf(ASSET + ".pt", precision=torch.float32)[0].to(DEV)
    (m,) = M.meshes_many(dec, [torch.tensor(GT_LATENT)], resolution=24)
    n = 6000
    g = torch.Generator().manual_seed(11)
    syncs, (s,) = count_syncs(lambda: S.draw_sdf_samples([m], n=n, generator=g))
    assert syncs == 0 and len(s) == n and s.counts == (2820, 2820, 360) and s.rows.is_cuda and s.rows.shape == (n, 4)
    path = str(tmp_path / "box.npz")
    syncs_save, _ = count_syncs(lambda: s.save(path))
    rows = s.numpy()
    print("draw_sdf_samples: %d samples, %d host syncs while drawing, %d in save; %d inside, flags %d"
          % (n, syncs, syncs_save, int((rows[:, 3] < 0).sum()), int(s.flags.cpu())))
    assert syncs_save == 1 and int(s.flags.cpu()) == 0 and np.isfinite(rows).all()
    back = S.SdfSamples.load(path)
    assert len(back) == n and np.array_equal(np.sort(back.numpy()[:, 3]), np.sort(rows[:, 3]))
    # the near-surface rows are near the surface, by their widths; the uniform rows fill the cube
    d = np.abs(rows[:, 3])
    sa, sb = 0.005 ** 0.5, 0.0005 ** 0.5
    assert d[:2820].max() <= 6 * sa * 3 ** 0.5 and d[2820:5640].max() <= 6 * sb * 3 ** 0.5 and np.median(d[:2820]) > np.median(d[2820:5640])
    assert np.abs(rows[5640:, :3]).max() <= 1.0 and np.abs(rows[5640:, :3]).max() > 0.9
    # the same generator state gives the same rows
    (s2,) = S.draw_sdf_samples([m], n=n, generator=torch.Generator().manual_seed(11))
    assert torch.equal(s2.rows, s.rows)
    # the prior explains its own shape better than the antipodal latent does: two measured values, compared with each other
    lat = torch.tensor(GT_LATENT)
    own, own_sign = S.prior_residuals(dec, lat[None], [s])
    anti, anti_sign = S.prior_residuals(dec, -lat[None], [s])
    print("prior_residuals: own latent L1 %.5f sign agreement %.4f; antipodal latent L1 %.5f sign agreement %.4f"
          % (float(own), float(own_sign), float(anti), float(anti_sign)))
    assert float(own) < float(anti)


def test_mesh_to_sdf_tool_turns_a_saved_ply_into_samples(tmp_path, capsys):
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("mesh_to_sdf", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                                             "tools", "mesh_to_sdf.py"))
    mesh_to_sdf = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mesh_to_sdf)
    v, f = C.icosphere(2, 2.5)
    M.Mesh(up(v + np.float32(4.0)), up(f)).save(str(tmp_path / "ball.ply"))
    mesh_to_sdf.main(["--out", str(tmp_path / "out"), "--n", "3000", "--seed", "4", str(tmp_path / "ball.ply")])
    back = S.SdfSamples.load(str(tmp_path / "out" / "ball.npz"))
    rows = back.numpy()
    # in the unit-sphere frame the ball has radius 1 / 1.03 around the origin; the mesh's sag is below 0.02 at this subdivision
    r = np.linalg.norm(rows[:, :3].astype(np.float64), axis=1)
    err = np.abs(rows[:, 3] - (r - 1 / 1.03)).max()
    print("mesh_to_sdf: %d rows, %d inside, max | sdf - (|x| - 1 / 1.03) | = %.4f" % (len(rows), int((rows[:, 3] < 0).sum()), err))
    assert len(back) == 3000 and err < 0.02 and 0 < (rows[:, 3] < 0).sum() < 3000 and '"flags": 0' in capsys.readouterr().out
