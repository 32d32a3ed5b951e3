"""Verification on the device (csrc/verify.hip, sdflabel_amd/verify.py) against the numpy restatement tests/_verify_ref.py: masks, depth
bits, triangle indices, flags, rows and counts must be EQUAL -- both sides do the same float64 operations in the same order.  Every figure
is printed before it is asserted."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

import sdflabel_amd
from sdflabel_amd import _lib
from sdflabel_amd import mesh as M
from sdflabel_amd import verify as V
from sdflabel_amd.fixtures import ASSET, ASSET_ELLIPSOID, ASSET_ELLIPSOID_LN, GT_LATENT
from tests import _mesh_ref as MR
from tests import _verify_cases as VC
from tests import _verify_ref as VR

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
    return VC.cases()


@pytest.fixture(scope="module")
def refs(cases):
    """name -> (mask, depth, triangle, flags) of the restatement; computed once, never modified"""
    return {n: VR.raster(v, f, K, w, z) for n, (v, f, K, w, z) in cases.items()}


def cam_mesh(v, f):
    return M.Mesh(torch.from_numpy(np.ascontiguousarray(v, np.float32)).to(DEV), torch.from_numpy(np.ascontiguousarray(f, np.int32)).to(DEV),
                  frame="camera")


def raw_raster(meshes, K, wins, z_min=0.1):
    """sdfr_mesh_raster on outputs that sit between guard rows; returns per mesh (mask, depth, triangle, flags) after checking the guards"""
    L = _lib.lib()
    B = len(meshes)
    wins = np.asarray(wins, np.int32).reshape(-1, 4)
    voff = np.concatenate([[0], np.cumsum([len(v) for v, _ in meshes])]).astype(np.int64)
    toff = np.concatenate([[0], np.cumsum([len(f) for _, f in meshes])]).astype(np.int64)
    poff = np.concatenate([[0], np.cumsum((wins[:, 2] - wins[:, 0]).astype(np.int64) * (wins[:, 3] - wins[:, 1]))]).astype(np.int64)
    V_, T, P = int(voff[-1]), int(toff[-1]), int(poff[-1])
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    verts = up(np.concatenate([v for v, _ in meshes]).astype(np.float32).reshape(-1, 3))
    faces = up(np.concatenate([f for _, f in meshes]).astype(np.int32).reshape(-1, 3))
    d_voff, d_toff, d_poff, d_win = up(voff), up(toff), up(poff), up(wins)
    keys = torch.full((P + 2 * GUARD,), 0x1234, dtype=torch.int64, device=DEV)
    mask = torch.full((P + 2 * GUARD,), 0xAB, dtype=torch.uint8, device=DEV)
    depth = torch.full((P + 2 * GUARD,), 7.0, dtype=torch.float32, device=DEV)
    tri = torch.full((P + 2 * GUARD,), -5, dtype=torch.int32, device=DEV)
    flags = torch.full((B + 2 * GUARD,), 99, dtype=torch.int32, device=DEV)
    k4 = (ctypes.c_double * 4)(*K)
    Pt = _lib.ptr
    _lib.check(L.sdfr_mesh_raster(Pt(verts), V_, Pt(faces), T, Pt(d_voff), Pt(d_toff), Pt(d_win), Pt(d_poff), P, B, VC.W, VC.H, k4, z_min,
                                  Pt(keys[GUARD:]), Pt(mask[GUARD:]), Pt(depth[GUARD:]), Pt(tri[GUARD:]), Pt(flags[GUARD:]), _lib.stream_ptr()),
               "sdfr_mesh_raster")
    torch.cuda.synchronize()
    for t, fill in ((keys, 0x1234), (mask, 0xAB), (depth, 7.0), (tri, -5), (flags, 99)):
        n = t.shape[0] - 2 * GUARD
        assert (t[:GUARD] == fill).all() and (t[GUARD + n:] == fill).all(), "a guard row was written"
    mask, depth, tri, flags = (t[GUARD:t.shape[0] - GUARD].cpu().numpy() for t in (mask, depth, tri, flags))
    out = []
    for b in range(B):
        shape = (int(wins[b, 3] - wins[b, 1]), int(wins[b, 2] - wins[b, 0]))
        s = slice(int(poff[b]), int(poff[b + 1]))
        out.append((mask[s].reshape(shape), depth[s].reshape(shape), tri[s].reshape(shape), int(flags[b])))
    return out


def same(got, want, name=""):
    assert got[0].shape == want[0].shape, (name, got[0].shape, want[0].shape)
    print("%s: %d covered pixels (restatement %d), flags %d (%d)" % (name, int(got[0].sum()), int(want[0].sum()), got[3], want[3]))
    assert got[0].dtype == np.uint8 and got[0].tobytes() == want[0].tobytes(), name
    assert got[1].dtype == np.float32 and got[1].tobytes() == want[1].tobytes(), name
    assert got[2].dtype == np.int32 and got[2].tobytes() == want[2].tobytes(), name
    assert got[3] == want[3], name


def host(r):
    return r.mask.cpu().numpy(), r.depth.cpu().numpy(), r.triangle.cpu().numpy(), int(r.flags.cpu())


# ---- the rasteriser ----------------------------------------------------------------------------------------------------------------------------

CASES = ["edges_through_samples", "edges_through_samples_z2", "shared_edge", "coplanar_overlap", "near_over_far", "partly_outside_window",
         "partly_outside_image", "zero_area", "behind_z_min", "nan_vertex", "bad_index", "empty_mesh", "empty_window", "full_window", "cube"]


@pytest.mark.parametrize("name", CASES)
def test_raster_equals_the_restatement(cases, refs, name):
    """every case alone, its outputs between guard rows.  full_window: one triangle over 48 x 32 pixels, the wave's path; nan_vertex holds
    NaN and infinite vertices and triangles whose projections lie 10^39 pixels outside the image"""
    v, f, K, w, z = cases[name]
    (got,) = raw_raster([(v, f)], K, [w], z)
    same(got, refs[name], name)
    if name == "behind_z_min":
        assert got[3] == V.FLAG_BEHIND
    if name == "shared_edge":
        assert got[2][15, 10:21].tolist() == [1] * 5 + [0] * 6 and got[2][16, 15] == 1            # the diagonal pixel (15, 15) goes to index 0


def test_raster_marching_tetrahedra_sphere():
    """2-5 k triangles of a few pixels each: the lane-per-triangle path, many triangles meeting in every pixel"""
    from sdflabel_amd.frame import assemble_labels
    (m,) = M.mesh_from_sdf(torch.from_numpy(MR.shape_sdf("sphere", 24)).to(DEV))
    _, cam_T = assemble_labels(np.zeros((1, 6), np.float32), np.array([0.7], np.float32), np.array([[0.05, -0.02, 3.0]], np.float32),
                               np.array([1.7], np.float32), np.eye(4), [None])
    m.scale, m.cam_T = 1.7, cam_T[0]
    c = m.to_camera()
    win = (3, 1, 62, 47)
    (r,) = V.raster_many([c], VC.K_SPHERE, [win], (VC.W, VC.H))
    want = VR.raster(c.vertices_numpy(), c.faces_numpy(), VC.K_SPHERE, win)
    print("sphere R = 24: %d triangles, %d distinct winners" % (len(c), len(np.unique(want[2][want[0] != 0]))))
    assert 2000 <= len(c) <= 6000
    same(host(r), want, "sphere24")


def test_ragged_batch_equals_solo_and_other_order(cases, refs):
    names = ["near_over_far", "partly_outside_window", "full_window", "empty_mesh", "nan_vertex"]
    meshes = [cam_mesh(cases[n][0], cases[n][1]) for n in names]
    wins = [cases[n][3] for n in names]
    syncs, a = count_syncs(lambda: V.raster_many(meshes, VC.K8, wins, (VC.W, VC.H)))
    assert syncs == 0, syncs
    order = [3, 2, 4, 0, 1]
    b = V.raster_many([meshes[i] for i in order], VC.K8, [wins[i] for i in order], (VC.W, VC.H))
    for i, n in enumerate(names):
        assert a[i].window == tuple(wins[i]) and a[i].mask.shape == refs[n][0].shape
        same(host(a[i]), refs[n], n)
        (solo,) = V.raster_many([meshes[i]], VC.K8, [wins[i]], (VC.W, VC.H))
        j = order.index(i)
        for x in (solo, b[j]):
            assert torch.equal(x.mask, a[i].mask) and torch.equal(x.depth.view(torch.int32), a[i].depth.view(torch.int32))
            assert torch.equal(x.triangle, a[i].triangle) and torch.equal(x.flags, a[i].flags)


def test_two_runs_give_the_same_bits(cases):
    v, f, K, w, z = cases["sphere24"]
    m = cam_mesh(v, f)
    (a,), (b,) = V.raster_many([m], K, [w], (VC.W, VC.H)), V.raster_many([m], K, [w], (VC.W, VC.H))
    assert torch.equal(a.mask, b.mask) and torch.equal(a.depth.view(torch.int32), b.depth.view(torch.int32)) and torch.equal(a.triangle, b.triangle)
    assert int(a.mask.sum()) > 500


def test_raster_many_refusals(cases):
    v, f, K, w, z = cases["edges_through_samples"]
    m = cam_mesh(v, f)
    with pytest.raises(ValueError):
        V.raster_many([M.Mesh(m.vertices, m.faces)], K, [w], (VC.W, VC.H))                  # lattice frame
    with pytest.raises(ValueError):
        V.raster_many([m], K, [(0, 0, VC.W + 1, VC.H)], (VC.W, VC.H))                       # not clipped to the image
    with pytest.raises(ValueError):
        V.raster_many([m], K, [w, w], (VC.W, VC.H))
    assert V.raster_many([], K, [], (VC.W, VC.H)) == []


# ---- the counts of the projective test ------------------------------------------------------------------------------------------------------------

def test_mask_counts_equal_numpy(cases, refs):
    names = ["edges_through_samples", "near_over_far", "partly_outside_window", "empty_mesh", "empty_window", "full_window"]
    meshes = [cam_mesh(cases[n][0], cases[n][1]) for n in names]
    wins = np.asarray([cases[n][3] for n in names])
    rb = V.raster_batch(meshes, VC.K8, wins, (VC.W, VC.H), 0.1)
    rng = np.random.default_rng(9)
    labels = [(rng.random(refs[n][0].shape) < 0.4).astype(np.uint8) for n in names]
    packed = torch.from_numpy(np.concatenate([l.reshape(-1) for l in labels])).to(DEV)
    plain, with_label = rb.mask_counts().cpu().numpy(), rb.mask_counts(packed).cpu().numpy()
    for b, n in enumerate(names):
        print(n, plain[b].tolist(), with_label[b].tolist())
        assert plain[b].tolist() == VR.mask_counts(refs[n][0], wins[b]).tolist(), n
        assert with_label[b].tolist() == VR.mask_counts(refs[n][0], wins[b], labels[b]).tolist(), n
    assert with_label[1, 6] > 0 and plain[3].tolist() == [0] * 8


# ---- the points of the geometric test -------------------------------------------------------------------------------------------------------------

BAND = 0.2
PARAMS = {"latent": torch.tensor(GT_LATENT), "scale": torch.tensor([2.0]), "yaw": torch.tensor([0.6]), "trans": torch.tensor([0.1, 0.0, 3.5])}


@pytest.fixture(scope="module")
def ell():
    """the ellipsoid decoder, its polished mesh in both frames; computed once, never modified"""
    dec = sdflabel_amd.setup_dsdf(ASSET_ELLIPSOID + ".pt", precision=torch.float32)[0].to(DEV)
    (m,) = M.meshes_many(dec, [PARAMS], resolution=20)
    return dec, m, m.to_camera()


def restated_counts(details, band):
    pose = details["pose"].cpu().numpy()
    return VR.band_counts(details["sdf"].cpu().numpy(), details["in_cube"].cpu().numpy(), details["ptoff"], pose, band)


def test_point_rows_equal_the_restatement(ell):
    dec = ell[0]
    points, ptoff, poses, lat, _, _ = VC.point_problem()
    params = [{"latent": lat[b], "scale": poses[b][5:6], "yaw": np.float32([y]), "trans": poses[b][2:5]} for b, y in enumerate((0.7, -2.0, 3.0))]
    clouds = [points[ptoff[b]:ptoff[b + 1]] for b in range(3)]
    counts, d = V.band_counts(dec, params, clouds, band=BAND, return_details=True)
    pose = d["pose"].cpu().numpy()
    assert pose[:, 2:].tobytes() == np.ascontiguousarray(poses[:, 2:]).tobytes()
    # host parameters: the cosine and sine are torch's float32 values on the CPU, the ones frame.assemble_labels puts into cam_T
    y32 = torch.tensor([0.7, -2.0, 3.0], dtype=torch.float32)
    assert pose[:, 0].tobytes() == torch.cos(y32).numpy().tobytes() and pose[:, 1].tobytes() == torch.sin(y32).numpy().tobytes()
    rows, inside = VR.point_rows(points, ptoff, pose, lat)
    assert d["rows"].cpu().numpy().tobytes() == rows.tobytes() and d["in_cube"].cpu().numpy().tobytes() == inside.tobytes()
    assert 0 < inside.sum() < len(inside)
    want = restated_counts(d, BAND)
    print("counts", counts.cpu().numpy().tolist(), "restatement", want.tolist())
    assert counts.cpu().numpy().tolist() == want.tolist() and want[:, 0].tolist() == [300, 0, 150]
    # chunked staging gives the same rows and counts
    small = 128 * 4 * (lat.shape[1] + 3)
    counts2, d2 = V.band_counts(dec, params, clouds, band=BAND, staging_bytes=small, return_details=True)
    assert torch.equal(counts2, counts) and torch.equal(d2["rows"].view(torch.int32), d["rows"].view(torch.int32))       # (bits: a row is NaN)
    assert torch.equal(d2["sdf"].view(torch.int32), d["sdf"].view(torch.int32))


def test_point_rows_invert_the_camera_frame(ell):
    dec, m, cam = ell
    _, d = V.band_counts(dec, [PARAMS], [cam.vertices], band=BAND, return_details=True)
    L = len(GT_LATENT)
    back = d["rows"][:, L:].cpu().numpy().astype(np.float64)
    bound = VR.roundtrip_bound(float(PARAMS["scale"]), PARAMS["trans"].numpy())
    err = np.abs(back - m.vertices_numpy()).max()
    print("lattice -> camera -> lattice over %d vertices: max error %.3g, bound %.3g" % (len(back), err, bound))
    assert err < bound
    assert torch.equal(d["rows"][:, :L], torch.tensor(GT_LATENT, device=DEV).expand(len(back), L))           # the latent goes in raw


def test_band_counts_on_the_ellipsoid(ell):
    dec, m, cam = ell
    n = int(cam.vertices.shape[0])
    scale = float(PARAMS["scale"])
    on = cam.vertices
    off = cam.vertices + 3 * BAND * cam.normals
    away = cam.vertices + torch.tensor([3.0 * scale, 0.0, 0.0], device=DEV)
    counts, d = V.band_counts(dec, [PARAMS] * 3, [on, off, away], band=BAND, return_details=True)
    c = counts.cpu().numpy()
    print("%d points per cloud; counts on the surface %s, 3 bands off %s, outside the cube %s" % (n, c[0].tolist(), c[1].tolist(), c[2].tolist()))
    assert 1000 <= n <= 2500
    assert c.tolist() == restated_counts(d, BAND).tolist()
    assert c[0].tolist() == [n, n, n]                                   # polished vertices: all in the band
    assert c[1, 0] == n and c[1, 2] == 0                               # pushed three bands along the normals: none
    assert c[2].tolist() == [n, 0, 0]                                   # outside the cube: none, whatever the decoder says there
    assert V.band_counts(dec, [], []).shape == (0, 3)
    empty = V.band_counts(dec, [PARAMS], [torch.zeros((0, 3), device=DEV)]).cpu().numpy()
    assert empty.tolist() == [[0, 0, 0]]


@pytest.mark.parametrize("asset,precision", [(ASSET_ELLIPSOID, torch.float16), (ASSET_ELLIPSOID_LN, torch.float32)], ids=["float16", "layernorm"])
def test_band_counts_other_decoders(ell, asset, precision):
    cam = ell[2]
    dec = sdflabel_amd.setup_dsdf(asset + ".pt", precision=precision)[0].to(DEV)
    pts = cam.vertices + 0.5 * BAND * cam.normals * torch.linspace(-2, 2, cam.vertices.shape[0], device=DEV)[:, None]
    counts, d = V.band_counts(dec, [PARAMS], [pts], band=BAND, return_details=True)
    c = counts.cpu().numpy()
    print("counts", c.tolist())
    assert c.tolist() == restated_counts(d, BAND).tolist() and 0 < c[0, 2] <= c[0, 1] <= c[0, 0]
    assert np.isfinite(d["sdf"].cpu().numpy()).all()


# ---- the verdict -------------------------------------------------------------------------------------------------------------------------------

K_ELL = np.array([[60.0, 0, 32.0], [0, 60.0, 24.0], [0, 0, 1]])


def projected_box(cam):
    v = cam.vertices_numpy()
    u, w = VR.project(60.0, 32.0, v[:, 0], v[:, 2]), VR.project(60.0, 24.0, v[:, 1], v[:, 2])
    return [int(np.floor(u.min())), int(np.floor(w.min())), int(np.ceil(u.max())), int(np.ceil(w.max()))]


def test_verify_many_accepts_the_shape_and_rejects_it_moved(ell):
    dec, m, cam = ell
    box = projected_box(cam)
    w, h = box[2] - box[0], box[3] - box[1]
    v = cam.vertices_numpy()
    extent = float(v[:, 0].max() - v[:, 0].min())
    scale = float(PARAMS["scale"])
    moved_p = dict(PARAMS, trans=PARAMS["trans"] + torch.tensor([(1.05 * extent + BAND) / scale, 0.0, 0.0]))
    (mm,) = M.meshes_many(dec, [moved_p], resolution=20)
    moved = mm.to_camera()
    args = ([PARAMS, moved_p], [cam, moved], [cam.vertices, cam.vertices], K_ELL, [box, box], (VC.W, VC.H))
    V.verify_many(dec, *args)                                           # (the decoder's handle is built outside the counted call)
    syncs, (good, bad) = count_syncs(lambda: V.verify_many(dec, *args, band=BAND))
    print("label box %s (%d x %d), good %s" % (box, w, h, good))
    print("moved %s" % bad)
    assert syncs == 1, syncs
    assert good["iou_box"] >= (w - 2) * (h - 2) / float(w * h)
    assert good["n_pts"] == good["n_band"] == len(v) and good["share"] == 1.0 and good["iou_mask"] is None and good["flags"] == 0
    assert good["ok"] and good["why"] == []
    assert bad["n_band"] == 0 and bad["iou_box"] < good["iou_box"] and not bad["ok"] and {"iou", "share"} <= set(bad["why"])
    # the figures are the restatement's
    rm = VR.raster(cam.vertices_numpy(), cam.faces_numpy(), (60.0, 60.0, 32.0, 24.0), good["window"])
    c = VR.mask_counts(rm[0], good["window"])
    assert good["area"] == c[0] and good["mask_box"] == c[1:5].tolist()
    # a label mask: the rendered mask itself gives IoU 1, and the verdict can use it
    lab = torch.from_numpy(rm[0]).to(DEV)
    (one,) = V.verify_many(dec, [PARAMS], [cam], [cam.vertices], K_ELL, [box], (VC.W, VC.H), label_masks=[lab], iou="mask")
    assert one["iou_mask"] == 1.0 and one["ok"]
    l, t, r, b = good["window"]
    boxed = lab[box[1] - t:box[3] - t, box[0] - l:box[2] - l].contiguous()                 # of the label box's shape: placed into the window
    (two,) = V.verify_many(dec, [PARAMS], [cam], [cam.vertices], K_ELL, [box], (VC.W, VC.H), label_masks=[boxed])
    inter = int(boxed.sum())
    print("label mask of the box's shape: iou_mask %.4f" % two["iou_mask"])
    assert two["iou_mask"] == inter / float(c[0]) and two["ok"]
    (none,) = V.verify_many(dec, [PARAMS], [cam], [torch.zeros((0, 3), device=DEV)], K_ELL, [box], (VC.W, VC.H))
    assert not none["ok"] and "no_points" in none["why"] and none["share"] == 0.0
    with pytest.raises(ValueError):
        V.verify_many(dec, [PARAMS], [cam], [cam.vertices], K_ELL, [box], (VC.W, VC.H), iou="mask")


def test_verify_many_with_a_raster_batch_gives_the_same_verdicts(ell):
    """raster= skips the rasterisation and nothing else: equal dicts, still one host read; also with an empty window and an empty mesh"""
    dec, m, cam = ell
    box = projected_box(cam)
    none = cam_mesh(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    meshes, boxes = [cam, cam, none], [box, [10, 10, 10, 20], box]
    lab = [None, None, torch.ones((box[3] - box[1], box[2] - box[0]), dtype=torch.uint8, device=DEV)]
    args = ([PARAMS] * 3, meshes, [cam.vertices] * 3, K_ELL, boxes, (VC.W, VC.H))
    want = V.verify_many(dec, *args, label_masks=lab)
    rb = V.raster_batch(meshes, K_ELL, V.label_windows(boxes, (VC.W, VC.H), 0.25)[1], (VC.W, VC.H))
    syncs, got = count_syncs(lambda: V.verify_many(dec, *args, label_masks=lab, raster=rb))
    print(got)
    assert syncs == 1, syncs
    assert got == want
    assert got[0]["ok"] and got[1]["window"][0] == got[1]["window"][2] and got[1]["area"] == 0 and got[2]["area"] == 0 and got[2]["flags"] == 0


# ---- the frame pipeline --------------------------------------------------------------------------------------------------------------------------

def test_refine_frame_verify():
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
    with pytest.raises(ValueError):
        refine_frame(annos, dec16, grid, latents, K_orig, p_WC, 3, W8, seed=7, verify=True)
    OP.clear_refiner_cache()
    est0, kept0 = refine_frame(annos, dec16, grid, latents, K_orig, p_WC, 3, W8, seed=7)
    OP.clear_refiner_cache()
    est, kept, st = refine_frame(annos, dec16, grid, latents, K_orig, p_WC, 3, W8, seed=7, return_stages=True, mesh_resolution=16, verify=True)
    assert kept == kept0 and len(kept) >= 2
    for k in est0:
        assert (est[k] == est0[k]) if k == "name" else (est[k].dtype == est0[k].dtype and est[k].tobytes() == est0[k].tobytes()), k
    assert len(st["verify"]) == len(kept) == len(st["meshes"])
    for i, r in zip(kept, st["verify"]):
        print(i, r)
        assert r["n_pts"] == int(st["lidar"][i][0].shape[0])
        assert all(np.isfinite(r[k]) for k in ("iou_box", "share", "area", "n_pts", "n_cube", "n_band", "flags")) and r["iou_mask"] is None
        assert len(r["mask_box"]) == 4 and isinstance(r["ok"], bool) and isinstance(r["why"], list)
        assert 0.0 <= r["iou_box"] <= 1.0 and 0.0 <= r["share"] <= 1.0 and r["n_band"] <= r["n_cube"] <= r["n_pts"]


def test_refine_sample_verify_with_detector_masks():
    """label_type='maskrcnn': the matched detector masks become the label masks, placed into each window; the frame itself is unchanged"""
    from sdflabel_amd.fixtures import stand_in_css, synthetic_sample
    from sdflabel_amd.pipelines import optimizer as OP
    from sdflabel_amd.pipelines import refinement as rtools
    from sdflabel_amd.pipelines.frame import refine_sample
    dec32 = sdflabel_amd.setup_dsdf(ASSET + ".pt", precision=torch.float32)[0].to(DEV)
    dec16 = sdflabel_amd.setup_dsdf(ASSET + ".pt", precision=torch.float16)[0].to(DEV)
    smp, lidar = synthetic_sample(dec32, 40, 32, DEV)
    net = stand_in_css().to(DEV)
    grid = sdflabel_amd.Grid3D(40, DEV)
    W8, iters = {"2d": 0.3, "3d": 0.5}, 3
    annos = rtools.get_annos("", smp)
    H, W = smp["image"].shape[:2]
    rng = np.random.default_rng(3)
    det = np.stack([a["bbox"] + rng.uniform(0.0, 2.9, 4) * [1, 1, -1, -1] for a in annos]).astype(np.float32)
    masks = []
    for l, t, r, b in det.astype(np.int64):
        m = torch.ones((b - t, r - l), dtype=torch.bool)
        m[: (b - t) // 6] = False
        masks.append(m)
    labels = {"bboxes": torch.from_numpy(det), "masks": masks}
    common = dict(label_type="maskrcnn", maskrcnn_labels=labels, lidar=lidar, seed=7)
    with pytest.raises(ValueError):
        refine_sample(smp, net, dec16, grid, iters, W8, verify=True, **common)
    OP.clear_refiner_cache()
    est0, kept0, _ = refine_sample(smp, net, dec16, grid, iters, W8, **common)
    OP.clear_refiner_cache()
    est, kept, _, st = refine_sample(smp, net, dec16, grid, iters, W8, return_stages=True, mesh_resolution=16, verify={"margin": 0.5}, **common)
    assert kept == kept0 and len(kept) >= 1
    for k in est0:
        assert (est[k] == est0[k]) if k == "name" else est[k].tobytes() == est0[k].tobytes(), k
    assert len(st["verify"]) == len(kept) == len(st["meshes"])
    best = st["match"]["best"].cpu().numpy()
    for i, r, m in zip(kept, st["verify"], st["meshes"]):
        print(i, r)
        l, t, rr, b = r["window"]
        bl, bt, br, bb = st["boxes"][i]
        assert 0 <= l <= bl and 0 <= t <= bt and br <= rr <= W and bb <= b <= H
        (ras,) = V.raster_many([m], smp["orig_cam"], [r["window"]], (W, H))
        lab = torch.zeros((b - t, rr - l), dtype=torch.bool)
        lab[bt - t:bb - t, bl - l:br - l] = masks[int(best[i])]
        got = ras.mask.cpu().bool()
        union = int((got | lab).sum())
        want = float(int((got & lab).sum())) / float(union) if union else 0.0
        assert r["iou_mask"] == want and r["area"] == int(got.sum()) and 0.0 <= r["iou_box"] <= 1.0
