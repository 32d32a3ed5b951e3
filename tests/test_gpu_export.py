"""The training-crop export on the device (csrc/crops.hip, sdflabel_amd/export.py) against the numpy restatement tests/_export_ref.py:
owners, NOCS bytes, RGB bytes, flags and counts must be EQUAL -- both sides do the same float64 operations in the same order.  Every
figure is printed before it is asserted."""
import ctypes

import numpy as np
import pytest
import torch

import sdflabel_amd
from sdflabel_amd import _lib
from sdflabel_amd import export as E
from sdflabel_amd import mesh as M
from sdflabel_amd import verify as V
from sdflabel_amd.fixtures import ASSET
from tests import _export_cases as EC
from tests import _export_ref as ER
from tests import _mesh_ref as MR
from tests import _verify_cases as VC
from tests import _verify_ref as VR
from tests.test_gpu_verify import cam_mesh, count_syncs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 256


def restate(b):
    return ER.export(b["meshes"], b["attrs"], b["K"], b["windows"], b["boxes"], 0.1, b["occlusion"], b["colors"], b["triangles"])


@pytest.fixture(scope="module")
def batches():
    return EC.batches()


@pytest.fixture(scope="module")
def refs(batches):
    """name -> the restatement's result per annotation; computed once, never modified"""
    return {n: restate(b) for n, b in batches.items()}


def guarded(n, dtype, fill):
    return torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)


def inner(t):
    n = t.shape[0] - 2 * GUARD
    return t[GUARD:GUARD + n]


def raw_export(b, qoff=None):
    """sdfr_mesh_raster, then sdfr_crop_owner / sdfr_crop_export / sdfr_crop_counts on outputs that sit between guard rows.  qoff: an offset
    table to pass in place of the boxes' own.  Returns per annotation a dict (owner, uvw, rgb, counts, flag) after checking the guards."""
    L = _lib.lib()
    B = len(b["meshes"])
    wins = np.asarray(b["windows"], np.int32).reshape(-1, 4)
    boxes = np.asarray(b["boxes"], np.int32).reshape(-1, 4)
    voff = np.concatenate([[0], np.cumsum([len(v) for v, _ in b["meshes"]])]).astype(np.int64)
    toff = np.concatenate([[0], np.cumsum([len(f) for _, f in b["meshes"]])]).astype(np.int64)
    poff = np.concatenate([[0], np.cumsum((wins[:, 2] - wins[:, 0]).astype(np.int64) * (wins[:, 3] - wins[:, 1]))]).astype(np.int64)
    own_q = np.concatenate([[0], np.cumsum((boxes[:, 2] - boxes[:, 0]).astype(np.int64) * (boxes[:, 3] - boxes[:, 1]))]).astype(np.int64)
    V_, T, P, Q = int(voff[-1]), int(toff[-1]), int(poff[-1]), int(own_q[-1])
    assert Q <= P                                             # what the entry points require; the buffers below have exactly these sizes
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    verts = up(np.concatenate([v for v, _ in b["meshes"]]).astype(np.float32).reshape(-1, 3))
    faces = up(np.concatenate([f for _, f in b["meshes"]]).astype(np.int32).reshape(-1, 3))
    attrs = up(np.concatenate(b["attrs"]).astype(np.float32).reshape(-1, 3))
    d_voff, d_toff, d_poff, d_win, d_box = up(voff), up(toff), up(poff), up(wins), up(boxes)
    d_qoff = up(own_q if qoff is None else np.asarray(qoff, np.int64))
    keys = torch.empty((P,), dtype=torch.int64, device=DEV)
    mask = torch.empty((P,), dtype=torch.uint8, device=DEV)
    depth = torch.empty((P,), dtype=torch.float32, device=DEV)
    tri = torch.empty((P,), dtype=torch.int32, device=DEV)
    rflags = torch.empty((B,), dtype=torch.int32, device=DEV)
    k4 = (ctypes.c_double * 4)(*b["K"])
    Pt, st = _lib.ptr, _lib.stream_ptr()
    _lib.check(L.sdfr_mesh_raster(Pt(verts) if V_ else None, V_, Pt(faces) if T else None, T, Pt(d_voff), Pt(d_toff), Pt(d_win), Pt(d_poff), P, B,
                                  VC.W, VC.H, k4, 0.1, Pt(keys) if P else None, Pt(mask) if P else None, Pt(depth) if P else None,
                                  Pt(tri) if P else None, Pt(rflags), st), "sdfr_mesh_raster")
    if b["triangles"] is not None:
        host = tri.cpu().numpy().copy()
        for i, t in enumerate(b["triangles"]):
            if t is not None:
                host[int(poff[i]):int(poff[i + 1])] = np.asarray(t, np.int32).reshape(-1)
        tri = up(host)
    colors = None if b["colors"] is None else up(np.concatenate([np.asarray(c, np.float32).reshape(-1, 3) for c in b["colors"]]))
    owner = guarded(P, torch.int32, -7) if b["occlusion"] else None
    uvw, rgb = guarded(3 * Q, torch.uint8, 0xAB), (guarded(3 * Q, torch.uint8, 0xCD) if colors is not None else None)
    flags, counts = guarded(B, torch.int32, 99), guarded(4 * B, torch.int32, -5)
    d_owner = None if owner is None or P == 0 else Pt(inner(owner))
    if b["occlusion"]:
        _lib.check(L.sdfr_crop_owner(Pt(mask) if P else None, Pt(depth) if P else None, Pt(d_win), Pt(d_poff), P, B, VC.W, VC.H, d_owner, st),
                   "sdfr_crop_owner")
    _lib.check(L.sdfr_crop_export(Pt(verts) if V_ else None, V_, Pt(faces) if T else None, T, Pt(attrs) if V_ else None, Pt(d_voff), Pt(d_toff),
                                  Pt(d_win), Pt(d_poff), P, Pt(tri) if P else None, d_owner, Pt(d_box), Pt(d_qoff), Q,
                                  Pt(colors) if (colors is not None and Q) else None, B, VC.W, VC.H, k4, 0.1, Pt(inner(uvw)) if Q else None,
                                  Pt(inner(rgb)) if (rgb is not None and Q) else None, Pt(inner(flags)), st), "sdfr_crop_export")
    _lib.check(L.sdfr_crop_counts(Pt(mask) if P else None, d_owner, Pt(d_win), Pt(d_poff), P, Pt(d_box), Pt(d_qoff), Q, Pt(inner(flags)), B, VC.W,
                                  VC.H, Pt(inner(counts)), st), "sdfr_crop_counts")
    torch.cuda.synchronize()
    for t, fill in ((owner, -7), (uvw, 0xAB), (rgb, 0xCD), (flags, 99), (counts, -5)):
        if t is not None:
            n = t.shape[0] - 2 * GUARD
            assert (t[:GUARD] == fill).all() and (t[GUARD + n:] == fill).all(), "a guard row was written"
    owner_h = None if owner is None else inner(owner).cpu().numpy()
    uvw_h, rgb_h = inner(uvw).cpu().numpy(), (None if rgb is None else inner(rgb).cpu().numpy())
    flags_h, counts_h = inner(flags).cpu().numpy(), inner(counts).cpu().numpy().reshape(B, 4)
    out = []
    for i in range(B):
        ws = (int(wins[i, 3] - wins[i, 1]), int(wins[i, 2] - wins[i, 0]))
        bs = (int(boxes[i, 3] - boxes[i, 1]), int(boxes[i, 2] - boxes[i, 0]), 3)
        q = slice(3 * int(own_q[i]), 3 * int(own_q[i + 1]))
        out.append(dict(owner=None if owner_h is None else owner_h[int(poff[i]):int(poff[i + 1])].reshape(ws), uvw=uvw_h[q].reshape(bs),
                        rgb=None if rgb_h is None else rgb_h[q].reshape(bs), counts=counts_h[i], flag=int(flags_h[i])))
    return out


def same(got, want, name):
    for i, (g, w) in enumerate(zip(got, want)):
        print("%s[%d]: counts %s (restatement %s), %d labelled pixels" % (name, i, g["counts"].tolist(), w["counts"].tolist(),
                                                                           int((g["uvw"].astype(np.int64).sum(-1) > 0).sum())))
        if w["owner"] is not None:
            assert g["owner"].dtype == np.int32 and g["owner"].tobytes() == w["owner"].tobytes(), name
        assert g["uvw"].shape == w["uvw"].shape and g["uvw"].tobytes() == w["uvw"].tobytes(), name
        if w["rgb"] is not None:
            assert g["rgb"].tobytes() == w["rgb"].tobytes(), name
        assert g["counts"].tolist() == w["counts"].tolist() and g["flag"] == w["counts"][3], name


# ---- the kernels -------------------------------------------------------------------------------------------------------------------------------

BATCHES = ["single_triangle", "cube_box_inside_window", "posed_cube", "depth_tie", "near_over_far", "occluder_window_short", "occlusion_off",
           "box_at_the_image_border", "empty_window", "empty_mesh", "nan_vertex", "zero_bytes", "bad_triangle_index", "box_outside_window"]


@pytest.mark.parametrize("name", BATCHES)
def test_export_equals_the_restatement(batches, refs, name):
    """every batch alone, its outputs between guard rows.  The colour crops hold NaN, infinities, negative values and values above 1;
    bad_triangle_index: a triangle image with 7 and -3 for a mesh of one triangle (flag set, zeros written); box_outside_window: the flag,
    zeros, and the annotation beside it untouched"""
    assert set(BATCHES) == set(batches)
    got = raw_export(batches[name])
    same(got, refs[name], name)
    if name in ("bad_triangle_index", "box_outside_window"):
        assert got[0]["flag"] == V.FLAG_INVALID and not got[0]["uvw"].any() and not got[0]["rgb"].any() and got[1]["flag"] == 0
        assert got[1]["uvw"].any()
    if name == "depth_tie":
        assert (got[0]["owner"] <= 0).all() and (got[1]["owner"] == 0).sum() > 50                 # the lower index wins the exact ties


def test_sphere_equals_the_restatement():
    """5 k triangles of a few pixels each, many meeting in every pixel, the lattice vertices as attributes; outputs between guard rows"""
    b = EC.sphere_batch()[0]
    got, want = raw_export(b), restate(b)
    same(got, want, "sphere24")
    assert want[0]["counts"][1] > 1000 and (got[0]["uvw"].astype(np.int64).sum(-1) > 0).sum() == want[0]["counts"][2]


def test_sphere_from_device_meshes():
    """marching tetrahedra on the device, Mesh.to_camera, the lattice vertices riding along as attributes: 2-5 k triangles of a few pixels"""
    from sdflabel_amd.frame import assemble_labels
    (m,) = M.mesh_from_sdf(torch.from_numpy(MR.shape_sdf("sphere", 24)).to(DEV))
    scale, yaw, trans = 1.7, 0.7, (0.05, -0.02, 3.0)
    _, cam_T = assemble_labels(np.zeros((1, 6), np.float32), np.array([yaw], np.float32), np.array([trans], np.float32),
                               np.array([scale], np.float32), np.eye(4), [None])
    m.scale, m.cam_T = scale, cam_T[0]
    c = m.to_camera()
    assert c.lattice_vertices is m.vertices
    (crop,) = E.crops_many([c], VC.K_SPHERE, [VC.FULL], (VC.W, VC.H), margin=0.0)
    assert crop.box == VC.FULL and crop.window == VC.FULL and crop.rgb is None
    b = dict(K=VC.K_SPHERE, meshes=[(c.vertices_numpy(), c.faces_numpy())], attrs=[m.vertices_numpy()], windows=[VC.FULL], boxes=[VC.FULL],
             colors=None, triangles=None, occlusion=True)
    (want,) = restate(b)
    got = crop.uvw.cpu().numpy()
    print("sphere R = 24: %d triangles, counts %s (restatement %s)" % (len(c), crop.counts.cpu().tolist(), want["counts"].tolist()))
    assert got.tobytes() == want["uvw"].tobytes() and crop.counts.cpu().tolist() == want["counts"].tolist() and int(crop.flags.cpu()) == 0
    assert want["counts"][1] > 1000
    # the unprojection identity on the device's bytes
    pose = VR.pose_row(np.cos(np.float32(yaw)), np.sin(np.float32(yaw)), trans, scale)
    err = identity_errors(got, want["mask"], want["depth"], VC.K_SPHERE, VC.FULL, pose)
    bound = 1.0 / 255.0 + ER.shade_bound(scale, trans)
    print("unprojection identity: max error %.9g, bound %.9g" % (err.max(), bound))
    assert err.max() <= bound


def identity_errors(uvw, seen, depth, K, box, pose):
    """|byte / 127.5 - 1 - point_x(pixel unprojected at the raster's depth)| over the pixels `seen` of a crop at `box`"""
    ys, xs = np.nonzero(seen)
    d = depth[ys, xs].astype(np.float64)
    px, py = xs + float(box[0]), ys + float(box[1])
    pc = np.stack([(px - K[2]) / K[0] * d, (py - K[3]) / K[1] * d, d], 1).astype(np.float32)
    x, _ = VR.point_x(pc, pose)
    return np.abs(uvw[ys, xs].astype(np.float64) / 127.5 - 1.0 - x.astype(np.float64))


def test_offset_tables_that_do_not_fit(batches, refs):
    """qoff off by one: both annotations are flagged and every byte is zero; a last offset beyond Q: that annotation alone.  Guards intact."""
    b = batches["near_over_far"]
    want = refs["near_over_far"]
    q = [0, 64 * 48, 64 * 48 + 26 * 24]
    got = raw_export(b, qoff=[0, q[1] - 1, q[2]])
    for g in got:
        print(g["counts"].tolist(), g["flag"])
        assert g["flag"] == V.FLAG_INVALID and g["counts"].tolist() == [0, 0, 0, V.FLAG_INVALID] and not g["uvw"].any() and not g["rgb"].any()
    got = raw_export(b, qoff=[0, q[1], q[2] + 5])
    same(got[:1], want[:1], "first of two")
    assert got[1]["flag"] == V.FLAG_INVALID and not got[1]["uvw"].any() and not got[1]["rgb"].any()
    got = raw_export(b, qoff=[-3, q[1], q[2]])
    assert got[0]["flag"] == V.FLAG_INVALID and not got[0]["uvw"].any()
    same(got[1:], want[1:], "second of two")


# ---- crops_many --------------------------------------------------------------------------------------------------------------------------------

def frame_problem(batches):
    """three annotations with label boxes: one cut by the image border, one small; colours of the label boxes' shapes"""
    c = VC.cases()
    far, near = batches["near_over_far"]["meshes"]
    meshes = [far, near, (c["partly_outside_image"][0], c["partly_outside_image"][1])]
    rng = np.random.default_rng(21)
    attrs = [rng.uniform(-1, 1, (len(v), 3)).astype(np.float32) for v, _ in meshes]
    labels = [[6.3, 5.0, 58.2, 42.5], [20, 10, 40, 30], [-6, -4, 30, 40]]
    colors = [EC.colour_crop(rng, (int(np.floor(l)), int(np.floor(t)), int(np.ceil(r)), int(np.ceil(b)))) for l, t, r, b in labels]
    return meshes, attrs, labels, colors


def on_device(meshes, attrs):
    return [cam_mesh(v, f) for v, f in meshes], [torch.from_numpy(a).to(DEV) for a in attrs]


def run_many(meshes, attrs, labels, colors, **kw):
    dm, da = on_device(meshes, attrs)
    return E.crops_many(dm, VC.K8, labels, (VC.W, VC.H), colors=colors, attributes=da, **kw)


def host(c):
    return c.uvw.cpu().numpy(), (None if c.rgb is None else c.rgb.cpu().numpy()), c.counts.cpu().numpy(), int(c.flags.cpu())


def test_crops_many_equals_the_restatement(batches):
    meshes, attrs, labels, colors = frame_problem(batches)
    lbox, win = V.label_windows(labels, (VC.W, VC.H), 0.25)
    box = np.stack([np.clip(lbox[:, 0], 0, VC.W), np.clip(lbox[:, 1], 0, VC.H), np.clip(lbox[:, 2], 0, VC.W), np.clip(lbox[:, 3], 0, VC.H)], 1)
    assert box[2].tolist() == [0, 0, 30, 40] and lbox[2].tolist() == [-6, -4, 30, 40]          # cut by the image border
    cut = [colors[i][box[i][1] - lbox[i][1]:box[i][3] - lbox[i][1], box[i][0] - lbox[i][0]:box[i][2] - lbox[i][0]] for i in range(3)]
    for occ in (True, False):
        want = ER.export(meshes, attrs, VC.K8, win, box, 0.1, occ, cut)
        dm, da = on_device(meshes, attrs)
        syncs, got = count_syncs(lambda: E.crops_many(dm, VC.K8, labels, (VC.W, VC.H), colors=colors, attributes=da, occlusion=occ))
        assert syncs == 0, syncs
        for i in range(3):
            uvw, rgb, counts, flags = host(got[i])
            print("occlusion %s, annotation %d: box %s, window %s, counts %s" % (occ, i, got[i].box, got[i].window, counts.tolist()))
            assert got[i].box == tuple(box[i]) and got[i].window == tuple(win[i]) and uvw.shape == want[i]["uvw"].shape
            assert uvw.tobytes() == want[i]["uvw"].tobytes() and rgb.tobytes() == want[i]["rgb"].tobytes()
            assert counts.tolist() == want[i]["counts"].tolist() and flags == want[i]["flags"]
        if occ:
            assert want[0]["counts"][2] < want[0]["counts"][1]                                   # the near triangle hides a part of the far one
    # colours of the clipped boxes' shapes, on the host, give the same bytes; without colours there is no rgb
    again = run_many(meshes, attrs, labels, cut)
    plain = run_many(meshes, attrs, labels, None)
    for i in range(3):
        assert torch.equal(again[i].rgb, got[i].rgb) and plain[i].rgb is None


def test_ragged_batch_without_occlusion_equals_solo_and_other_order(batches):
    meshes, attrs, labels, colors = frame_problem(batches)
    a = run_many(meshes, attrs, labels, colors, occlusion=False)
    order = [2, 0, 1]
    b = run_many([meshes[i] for i in order], [attrs[i] for i in order], [labels[i] for i in order], [colors[i] for i in order], occlusion=False)
    for i in range(3):
        (solo,) = run_many(meshes[i:i + 1], attrs[i:i + 1], labels[i:i + 1], colors[i:i + 1], occlusion=False)
        for x in (solo, b[order.index(i)]):
            assert torch.equal(x.uvw, a[i].uvw) and torch.equal(x.rgb, a[i].rgb) and torch.equal(x.counts, a[i].counts)
            assert torch.equal(x.flags, a[i].flags) and x.box == a[i].box and x.window == a[i].window
        assert int(a[i].counts[1]) > 0 and int(a[i].counts[1]) == int(a[i].counts[2])


def test_two_runs_give_the_same_bits(batches):
    meshes, attrs, labels, colors = frame_problem(batches)
    a, b = run_many(meshes, attrs, labels, colors), run_many(meshes, attrs, labels, colors)
    for x, y in zip(a, b):
        assert torch.equal(x.uvw, y.uvw) and torch.equal(x.rgb, y.rgb) and torch.equal(x.counts, y.counts) and torch.equal(x.flags, y.flags)
    assert sum(int(x.counts[2]) for x in a) > 1000


def same_crops(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.box == w.box and g.window == w.window and g.uvw.shape == w.uvw.shape
        assert torch.equal(g.uvw, w.uvw) and torch.equal(g.counts, w.counts) and torch.equal(g.flags, w.flags)
        assert (g.rgb is None and w.rgb is None) or torch.equal(g.rgb, w.rgb)


def test_crops_many_with_a_raster_batch_gives_the_same_bits(batches):
    """raster= skips the rasterisation and nothing else; the third annotation's window is cut by the image border"""
    meshes, attrs, labels, colors = frame_problem(batches)
    dm, da = on_device(meshes, attrs)
    size = (VC.W, VC.H)
    rb = V.raster_batch(dm, VC.K8, V.label_windows(labels, size, 0.25)[1], size)
    for occ in (True, False):
        want = E.crops_many(dm, VC.K8, labels, size, colors=colors, attributes=da, occlusion=occ)
        syncs, got = count_syncs(lambda: E.crops_many(dm, VC.K8, labels, size, colors=colors, attributes=da, occlusion=occ, raster=rb))
        assert syncs == 0, syncs
        same_crops(got, want)
        print("occlusion %s: visible %s" % (occ, [int(c.counts[2]) for c in got]))
        assert want[2].box == (0, 0, 30, 40) and want[2].window[:2] == (0, 0) and sum(int(c.counts[2]) for c in want) > 1000
    # an empty window and a mesh without triangles beside a usual annotation
    empty = (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    meshes, attrs = [meshes[0], empty, meshes[1]], [attrs[0], np.zeros((0, 3), np.float32), attrs[1]]
    labels = [[10, 10, 10, 20], labels[0], labels[1]]
    rng = np.random.default_rng(22)
    colors = [EC.colour_crop(rng, (10, 10, 10, 20)), colors[0], colors[1]]
    dm, da = on_device(meshes, attrs)
    rb = V.raster_batch(dm, VC.K8, V.label_windows(labels, size, 0.25)[1], size)
    want = E.crops_many(dm, VC.K8, labels, size, colors=colors, attributes=da)
    same_crops(E.crops_many(dm, VC.K8, labels, size, colors=colors, attributes=da, raster=rb), want)
    assert want[0].uvw.shape == (10, 0, 3) and want[0].window[0] == want[0].window[2] and int(want[1].counts[1]) == 0 and int(want[2].counts[2]) > 0
    assert [int(c.flags) for c in want] == [0, 0, 0]


def test_a_raster_batch_made_for_something_else_is_refused(batches, monkeypatch):
    """the host check of raster= comes before any launch: the library is not even looked up"""
    meshes, attrs, labels, colors = frame_problem(batches)
    dm, da = on_device(meshes, attrs)
    size, K = (VC.W, VC.H), VC.K8
    win = V.label_windows(labels, size, 0.25)[1]
    other_faces = cam_mesh(meshes[2][0], np.concatenate([meshes[2][1], meshes[2][1]]))
    assert len(other_faces.vertices) == len(dm[2].vertices) and len(other_faces.faces) != len(dm[2].faces)
    K_ulp = tuple(np.nextafter(k, np.inf) if i == 2 else k for i, k in enumerate(K))
    stale = {
        "margin": V.raster_batch(dm, K, win, size),
        "one mesh fewer": V.raster_batch(dm[:2], K, win[:2], size),
        "face count": V.raster_batch(dm[:2] + [other_faces], K, win, size),
        "z_min": V.raster_batch(dm, K, win, size, z_min=0.2),
        "image_size": V.raster_batch(dm, K, win, (VC.W + 1, VC.H)),
        "K one ulp": V.raster_batch(dm, K_ulp, win, size),
    }
    good = V.raster_batch(dm, K, win, size)
    torch.cuda.synchronize()

    def no_library():
        raise AssertionError("the library was reached before the raster batch was refused")

    monkeypatch.setattr(_lib, "lib", no_library)
    for name, rb in stale.items():
        with pytest.raises(ValueError) as e:
            E.crops_many(dm, K, labels, size, colors=colors, attributes=da, margin=0.1 if name == "margin" else 0.25, raster=rb)
        print("%s: %s" % (name, str(e.value)[:160]))
        assert "raster batch" in str(e.value), name
    with pytest.raises(ValueError):
        V.verify_many(None, [None] * 3, dm, [None] * 3, K, labels, size, margin=0.1, raster=good)
    with pytest.raises(AssertionError):                                                       # and a batch that fits gets as far as the library
        E.crops_many(dm, K, labels, size, colors=colors, attributes=da, raster=good)


# ---- the frame pipeline --------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def frame_export(tmp_path_factory):
    """the inputs of test_gpu_verify.py::test_refine_frame_verify with crops=True, and the folder export_frame wrote; computed once"""
    pytest.importorskip("PIL")
    from sdflabel_amd.pipelines import optimizer as OP
    from sdflabel_amd.pipelines.export_crops import export_frame
    from sdflabel_amd.pipelines.frame import refine_frame
    from tests.test_gpu_frame import _synthetic_frame
    dec32 = sdflabel_amd.setup_dsdf(ASSET + ".pt", precision=torch.float32)[0].to(DEV)
    dec16 = sdflabel_amd.setup_dsdf(ASSET + ".pt", precision=torch.float16)[0].to(DEV)
    annos, K_orig, latents = _synthetic_frame(dec32, n=4)
    grid = sdflabel_amd.Grid3D(40, DEV)
    p_WC = np.eye(4)
    p_WC[:3, 3] = [0.1, -0.2, 0.3]
    W8 = {"2d": 0.3, "3d": 0.5}
    args = (annos, dec16, grid, latents, K_orig, p_WC, 3, W8)
    with pytest.raises(ValueError):
        refine_frame(*args, seed=7, crops=True)
    OP.clear_refiner_cache()
    est0, kept0 = refine_frame(*args, seed=7)
    OP.clear_refiner_cache()
    est, kept, st = refine_frame(*args, seed=7, return_stages=True, mesh_resolution=16, verify=True, crops=True)
    path = tmp_path_factory.mktemp("crops")
    with E.CropWriter(path) as writer:
        syncs, written = count_syncs(lambda: export_frame(st, writer, only_ok=False))
    return dict(est0=est0, kept0=kept0, est=est, kept=kept, stages=st, K=K_orig, path=str(path), written=written, syncs=syncs, annos=annos,
                args=args, dec16=dec16)


def test_refine_frame_crops(frame_export):
    from sdflabel_amd.datasets.crops import Crops
    f = frame_export
    est0, est, kept, st, K = f["est0"], f["est"], f["kept"], f["stages"], np.asarray(f["K"], np.float64)
    assert kept == f["kept0"] and len(kept) >= 2
    for k in est0:
        assert (est[k] == est0[k]) if k == "name" else (est[k].dtype == est0[k].dtype and est[k].tobytes() == est0[k].tobytes()), k
    crops = st["crops"]
    assert len(crops) == len(kept) == len(st["meshes"]) == len(st["verify"])
    live = [j for j, lab in enumerate(st["labels"]) if lab is not None]
    k4 = (K[0, 0], K[1, 1], K[0, 2], K[1, 2])
    size = (max(c.window[2] for c in crops), max(c.window[3] for c in crops))
    total = 0
    for c, m, i, j in zip(crops, st["meshes"], kept, live):
        l, t, r, b = (int(x) for x in f["annos"][i]["bbox"])
        assert c.box == (max(l, 0), max(t, 0), r, b) and c.window == st["verify"][live.index(j)]["window"]
        (ras,) = V.raster_many([m], K, [c.window], size)
        wl, wt = c.window[:2]
        sl = (slice(c.box[1] - wt, c.box[3] - wt), slice(c.box[0] - wl, c.box[2] - wl))
        uvw, depth, mask = c.uvw.cpu().numpy(), ras.depth.cpu().numpy()[sl], ras.mask.cpu().numpy()[sl]
        seen = uvw.astype(np.int64).sum(-1) > 0
        counts = c.counts.cpu().tolist()
        assert counts[:3] == [seen.size, int(mask.sum()), int(seen.sum())] and not (seen & (mask == 0)).any() and int(c.flags.cpu()) == 0
        pose, _ = V._pose_rows([st["params"][j]], torch.device(DEV))
        pose = pose.cpu().numpy()[0]
        err = identity_errors(uvw, seen, depth, k4, c.box, pose)
        bound = 1.0 / 255.0 + ER.shade_bound(float(pose[5]), pose[2:5])
        print("annotation %d: box %s, counts %s, unprojection identity max error %.9g, bound %.9g" % (i, c.box, counts, err.max(), bound))
        assert seen.sum() > 50 and err.max() <= bound
        rgb = c.rgb.cpu().numpy()
        assert (rgb == 128).all()                                                              # the synthetic frame's colour is 0.5 everywhere
        total += int(seen.sum())
    # export_frame(only_ok=False): one host read, and Crops reads the folder back identically
    assert f["syncs"] == 1 and f["written"] == list(range(len(crops)))
    ds = Crops(f["path"])
    assert len(ds) == len(crops)
    for n, (c, j) in enumerate(zip(crops, live)):
        s = ds[n]
        assert s["uvw"].tobytes() == c.uvw.cpu().numpy().tobytes() and s["rgb"].tobytes() == c.rgb.cpu().numpy().tobytes()
        lat = torch.as_tensor(st["params"][j]["latent"]).detach().float().cpu().reshape(-1)
        assert torch.equal(s["latent"], lat)                                                   # the raw refined latent
        want_k = K.copy()
        want_k[0, 2] -= c.box[0]
        want_k[1, 2] -= c.box[1]
        assert s["intrinsics"].numpy().tobytes() == want_k.astype(np.float32).tobytes()
        assert s["pose"].numpy().tobytes() == np.asarray(st["labels"][j][2], np.float64).astype(np.float32).tobytes()
    # only the accepted ones, and the visible share as a threshold
    from sdflabel_amd.pipelines.export_crops import export_frame

    class Sink:
        def __init__(self):
            self.n = 0

        def add(self, *a, **k):
            self.n += 1

    ok = [n for n, r in enumerate(st["verify"]) if r["ok"] and int(crops[n].counts[2]) > 0]
    assert export_frame(st, Sink()) == ok
    assert export_frame(st, Sink(), only_ok=False, min_visible=1.1) == []
    with pytest.raises(ValueError):
        export_frame({k: v for k, v in st.items() if k != "verify"}, Sink())


def test_refine_frame_rasterises_once(frame_export, monkeypatch):
    """verify and crops that agree on image size, margin and z_min share one raster batch; otherwise each makes its own.  Either way the
    stages are those of separate verify_many / crops_many calls on stages['meshes']"""
    from sdflabel_amd.pipelines import optimizer as OP
    from sdflabel_amd.pipelines.frame import _grown_size, refine_frame
    f = frame_export
    calls = []
    real = V.raster_batch
    monkeypatch.setattr(V, "raster_batch", lambda *a, **k: calls.append(1) or real(*a, **k))
    for verify, crops, n in ((True, True, 1), ({"margin": 0.25}, {"margin": 0.5}, 2)):
        OP.clear_refiner_cache()
        del calls[:]
        est, kept, st = refine_frame(*f["args"], seed=7, return_stages=True, mesh_resolution=16, verify=verify, crops=crops)
        print("verify=%s crops=%s: %d raster batches" % (verify, crops, len(calls)))
        assert len(calls) == n
        assert kept == f["kept0"]
        live = [j for j, lab in enumerate(st["labels"]) if lab is not None]
        boxes = [f["annos"][i]["bbox"] for i in kept]
        vm, cm = (0.25, 0.25) if verify is True else (verify["margin"], crops["margin"])
        want_v = V.verify_many(f["dec16"], [st["params"][j] for j in live], st["meshes"], [st["lidar"][i][0] for i in kept], f["K"], boxes,
                               _grown_size(boxes, vm), margin=vm)
        want_c = E.crops_many(st["meshes"], f["K"], boxes, _grown_size(boxes, cm), colors=[f["annos"][i]["color"] for i in kept], margin=cm)
        assert st["verify"] == want_v
        same_crops(st["crops"], want_c)
        if verify is True:                                                                     # and the fixture's own call gave these bits
            assert st["verify"] == f["stages"]["verify"]
            same_crops(st["crops"], f["stages"]["crops"])


def test_exported_folder_feeds_a_training_step(frame_export):
    """the folder export_frame wrote, through DeviceCropLoader (the augmentation kernels) into one train_step: finite losses"""
    from sdflabel_amd.datasets.crops import Crops, DeviceCropLoader
    from sdflabel_amd.networks.resnet_css import setup_css
    from sdflabel_amd.pipelines.train_css import train_step
    ds = Crops(frame_export["path"])
    loader = DeviceCropLoader(ds, batch_size=2, shuffle=True, generator=torch.Generator().manual_seed(7), device=DEV)
    b = next(iter(loader))
    assert tuple(b["rgb"].shape) == (2, 3, 128, 128) and b["uvw"].dtype == torch.uint8 and 0 < int(b["mask"].sum()) < b["mask"].numel()
    assert torch.equal(b["mask"], (b["uvw"].int().sum(1) > 0).to(torch.uint8))
    torch.manual_seed(1)
    net = setup_css(mode="train").to(DEV)
    got = train_step(net, torch.optim.Adam(net.parameters(), lr=1e-4), b)
    for k in ("loss", "uvw", "mask", "latent"):
        print("%s: %.9g" % (k, float(got[k])))
        assert torch.isfinite(got[k]).all(), k


def test_refine_sample_crops():
    """from a loaded sample: the windows are clipped to the sample's image, the RGB bytes are the image's own, the frame itself is unchanged"""
    from sdflabel_amd.fixtures import stand_in_css, synthetic_sample
    from sdflabel_amd.pipelines import optimizer as OP
    from sdflabel_amd.pipelines.frame import refine_sample
    dec32 = sdflabel_amd.setup_dsdf(ASSET + ".pt", precision=torch.float32)[0].to(DEV)
    dec16 = sdflabel_amd.setup_dsdf(ASSET + ".pt", precision=torch.float16)[0].to(DEV)
    smp, lidar = synthetic_sample(dec32, 40, 32, DEV)
    net = stand_in_css().to(DEV)
    grid = sdflabel_amd.Grid3D(40, DEV)
    W8, iters = {"2d": 0.3, "3d": 0.5}, 3
    with pytest.raises(ValueError):
        refine_sample(smp, net, dec16, grid, iters, W8, lidar=lidar, seed=7, crops=True)
    OP.clear_refiner_cache()
    est0, kept0, _ = refine_sample(smp, net, dec16, grid, iters, W8, lidar=lidar, seed=7)
    OP.clear_refiner_cache()
    est, kept, _, st = refine_sample(smp, net, dec16, grid, iters, W8, lidar=lidar, seed=7, return_stages=True, mesh_resolution=16,
                                     crops={"occlusion": False})
    assert kept == kept0 and len(kept) >= 1 and len(st["crops"]) == len(kept) == len(st["meshes"])
    for k in est0:
        assert (est[k] == est0[k]) if k == "name" else est[k].tobytes() == est0[k].tobytes(), k
    H, W = smp["image"].shape[:2]
    image = np.asarray(smp["image"], np.float32)
    for i, c in zip(kept, st["crops"]):
        l, t, r, b = c.box
        assert list(c.box) == [int(x) for x in st["boxes"][i]] and 0 <= c.window[0] <= l and r <= c.window[2] <= W and b <= c.window[3] <= H
        counts = c.counts.cpu().tolist()
        print(i, c.box, c.window, counts)
        assert c.rgb.cpu().numpy().tobytes() == ER.rgb_bytes(image[t:b, l:r]).tobytes()
        assert counts[0] == (b - t) * (r - l) and counts[1] == counts[2] > 0 and int(c.flags.cpu()) == 0
        assert int((c.uvw.int().sum(-1) > 0).sum()) == counts[2]
