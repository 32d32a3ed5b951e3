"""The synthetic bootstrap crops on the device (csrc/synth.hip, sdflabel_amd/synth.py) against the numpy restatement tests/_synth_ref.py:
owners, RGB bytes, NOCS bytes, flags and counts must be EQUAL -- both sides do the same float64 operations in the same order.  Every
figure is printed before it is asserted."""
import ctypes

import numpy as np
import pytest
import torch

import sdflabel_amd
from sdflabel_amd import _lib
from sdflabel_amd import export as E
from sdflabel_amd import synth
from sdflabel_amd import verify as V
from sdflabel_amd.fixtures import ASSET, GT_LATENT
from tests import _export_ref as ER
from tests import _synth_cases as SC
from tests import _synth_ref as SR
from tests.test_gpu_export import identity_errors
from tests.test_gpu_verify import count_syncs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 256
INVALID_FIRST = ("triangles_of_another_mesh", "box_outside_window", "scene_outside_the_table")


def restate(b):
    return SR.render(b["meshes"], b["normals"], b["K"], b["windows"], b["boxes"], b["size"], b["paint"], b["light"], b["ramp"], b["scene"],
                     b["bg_index"], b["bgs"], 0.1, b["triangles"])


@pytest.fixture(scope="module")
def batches():
    return SC.batches()


@pytest.fixture(scope="module")
def refs(batches):
    """name -> the restatement's result per annotation; computed once, never modified"""
    return {n: restate(b) for n, b in batches.items()}


def guarded(n, dtype, fill):
    return torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)


def inner(t):
    n = t.shape[0] - 2 * GUARD
    return t[GUARD:GUARD + n]


def raw_synth(b, qoff=None):
    """sdfr_mesh_raster, then sdfr_synth_owner / sdfr_crop_export (the normals as attributes) / sdfr_synth_shade / sdfr_crop_counts on outputs
    that sit between guard rows.  qoff: an offset table to pass in place of the boxes' own.  Returns per annotation a dict (owner, rgb, uvw,
    counts, flag) after checking the guards."""
    L = _lib.lib()
    B = len(b["meshes"])
    W, H = b["size"]
    wins = np.asarray(b["windows"], np.int32).reshape(-1, 4)
    boxes = np.asarray(b["boxes"], np.int32).reshape(-1, 4)
    voff = np.concatenate([[0], np.cumsum([len(v) for v, _ in b["meshes"]])]).astype(np.int64)
    toff = np.concatenate([[0], np.cumsum([len(f) for _, f in b["meshes"]])]).astype(np.int64)
    poff = np.concatenate([[0], np.cumsum((wins[:, 2] - wins[:, 0]).astype(np.int64) * (wins[:, 3] - wins[:, 1]))]).astype(np.int64)
    own_q = np.concatenate([[0], np.cumsum((boxes[:, 2] - boxes[:, 0]).astype(np.int64) * (boxes[:, 3] - boxes[:, 1]))]).astype(np.int64)
    V_, T, P, Q = int(voff[-1]), int(toff[-1]), int(poff[-1]), int(own_q[-1])
    S = len(b["light"])
    assert Q <= P                                             # what the entry points require; the buffers below have exactly these sizes
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    verts = up(np.concatenate([v for v, _ in b["meshes"]]).astype(np.float32).reshape(-1, 3))
    faces = up(np.concatenate([f for _, f in b["meshes"]]).astype(np.int32).reshape(-1, 3))
    nrm = up(np.concatenate(b["normals"]).astype(np.float32).reshape(-1, 3))
    d_voff, d_toff, d_poff, d_win, d_box = up(voff), up(toff), up(poff), up(wins), up(boxes)
    d_qoff = up(own_q if qoff is None else np.asarray(qoff, np.int64))
    d_scene = None if b["scene"] is None else up(np.asarray(b["scene"], np.int32))
    d_paint, d_light, d_ramp = up(np.asarray(b["paint"], np.float64)), up(np.asarray(b["light"], np.float64)), up(np.asarray(b["ramp"], np.int32))
    NBG = 0 if b["bgs"] is None else len(b["bgs"])
    d_bgi = up(np.asarray(b["bg_index"], np.int32)) if NBG else None
    d_bg = up(np.stack(b["bgs"]).astype(np.uint8)) if NBG else None
    keys = torch.empty((P,), dtype=torch.int64, device=DEV)
    mask = torch.empty((P,), dtype=torch.uint8, device=DEV)
    depth = torch.empty((P,), dtype=torch.float32, device=DEV)
    tri = torch.empty((P,), dtype=torch.int32, device=DEV)
    rflags = torch.empty((B,), dtype=torch.int32, device=DEV)
    k4 = (ctypes.c_double * 4)(*b["K"])
    Pt, st = _lib.ptr, _lib.stream_ptr()
    mesh = (Pt(verts) if V_ else None, V_, Pt(faces) if T else None, T)
    _lib.check(L.sdfr_mesh_raster(*mesh, Pt(d_voff), Pt(d_toff), Pt(d_win), Pt(d_poff), P, B, W, H, k4, 0.1, Pt(keys) if P else None,
                                  Pt(mask) if P else None, Pt(depth) if P else None, Pt(tri) if P else None, Pt(rflags), st), "sdfr_mesh_raster")
    if b["triangles"] is not None:
        host = tri.cpu().numpy().copy()
        for i, t in enumerate(b["triangles"]):
            if t is not None:
                host[int(poff[i]):int(poff[i + 1])] = np.asarray(t, np.int32).reshape(-1)
        tri = up(host)
    owner = guarded(P, torch.int32, -7)
    uvw, rgb = guarded(3 * Q, torch.uint8, 0xAB), guarded(3 * Q, torch.uint8, 0xCD)
    eflags, sflags, counts = guarded(B, torch.int32, 99), guarded(B, torch.int32, 98), guarded(4 * B, torch.int32, -5)
    d_owner = Pt(inner(owner)) if P else None
    _lib.check(L.sdfr_synth_owner(Pt(mask) if P else None, Pt(depth) if P else None, Pt(d_win), Pt(d_poff), P, Pt(d_scene), B, W, H, d_owner, st),
               "sdfr_synth_owner")
    _lib.check(L.sdfr_crop_export(*mesh, Pt(nrm) if V_ else None, Pt(d_voff), Pt(d_toff), Pt(d_win), Pt(d_poff), P, Pt(tri) if P else None, d_owner,
                                  Pt(d_box), Pt(d_qoff), Q, None, B, W, H, k4, 0.1, Pt(inner(uvw)) if Q else None, None, Pt(inner(eflags)), st),
               "sdfr_crop_export")
    _lib.check(L.sdfr_synth_shade(*mesh, Pt(nrm) if V_ else None, Pt(d_voff), Pt(d_toff), Pt(d_win), Pt(d_poff), P, Pt(tri) if P else None, d_owner,
                                  Pt(d_scene), Pt(d_box), Pt(d_qoff), Q, Pt(d_paint), Pt(d_light), S, Pt(d_bgi), Pt(d_bg), NBG, Pt(d_ramp), B, W, H, k4,
                                  0.1, Pt(inner(rgb)) if Q else None, Pt(inner(sflags)), st), "sdfr_synth_shade")
    _lib.check(L.sdfr_crop_counts(Pt(mask) if P else None, d_owner, Pt(d_win), Pt(d_poff), P, Pt(d_box), Pt(d_qoff), Q, Pt(inner(eflags)), B, W, H,
                                  Pt(inner(counts)), st), "sdfr_crop_counts")
    torch.cuda.synchronize()
    for t, fill in ((owner, -7), (uvw, 0xAB), (rgb, 0xCD), (eflags, 99), (sflags, 98), (counts, -5)):
        n = t.shape[0] - 2 * GUARD
        assert (t[:GUARD] == fill).all() and (t[GUARD + n:] == fill).all(), "a guard row was written"
    owner_h, uvw_h, rgb_h = inner(owner).cpu().numpy(), inner(uvw).cpu().numpy(), inner(rgb).cpu().numpy()
    flags_h, counts_h = inner(sflags).cpu().numpy(), inner(counts).cpu().numpy().reshape(B, 4)
    out = []
    for i in range(B):
        ws = (int(wins[i, 3] - wins[i, 1]), int(wins[i, 2] - wins[i, 0]))
        bs = (int(boxes[i, 3] - boxes[i, 1]), int(boxes[i, 2] - boxes[i, 0]), 3)
        q = slice(3 * int(own_q[i]), 3 * int(own_q[i + 1]))
        out.append(dict(owner=owner_h[int(poff[i]):int(poff[i + 1])].reshape(ws), uvw=uvw_h[q].reshape(bs), rgb=rgb_h[q].reshape(bs),
                        counts=counts_h[i], flag=int(flags_h[i])))
    return out


def same(got, want, name, b=None):
    nocs = None
    if b is not None and b["triangles"] is None and all(w["flag"] == 0 for w in want):
        nocs = SR.nocs(b["meshes"], b["normals"], b["K"], b["windows"], b["boxes"], want)
    for i, (g, w) in enumerate(zip(got, want)):
        print("%s[%d]: flag %d (restatement %d), counts %s, %d shaded pixels of %d" % (name, i, g["flag"], w["flag"], g["counts"].tolist(),
                                                                                      int((~np.isnan(w["val"][..., 0])).sum()), w["val"][..., 0].size))
        assert g["owner"].dtype == np.int32 and g["owner"].tobytes() == w["owner"].tobytes(), name
        assert g["rgb"].shape == w["rgb"].shape and g["rgb"].tobytes() == w["rgb"].tobytes(), name
        assert g["flag"] == w["flag"], name
        if nocs is not None:
            assert g["uvw"].tobytes() == nocs[i][0].tobytes() and g["counts"].tolist() == nocs[i][1].tolist(), name


# ---- the kernels -------------------------------------------------------------------------------------------------------------------------------

BATCHES = ["tetrahedron", "one_pixel_box_and_whole_window", "window_clipped_at_the_image_corner", "occluder_at_another_offset",
           "occluder_window_short", "depth_tie", "two_scenes", "image_background", "zero_and_nan_normal", "shin_0_7_and_ks_0", "one_row_image",
           "empty_mesh", "empty_window", "empty_window_beside_another", "triangles_of_another_mesh", "box_outside_window", "scene_outside_the_table"]


@pytest.mark.parametrize("name", BATCHES)
def test_synth_equals_the_restatement(batches, refs, name):
    """every batch alone, its outputs between guard rows.  empty_mesh: T = 0; empty_window: Q = 0; the boxes' areas are no multiples of the
    workgroup's 256 threads; the last three: flag bit 1, zeros, and the annotation beside it -- in another scene -- untouched"""
    assert set(BATCHES) == set(batches)
    got = raw_synth(batches[name])
    same(got, refs[name], name, batches[name])
    if name in INVALID_FIRST:
        assert got[0]["flag"] == V.FLAG_INVALID and not got[0]["rgb"].any() and got[1]["flag"] == 0 and got[1]["rgb"].any()
    if name == "depth_tie":
        assert (got[0]["owner"] <= 0).all() and (got[1]["owner"] == 0).sum() > 50                 # the lower index wins the exact ties
    if name == "occluder_at_another_offset":
        assert (got[0]["owner"] == 1).sum() > 100                                                 # shaded at the occluder's own window pixel


def test_sphere_equals_the_restatement():
    """5 k triangles of a few pixels each with their exact normals; outputs between guard rows"""
    b = SC.sphere_batch()[0]
    got, want = raw_synth(b), restate(b)
    same(got, want, "sphere24", b)
    assert (want[0]["mask"] != 0).sum() > 1000 and len(np.unique(got[0]["rgb"])) > 100


def test_offset_tables_that_do_not_fit(batches, refs):
    """qoff off by one: both annotations are flagged and every byte is zero; a last offset beyond Q: that annotation alone.  Guards intact."""
    b, want = batches["occluder_at_another_offset"], refs["occluder_at_another_offset"]
    q = [0, 64 * 48, 64 * 48 + 26 * 24]
    got = raw_synth(b, qoff=[0, q[1] - 1, q[2]])
    for g in got:
        print(g["counts"].tolist(), g["flag"])
        assert g["flag"] == V.FLAG_INVALID and not g["rgb"].any() and not g["uvw"].any()
    got = raw_synth(b, qoff=[0, q[1], q[2] + 5])
    same(got[:1], want[:1], "first of two")
    assert got[1]["flag"] == V.FLAG_INVALID and not got[1]["rgb"].any()
    got = raw_synth(b, qoff=[-3, q[1], q[2]])
    assert got[0]["flag"] == V.FLAG_INVALID and not got[0]["rgb"].any()
    same(got[1:], want[1:], "second of two")


def pick(b, idx, scene, scenes):
    """annotations idx of batch b with the scene numbers `scene`; scenes: which of b's light / ramp / background rows the new table holds"""
    return dict(b, meshes=[b["meshes"][i] for i in idx], normals=[b["normals"][i] for i in idx], windows=[b["windows"][i] for i in idx],
                boxes=[b["boxes"][i] for i in idx], paint=b["paint"][idx], scene=scene, light=b["light"][scenes], ramp=b["ramp"][scenes],
                bg_index=[b["bg_index"][s] for s in scenes])


def test_two_runs_and_a_scene_alone_or_elsewhere_in_the_batch(batches):
    """the same bits twice; scene 0 of two_scenes (annotations 0 and 2) alone, and as scene 1 behind the other scene's annotation"""
    b = batches["two_scenes"]
    a, again = raw_synth(b), raw_synth(b)
    for x, y in zip(a, again):
        assert all(x[k].tobytes() == y[k].tobytes() for k in ("owner", "rgb", "uvw", "counts")) and x["flag"] == y["flag"] == 0
    alone = raw_synth(pick(b, [0, 2], [0, 0], [0]))
    moved = raw_synth(pick(b, [1, 0, 2], [0, 1, 1], [1, 0]))
    other = raw_synth(pick(b, [1], None, [1]))
    for k in ("rgb", "uvw", "counts"):
        assert alone[0][k].tobytes() == a[0][k].tobytes() == moved[1][k].tobytes() and alone[1][k].tobytes() == a[2][k].tobytes() == moved[2][k].tobytes()
        assert other[0][k].tobytes() == a[1][k].tobytes() == moved[0][k].tobytes()
    assert (a[0]["owner"] == 2).sum() > 100 and (moved[1]["owner"] == 2).sum() == (a[0]["owner"] == 2).sum() == (alone[0]["owner"] == 1).sum()


# ---- scenes_many ---------------------------------------------------------------------------------------------------------------------------------

SIZE = (96, 64)
K96 = (70.0, 70.0, 47.5, 31.5)


def hand_scenes():
    """two scenes of two objects each; in both the second object stands nearer and beside the first and hides a part of it"""
    def obj(lat, yaw, scale, centre, albedo, ks, shin, jitter):
        return {"latent": lat, "yaw": yaw, "scale": scale, "trans": [c / scale for c in centre], "albedo": albedo, "ks": ks, "shin": shin,
                "jitter": jitter, "z": centre[2]}
    s0 = {"index": 5, "light": SC.light_row(0.3, -0.6, -0.7, 0, 0)[:3], "ambient": 0.25, "kd": 0.7, "background": None,
          "ramp": [40, 90, 200, 120, 110, 60, 30, 1234], "objects": [obj(0, 0.5, 1.5, (-0.6, 0.1, 9.0), [0.8, 0.2, 0.2], 0.3, 4, [0.1, 0.05, -0.05, 0.1]),
                                                                     obj((0, 1, 0.4), -1.0, 1.4, (0.5, 0.2, 6.5), [0.2, 0.3, 0.8], 0.4, 5, [0, 0, 0, 0])]}
    s1 = {"index": 6, "light": SC.light_row(-0.5, -0.4, -0.6, 0, 0)[:3], "ambient": 0.2, "kd": 0.6, "background": 0,
          "ramp": [0] * 8, "objects": [obj(1, 2.4, 1.6, (0.4, -0.1, 10.0), [0.7, 0.7, 0.1], 0.0, 3, [-0.05, 0.1, 0.1, -0.05]),
                                       obj(2, 0.2, 1.3, (-0.3, 0.3, 7.0), [0.3, 0.8, 0.4], 0.5, 7, [0.1, 0.1, 0.1, 0.1])]}
    return [s0, s1]


@pytest.fixture(scope="module")
def rendered():
    """scenes_many on the committed decoder fit at R = 24; computed once"""
    dec = sdflabel_amd.setup_dsdf(ASSET + ".pt", precision=torch.float32)[0].to(DEV)
    rng = np.random.default_rng(3)
    latents = torch.from_numpy((np.asarray(GT_LATENT, np.float32) + rng.uniform(-0.1, 0.1, (3, 3)).astype(np.float32)))
    scenes = hand_scenes()
    bgs = torch.from_numpy(rng.integers(0, 256, (1, SIZE[1], SIZE[0], 3)).astype(np.uint8))
    meshes = synth.scene_meshes(dec, latents, scenes, resolution=24)
    syncs, (crops, report) = count_syncs(lambda: synth.scenes_many(dec, latents, scenes, K96, SIZE, resolution=24, backgrounds=bgs, meshes=meshes))
    whole, report2 = synth.scenes_many(dec, latents, scenes, K96, SIZE, resolution=24, backgrounds=bgs)      # the meshes made inside
    return dict(dec=dec, latents=latents, scenes=scenes, bgs=bgs.numpy(), meshes=meshes, syncs=syncs, crops=crops, report=report, whole=whole,
                report2=report2)


def test_scenes_many(rendered):
    r = rendered
    crops, scenes, (cam, rows) = r["crops"], r["scenes"], r["meshes"]
    print("scenes_many: %d host synchronisations, report %s" % (r["syncs"], r["report"]))
    assert r["syncs"] == 1                                                                # with the meshes at hand: the read of the mask counts
    assert r["report"]["kept"] == [(5, 0), (5, 1), (6, 0), (6, 1)] and r["report"]["dropped"] == [] and r["report2"] == r["report"]
    assert [(c.scene, c.object) for c in crops] == r["report"]["kept"] and len(crops) == len(r["whole"]) == 4
    for c, w in zip(crops, r["whole"]):                                                    # the same bits with the meshes made inside
        assert torch.equal(c.uvw, w.uvw) and torch.equal(c.rgb, w.rgb) and torch.equal(c.counts, w.counts) and c.box == w.box
    print("triangles per mesh: %s" % [len(m) for m in cam])
    assert all(m.frame == "camera" for m in cam) and all(100 < len(m) for m in cam)
    objs = [(si, o) for si, s in enumerate(scenes) for o in s["objects"]]
    # the restatement on the device's meshes: RGB, NOCS and counts
    b = dict(K=K96, size=SIZE, meshes=[(m.vertices_numpy(), m.faces_numpy()) for m in cam], normals=[m.normals_numpy() for m in cam],
             windows=[c.window for c in crops], boxes=[c.box for c in crops], scene=[si for si, _ in objs],
             paint=np.array([o["albedo"] + [o["ks"], o["shin"]] for _, o in objs], np.float64),
             light=np.array([s["light"] + [s["ambient"], s["kd"]] for s in scenes], np.float64), ramp=np.array([s["ramp"] for s in scenes], np.int32),
             bg_index=[-1, 0], bgs=[r["bgs"][0]], triangles=None)
    want = restate(b)
    nocs = SR.nocs(b["meshes"], [m.lattice_vertices.cpu().numpy() for m in cam], K96, b["windows"], b["boxes"], want)
    raster = V.raster_many(cam, K96, [c.window for c in crops], SIZE)
    hidden = shown = 0
    for i, (c, (si, o)) in enumerate(zip(crops, objs)):
        uvw, rgb, counts = c.uvw.cpu().numpy(), c.rgb.cpu().numpy(), c.counts.cpu().tolist()
        print("crop %d: scene %d, box %s in window %s, counts %s, flags %d" % (i, c.scene, c.box, c.window, counts, int(c.flags)))
        assert int(c.flags) == 0 and want[i]["flag"] == 0 and counts == nocs[i][1].tolist()
        assert rgb.tobytes() == want[i]["rgb"].tobytes() and uvw.tobytes() == nocs[i][0].tobytes()
        assert torch.equal(c.latent, rows[i]) and np.array_equal(c.extrinsics, cam[i].cam_T) and c.intrinsics[0, 2] == K96[2]
        # wherever the crop is visible its NOCS bytes are crops_many's for the same mesh and box without occlusion; zero elsewhere
        (solo,) = E.crops_many([cam[i]], K96, [list(c.box)], SIZE, occlusion=False)
        assert solo.box == c.box
        seen = uvw.astype(np.int64).sum(-1) > 0
        assert seen.sum() == counts[2] > 0 and (uvw[seen] == solo.uvw.cpu().numpy()[seen]).all() and not uvw[~seen].any()
        hidden += counts[1] - counts[2]
        # the unprojection identity of test_export_cpu on the visible pixels
        l, t = c.window[:2]
        sl = (slice(c.box[1] - t, c.box[3] - t), slice(c.box[0] - l, c.box[2] - l))
        depth = raster[i].depth.cpu().numpy()[sl]
        pose, _ = V._pose_rows([{"yaw": np.float32(o["yaw"]), "trans": np.asarray(o["trans"], np.float32), "scale": np.float32(o["scale"]),
                                 "latent": np.zeros(3, np.float32)}], torch.device(DEV))
        pose = pose.cpu().numpy()[0]
        err = identity_errors(uvw, seen, depth, K96, c.box, pose)
        bound = 1.0 / 255.0 + ER.shade_bound(float(pose[5]), pose[2:5])
        print("        unprojection identity max error %.9g, bound %.9g" % (err.max(), bound))
        assert err.max() <= bound
        # the background's own bytes exactly where nothing of the scene covers the pixel
        free = np.ones(uvw.shape[:2], bool)
        for j, (sj, _) in enumerate(objs):
            if sj != si:
                continue
            wl, wt, wr, wb = crops[j].window
            full = np.zeros((SIZE[1], SIZE[0]), bool)
            full[wt:wb, wl:wr] = raster[j].mask.cpu().numpy() != 0
            free &= ~full[c.box[1]:c.box[3], c.box[0]:c.box[2]]
        ys, xs = np.nonzero(free)
        bg = r["bgs"][0][ys + c.box[1], xs + c.box[0]] if si == 1 else SR.ramp_bytes(scenes[0]["ramp"], SIZE[1], xs + c.box[0], ys + c.box[1])
        assert not uvw[free].any() and (rgb[free] == bg).all()
        shown += int(free.sum())
    print("hidden pixels %d, background pixels compared %d" % (hidden, shown))
    assert hidden > 10 and shown > 20                                                      # something is occluded, some background is in sight


def test_bootstrap_crops_writes_a_folder_that_trains(rendered, tmp_path):
    """six crops through CropWriter; Crops reads them back with mask == visible set; DeviceCropLoader feeds one train_step"""
    pytest.importorskip("PIL")
    import json
    from sdflabel_amd.datasets.crops import Crops, DeviceCropLoader
    from sdflabel_amd.networks.resnet_css import setup_css
    from sdflabel_amd.pipelines.synth_crops import bootstrap_crops
    from sdflabel_amd.pipelines.train_css import train_step
    path = tmp_path / "crops"
    kw = dict(seed=3, batch_scenes=2, resolution=24, max_objects=2, scale_range=(1.2, 1.8), z_near=6.0, z_far=12.0, border=0.2)
    n = bootstrap_crops(rendered["dec"], rendered["latents"], path, 6, K96, SIZE, **kw)
    assert n == 6
    ds = Crops(str(path))
    gt = json.load(open(path / "crops.json"))
    assert len(ds) == 6 and sorted(gt) == [str(i) for i in range(6)]
    for i in range(6):
        s, e = ds[i], gt[str(i)][0]
        l, t, r_, b = e["box"]
        uvw = np.asarray(s["uvw"])
        print("crop %d: scene %d object %d yaw %.3f box %s visible %d covered %d" % (i, e["scene"], e["object"], e["yaw"], e["box"], e["visible"], e["covered"]))
        assert e["synthetic"] is True and uvw.shape == (b - t, r_ - l, 3) and np.asarray(s["rgb"]).shape == uvw.shape
        assert int((uvw.astype(np.int64).sum(-1) > 0).sum()) == e["visible"] > 0 and e["visible"] <= e["covered"]
        assert len(e["latent"]) == 3 and np.asarray(e["extrinsics"]).shape == (4, 4) and e["intrinsics"][0][2] == K96[2] - l
    # the scenes do not depend on the batching: the first crops of another batch size are the same files
    other = tmp_path / "other"
    bootstrap_crops(rendered["dec"], rendered["latents"], other, 3, K96, SIZE, **dict(kw, batch_scenes=3))
    ds2 = Crops(str(other))
    for i in range(3):
        assert np.asarray(ds2[i]["rgb"]).tobytes() == np.asarray(ds[i]["rgb"]).tobytes() and np.asarray(ds2[i]["uvw"]).tobytes() == np.asarray(ds[i]["uvw"]).tobytes()
    loader = DeviceCropLoader(ds, batch_size=2, shuffle=True, generator=torch.Generator().manual_seed(7), device=DEV)
    bt = next(iter(loader))
    assert tuple(bt["rgb"].shape) == (2, 3, 128, 128) and bt["uvw"].dtype == torch.uint8 and 0 < int(bt["mask"].sum()) < bt["mask"].numel()
    assert torch.equal(bt["mask"], (bt["uvw"].int().sum(1) > 0).to(torch.uint8))
    torch.manual_seed(1)
    net = setup_css(mode="train").to(DEV)
    got = train_step(net, torch.optim.Adam(net.parameters(), lr=1e-4), bt)
    for k in ("loss", "uvw", "mask", "latent"):
        print("%s: %.9g" % (k, float(got[k])))
        assert torch.isfinite(got[k]).all(), k
