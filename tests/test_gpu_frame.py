"""Frame labelling on the GPU (csrc/frame.hip, sdflabel_amd/frame.py, pipelines/refinement.py, pipelines/frame.py) against golden G18, recorded
from the reference's own utils/refinement.py functions by tools/make_golden_frame.py.  Every figure is printed before it is asserted."""
import warnings

import numpy as np
import pytest
import torch

import sdflabel_amd
from sdflabel_amd import _lib
from sdflabel_amd import frame as FR
from sdflabel_amd.pipelines import refinement as rtools
from tests._util import ASSET, gold

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
G3_TOL = 1e-5            # tests/test_gpu_parity.py test_surface_points_golden: |surface point - G3| < 1e-5


@pytest.fixture(scope="module")
def z():
    return gold("g18_frame_labels.npz")


@pytest.fixture(scope="module")
def dec32():
    return sdflabel_amd.setup_dsdf(ASSET + ".pt", precision=torch.float32)[0].to(DEV)


@pytest.fixture(scope="module")
def dec16():
    return sdflabel_amd.setup_dsdf(ASSET + ".pt", precision=torch.float16)[0].to(DEV)


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


# ---- reproject ---------------------------------------------------------------------------------------------------------------------------

def _rp_case(z, i):
    p = "rp%d_" % i
    depth = torch.from_numpy(z[p + "depth"])
    return dict(color=torch.from_numpy(z[p + "color"]), depth=depth.unsqueeze(0) if bool(z[p + "depth3d"]) else depth, K=torch.from_numpy(z[p + "K"]),
                filter=bool(z[p + "filter"]), points=z[p + "points"], colors=z[p + "colors"], yx=z[p + "yx"], Kinv=z[p + "Kinv"], name=str(z[p + "name"]))


def test_reproject_matches_the_reference(z):
    """counts and row order identical, colours bit-equal, points within 4 2^-24 (|k0 x| + |k1 y| + |k2|) depth per component (a 3-term float32
    dot product in either summation order, times the depth); crops without a hit and with one hit included"""
    n = int(z["rp_n"])
    seen = set()
    for i in range(n):
        c = _rp_case(z, i)
        (pts, cls), = FR.reproject_many([c["color"]], [c["depth"]], [c["K"]], filter=c["filter"])
        assert pts.is_cuda and pts.dtype == cls.dtype == torch.float32
        pts, cls = pts.cpu().numpy(), cls.cpu().numpy()
        m = c["points"].shape[0]
        seen.add(min(m, 2))
        assert pts.shape == cls.shape == (m, 3), (c["name"], pts.shape, m)
        assert np.array_equal(cls, c["colors"]), c["name"]                      # bit-equal colours in the reference's row order
        if m == 0:
            continue
        x, y = c["yx"][:, 1].astype(np.float64), c["yx"][:, 0].astype(np.float64)
        d = np.abs(c["depth"].squeeze().numpy()[c["yx"][:, 0], c["yx"][:, 1]].astype(np.float64))
        k = np.abs(c["Kinv"].astype(np.float64))
        bound = 4 * U * (k[:, 0][None] * x[:, None] + k[:, 1][None] * y[:, None] + k[:, 2][None]) * d[:, None]
        err = np.abs(pts.astype(np.float64) - c["points"])
        print("reproject %-28s n = %4d  largest |got - ref| = %.3e, largest share of the bound = %.3f" % (c["name"], m, err.max(), (err / np.maximum(bound, 1e-300)).max()))
        assert (err <= bound).all(), c["name"]
    assert seen == {0, 1, 2}


def test_reproject_batched_equals_single_crops_bit_for_bit(z):
    n = int(z["rp_n"])
    for filt in (False, True):
        cs = [_rp_case(z, i) for i in range(n)]
        single = [FR.reproject_many([c["color"]], [c["depth"]], [c["K"]], filter=filt)[0] for c in cs]
        syncs, many = count_syncs(lambda: FR.reproject_many([c["color"] for c in cs], [c["depth"] for c in cs], [c["K"] for c in cs], filter=filt))
        assert syncs == 1, syncs                                                # the read of the counts
        assert len(many) == n
        for (p1, c1), (pm, cm) in zip(single, many):
            assert p1.shape == pm.shape and torch.equal(p1, pm) and torch.equal(c1, cm)
        # device inputs give the same bits as host inputs
        dev = FR.reproject_many([c["color"].to(DEV) for c in cs], [c["depth"].to(DEV) for c in cs], [c["K"] for c in cs], filter=filt)
        for (p1, c1), (pd, cd) in zip(single, dev):
            assert torch.equal(p1, pd) and torch.equal(c1, cd)


def test_reproject_drop_in_function(z):
    c = _rp_case(z, 3)
    pts, cls = rtools.reproject(c["color"], c["depth"], c["K"], filter=True)
    assert torch.is_tensor(pts) and np.array_equal(cls.cpu().numpy(), c["colors"])
    pn, cn = rtools.reproject(c["color"].numpy(), c["depth"].numpy(), c["K"].numpy(), flip_color_channels=True, filter=True)
    assert isinstance(pn, np.ndarray) and np.array_equal(pn, pts.cpu().numpy()) and np.array_equal(cn, c["colors"][:, ::-1])


def test_reproject_capacity_overflow_sets_the_sticky_flag_and_writes_nothing_out_of_bounds(z):
    big, one = _rp_case(z, 4), _rp_case(z, 8)
    n_big = big["points"].shape[0]
    cap = 50
    assert n_big > cap
    args = ([big["color"], one["color"]], [big["depth"], one["depth"]], [big["K"], one["K"]])
    full = FR.reproject_device(*args, filter=False)
    out = FR.reproject_device(*args, filter=False, cap=cap)
    assert out["points"].shape == (2, cap, 3)
    assert out["cnt"].tolist() == full["cnt"].tolist() == [n_big, 1]            # the TRUE count
    assert out["over"].tolist() == [1, 0]
    assert torch.equal(out["points"][0], full["points"][0, :cap]) and torch.equal(out["colors"][0], full["colors"][0, :cap])
    assert torch.equal(out["points"][1, 0], full["points"][1, 0])               # the surplus of crop 0 did not spill into crop 1's rows
    again = FR.reproject_device([one["color"]], [one["depth"]], [one["K"]], filter=False, cap=cap, over=out["over"][:1])
    assert again["over"].tolist() == [1] and out["over"].tolist() == [1, 0]    # sticky: a later call that fits leaves the flag set
    with pytest.raises(_lib.SdfrError, match="cap"):
        FR.reproject_many(*args, filter=False, cap=cap)


def test_point_extents_c_abi(z):
    """sdfr_point_extents through the C ABI: ragged lists by offsets and a [B][cap] array, an empty list (count 0, NaN: never an extreme)"""
    rng = np.random.default_rng(5)
    clouds = [rng.normal(size=(n, 3)).astype(np.float32) + np.float32([0, 0, 6]) for n in (1500, 0, 1, 300)]
    A = rng.normal(size=(4, 3, 3)).astype(np.float32)
    s = rng.uniform(1, 3, 4).astype(np.float32)
    t = rng.normal(size=(4, 3)).astype(np.float32) + np.float32([0, 0, 20])
    K = np.tile(np.float32([[700, 0, 600], [0, 710, 180], [0, 0, 1]]).reshape(9), (4, 1))
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)      # noqa: E731
    flat, off, cnt, cap = FR._ragged(clouds, torch.device(DEV))
    ext, n = FR.point_extents(flat, off, cnt, cap, 4, T(A.reshape(4, 9)), T(s), T(t), T(K))
    ext, n = ext.cpu().numpy(), n.cpu().numpy()
    assert n.tolist() == [1500, 0, 1, 300] and np.isnan(ext[1]).all()
    for b in (0, 2, 3):
        q = clouds[b] * s[b]
        w = ((A[b, :, 0] * q[:, :1] + A[b, :, 1] * q[:, 1:2]) + A[b, :, 2] * q[:, 2:3]) + t[b]          # float32, the kernel's order
        uv = np.stack([np.float32(700) * (w[:, 0] / w[:, 2]) + np.float32(600), np.float32(710) * (w[:, 1] / w[:, 2]) + np.float32(180)], 1)
        want = np.float32([w[:, 0].min(), w[:, 0].max(), w[:, 1].min(), w[:, 1].max(), w[:, 2].min(), w[:, 2].max(),
                           uv[:, 0].min(), uv[:, 0].max(), uv[:, 1].min(), uv[:, 1].max()])
        assert np.array_equal(ext[b, :6], want[:6]), b
        assert np.abs(ext[b, 6:] - want[6:]).max() <= 8 * U * np.abs(want[6:]).max(), b      # the division may differ in its last bit
    padded = torch.zeros((4, cap, 3), device=DEV)
    for b, c in enumerate(clouds):
        if len(c):
            padded[b, :len(c)] = T(c)
    e2, n2 = FR.point_extents(padded, None, cnt, cap, 4, T(A.reshape(4, 9)), T(s), T(t), None)
    e2 = e2.cpu().numpy()
    assert n2.tolist() == n.tolist() and np.array_equal(e2[[0, 2, 3], :6], ext[[0, 2, 3], :6]) and np.isnan(e2[:, 6:]).all()
    h = _lib.lib()
    assert h.sdfr_point_extents(None, None, None, 4, 2, None, None, None, None, 0, None, None, None) == -1
    assert h.sdfr_reproject(None, None, None, None, 2, 16, 0, 16, None, None, None, None, None, 1, None) == -1


# ---- labels ------------------------------------------------------------------------------------------------------------------------------

def _label_params(z, i, dev=None):
    p = "label%d_" % i
    f = (lambda a: torch.from_numpy(a).to(dev)) if dev else (lambda a: a)
    return {"latent": f(z[p + "latent"]), "scale": f(z[p + "scale"]), "trans": f(z[p + "trans"]), "yaw": f(z[p + "yaw"])}


def _check_label(lab, cam_T, z, q, ext_tol, dim_slack):
    """extents within ext_tol -> dimensions within 2 ext_tol (+ the rounding of the difference), location within ext_tol (the bottom centre
    moves along one unit column of the rigid global_T) + 1e-6; the angles and cam_T do not depend on the surface: 1e-6"""
    dims = np.asarray(lab["dimensions"])
    figs = dict(dimensions=np.abs(dims.astype(np.float64) - z[q + "dimensions"].astype(np.float64)).max(),
                location=np.abs(lab["location"] - z[q + "location"]).max(), rotation_y=abs(lab["rotation_y"] - float(z[q + "rotation_y"])),
                alpha=abs(lab["alpha"] - float(z[q + "alpha"])), cam_T=np.abs(cam_T - z[q + "cam_T"]).max())
    print("   ", q, " ".join("%s %.3e" % kv for kv in figs.items()), "(extent tolerance %.3e)" % ext_tol)
    assert dims.dtype == z[q + "dimensions"].dtype
    assert figs["dimensions"] <= 2 * ext_tol + dim_slack
    assert figs["location"] <= ext_tol + 1e-6
    assert figs["rotation_y"] < 1e-6 and figs["alpha"] < 1e-6 and figs["cam_T"] < 1e-6


def test_labels_many_float32_matches_the_reference(z, dec32):
    """N identical; extents within the G3 surface tolerance (1e-5 per point coordinate) times the scale; label fields within what that
    propagates to, plus 1e-6; six annotations batched are bit-identical to one at a time; one host synchronisation per chunk"""
    n = int(z["label_n"])
    grid = sdflabel_amd.Grid3D(int(z["label_D"]), DEV)
    params = [_label_params(z, i) for i in range(n)]
    bboxes = [z["label%d_bbox" % i].tolist() for i in range(n)]
    pw = z["label_p_WC"]
    FR.labels_many(dec32, grid, params[:1], pw, bboxes[:1])                     # (the decoder's handle is built outside the counted call)
    syncs, (res, raw) = count_syncs(lambda: FR.labels_many(dec32, grid, params, pw, bboxes, return_raw=True))
    assert syncs == 1 and len(raw) == 1, syncs
    syncs2, res2 = count_syncs(lambda: FR.labels_many(dec32, grid, params, pw, bboxes, max_batch=4))
    assert syncs2 == 2, syncs2                                                  # two chunks
    for i in range(n):
        q = "label%d_f32_" % i
        lab, sp, cam_T = res[i]
        scale = float(z["label%d_scale" % i][0])
        ext = raw[0]["ext"][i]
        err = np.abs(ext.astype(np.float64) - z[q + "ext"].astype(np.float64)).max()
        print("label %d f32: N %d (golden %d), largest extent error %.3e, band margin %.3e" % (i, raw[0]["n"][i], int(z[q + "N"]), err,
                                                                                          float(z["label%d_band_margin" % i])))
        assert int(raw[0]["n"][i]) == int(z[q + "N"]) == len(sp)
        assert err <= G3_TOL * scale
        _check_label(lab, cam_T, z, q, G3_TOL * scale, 4 * U * 4.0)
        assert lab["bbox"] == bboxes[i] and lab["name"] == "Car" and lab["score"] == 1
        # batched == chunked == alone, bit for bit
        (l1, s1, c1), = FR.labels_many(dec32, grid, [_label_params(z, i, DEV)], pw, [bboxes[i]])
        for other in (res2[i][0], l1):
            assert np.array_equal(other["location"], lab["location"]) and other["dimensions"] == lab["dimensions"]
            assert other["rotation_y"] == lab["rotation_y"] and other["alpha"] == lab["alpha"]
        assert np.array_equal(c1, cam_T) and torch.equal(s1.device(), sp.device())
        # scaled_points: fetched on demand, the points the extents were taken over
        a = np.asarray(sp)
        assert a.dtype == np.float32 and a.shape == (int(z[q + "N"]), 3)
        assert np.array_equal(np.float32([a[:, 0].min(), a[:, 0].max(), a[:, 1].min(), a[:, 1].max(), a[:, 2].min(), a[:, 2].max()]), ext)
    # the drop-in function for one annotation
    p0 = _label_params(z, 0, DEV)
    lab, sp, cam_T = rtools.get_kitti_label(dec32, grid, p0["latent"], p0["scale"], p0["trans"], p0["yaw"], pw, bboxes[0])
    assert isinstance(sp, np.ndarray) and np.array_equal(lab["location"], res[0][0]["location"]) and np.array_equal(cam_T, res[0][2])


def test_labels_many_takes_the_latent_raw(z, dec32):
    """get_kitti_label evaluates params['latent'] un-normalised (utils/refinement.py:536): the label of a raw latent of norm != 1 has the
    golden's dimensions, and the normalised latent gives other ones (recorded from the reference as well)"""
    grid = sdflabel_amd.Grid3D(int(z["label_D"]), DEV)
    for i in range(int(z["label_n"])):
        p = _label_params(z, i)
        raw_dims = np.asarray(FR.labels_many(dec32, grid, [p], z["label_p_WC"], [[0, 0, 1, 1]])[0][0]["dimensions"])
        pn = dict(p, latent=(p["latent"] / np.linalg.norm(p["latent"])).astype(np.float32))
        nrm_dims = np.asarray(FR.labels_many(dec32, grid, [pn], z["label_p_WC"], [[0, 0, 1, 1]])[0][0]["dimensions"])
        tol = 2 * G3_TOL * float(p["scale"][0]) + 1e-6
        gap = np.abs(z["label%d_f32_dimensions" % i] - z["label%d_dimensions_normalised_latent" % i]).max()
        print("label %d: |latent| %.3f, dimensions raw vs normalised differ by %.3e" % (i, np.linalg.norm(p["latent"]), gap))
        assert gap > 100 * tol
        assert np.abs(raw_dims - z["label%d_f32_dimensions" % i]).max() <= tol
        assert np.abs(nrm_dims - z["label%d_dimensions_normalised_latent" % i]).max() <= tol


def test_labels_many_float16_matches_the_reference_float16(z, dec16):
    """the reference's own float16 run (decoder, grid and parameters half): per case the extents within twice the recorded
    |reference f16 - reference f32| extent difference (label<i>_f16_tol of the golden; the x2 covers the device's own rounding, of the same
    order).  The surface and its product with the scale are float16 values."""
    n = int(z["label_n"])
    grid = sdflabel_amd.Grid3D(int(z["label_D"]), DEV, torch.float16)
    params = [_label_params(z, i) for i in range(n)]
    bboxes = [z["label%d_bbox" % i].tolist() for i in range(n)]
    res, raw = FR.labels_many(dec16, grid, params, z["label_p_WC"], bboxes, return_raw=True)
    figs = []
    for i in range(n):
        q = "label%d_f16_" % i
        tol = float(z["label%d_f16_tol" % i])
        ext = raw[0]["ext"][i]
        assert ext.dtype == np.float16 == z[q + "ext"].dtype
        err = np.abs(ext.astype(np.float64) - z[q + "ext"].astype(np.float64))
        figs.append((err.max(), tol))
        print("label %d f16: N %d (reference f16 %d), extent errors %s, tolerance %.3e" % (i, raw[0]["n"][i], int(z[q + "N"]), np.array2string(err, precision=2), tol))
    for i in range(n):
        assert figs[i][0] <= figs[i][1], (i, figs)
    for i in range(n):
        q = "label%d_f16_" % i
        lab, sp, cam_T = res[i]
        assert sp.device().dtype == torch.float16 and np.asarray(sp).dtype == np.float16
        # dimensions are float16 differences of float16 extents: one more rounding of half an ulp of a value below 8
        _check_label(lab, cam_T, z, q, figs[i][1], 2.0 ** -9)


def test_labels_many_empty_band_and_capacity(z, dec32):
    grid = sdflabel_amd.Grid3D(int(z["label_D"]), DEV)
    params = [_label_params(z, i) for i in range(2)]
    res = FR.labels_many(dec32, grid, params, z["label_p_WC"], [[0, 0, 1, 1]] * 2, threshold=0.0)        # |sdf| < 0: no row
    assert res == [None, None]
    assert FR.frame_dict(res)["location"].shape[0] == 0
    with pytest.raises(_lib.SdfrError, match="cap"):
        FR.labels_many(dec32, grid, params, z["label_p_WC"], [[0, 0, 1, 1]] * 2, cap=64)                  # the sticky flag of the band selection
    assert FR.labels_many(dec32, grid, [], z["label_p_WC"], []) == []


# ---- initial parameters ------------------------------------------------------------------------------------------------------------------

def test_init_params_many_matches_the_reference_on_both_sides_of_the_iou_test(z):
    """world = rot (pcd scale) + tra on the device in float32: every coordinate is three products and three sums, so it is within
    4 2^-24 (sum of the |terms|) <= 32 2^-24 max|world| =: bw of the reference's; u, v within fx 2 bw / zmin + 8 2^-24 max|uv|; the decision
    iou < 0.7 is the reference's (the golden keeps |iou - 0.7| >= 1e-3); trans is exact where the height is kept, else within bw / scale + 1e-6"""
    n = int(z["init_n"])
    K = z["init_K_orig"]
    poses, pcds, scenes, bboxes, lats = [], [], [], [], []
    for i in range(n):
        p = "init%d_" % i
        scale = float(z[p + "scale"]) if bool(z[p + "scale_is_float"]) else np.float32(z[p + "scale"])
        poses.append({"scale": scale, "rot": z[p + "rot"].copy(), "tra": z[p + "tra"].copy()})
        pcds.append(torch.from_numpy(z[p + "pcd"]).to(DEV))
        scenes.append(torch.from_numpy(z[p + "scene"]).to(DEV))
        bboxes.append(z[p + "bbox"].tolist())
        lats.append(z[p + "latent"])
    poses.insert(2, None), pcds.insert(2, None), scenes.insert(2, None), bboxes.insert(2, None), lats.insert(2, None)
    half_groups = [[j for j in range(n + 1) if poses[j] is not None and pcds[j].dtype == torch.float16],
                   [j for j in range(n + 1) if poses[j] is None or pcds[j].dtype != torch.float16]]
    out, info = [None] * (n + 1), [None] * (n + 1)
    for grp in half_groups:                           # a launch holds clouds of one dtype
        syncs, (r, inf) = count_syncs(lambda: FR.init_params_many([poses[j] for j in grp], [pcds[j] for j in grp], [scenes[j] for j in grp],
                                                                  [bboxes[j] for j in grp], K, [lats[j] for j in grp], return_info=True))
        assert syncs == 1, syncs
        for j, a, b in zip(grp, r, inf):
            out[j], info[j] = a, b
    assert out[2] is None
    sides = set()
    for i in range(n):
        p = "init%d_" % i
        j = i if i < 2 else i + 1
        got, inf = out[j], info[j]
        bw = 32 * U * float(z[p + "world_absmax"])
        ref = z[p + "ext"]
        exyz = np.abs(inf["ext"][:6].astype(np.float64) - ref[:6]).max()
        euv = np.abs(inf["ext"][6:].astype(np.float64) - ref[6:]).max()
        buv = float(K[0, 0]) * 2 * bw / float(ref[4]) + 8 * U * np.abs(ref[6:]).max()
        low = float(z[p + "iou"]) < 0.7
        sides.add(low)
        etr = np.abs(got["trans"].astype(np.float64) - z[p + "trans"]).max()
        print("init %d: iou %.6f (reference %.6f, margin %.1e), world extents off by %.3e (bound %.3e), box off by %.3e px (bound %.3e), trans off "
              "by %.3e" % (i, inf["iou"], float(z[p + "iou"]), float(z[p + "iou_margin"]), exyz, bw, euv, buv, etr))
        assert exyz <= bw and euv <= buv
        assert inf["scene_ymin"] == z[p + "scene_ymin"]
        assert (inf["iou"] < 0.7) == low and abs(inf["iou"] - float(z[p + "iou"])) < 1e-3
        assert got["yaw"].shape == (1,) and got["yaw"][0] == float(z[p + "yaw"])
        assert got["trans"].dtype == z[p + "trans"].dtype
        if low:
            assert etr <= bw / float(z[p + "scale"]) + 1e-6
        else:
            assert np.array_equal(got["trans"], z[p + "trans"])
        assert got["scale"][0] == poses[j]["scale"] and np.array_equal(got["latent"], z[p + "latent"])
        assert np.array_equal(poses[j]["rot"], z[p + "rot"])                    # the caller's pose is left alone
    assert sides == {True, False}


# ---- the frame ---------------------------------------------------------------------------------------------------------------------------

def _synthetic_frame(dec32, n=8, area=32, D=40):
    """a frame of n annotations from fixtures.kitti_like_problems: one camera for the frame, every annotation's box placed so that the
    box-cornered intrinsics are its crop's own intrinsics scaled to the camera's focal length, the depth crop made from its lidar cloud"""
    from sdflabel_amd.fixtures import kitti_like_problems
    shapes, Ks, targets, lidars, starts = kitti_like_problems(dec32, D, area, n, DEV)
    K_orig = np.array([[720.0, 0, 600.0], [0, 720.0, 180.0], [0, 0, 1]], np.float32)
    annos = []
    for b in range(n):
        H, W = shapes[b]
        r = 720.0 / float(Ks[b][0, 0])
        Hc, Wc = int(round(H * r)), int(round(W * r))
        l, t = int(round(600.0 - float(Ks[b][0, 2]) * r)), int(round(180.0 - float(Ks[b][1, 2]) * r))
        p = lidars[b].astype(np.float64)
        u = (720.0 * p[:, 0] / p[:, 2] + 600.0 - l).astype(np.int32)
        v = (720.0 * p[:, 1] / p[:, 2] + 180.0 - t).astype(np.int32)
        ok = (u >= 0) & (u < Wc) & (v >= 0) & (v < Hc)
        depth = np.zeros((Hc, Wc), np.float32)
        depth[v[ok], u[ok]] = lidars[b][ok, 2]
        color = np.full((Hc, Wc, 3), 0.5, np.float32)
        annos.append({"bbox": [l, t, l + Wc, t + Hc], "color": color, "depth": depth, "nocs_pred": targets[b]})
    return annos, K_orig, [s["latent"] for s in starts]


def test_refine_frame_equals_the_hand_composed_stages_and_feeds_the_evaluator(dec32, dec16):
    import torch.nn.functional as F
    from sdflabel_amd.pipelines import detection_3d as D3
    from sdflabel_amd.pipelines import optimizer as OP
    from sdflabel_amd.pipelines.frame import refine_frame
    from sdflabel_amd.pipelines.pose import PoseEstimator
    annos, K_orig, latents = _synthetic_frame(dec32)
    n = len(annos)
    grid = sdflabel_amd.Grid3D(40, DEV)
    p_WC = np.eye(4)
    p_WC[:3, 3] = [0.1, -0.2, 0.3]
    W8 = {"2d": 0.3, "3d": 0.5}
    iters = 10
    OP.clear_refiner_cache()
    est, kept, st = refine_frame(annos, dec16, grid, latents, K_orig, p_WC, iters, W8, seed=7, return_stages=True)
    print("refine_frame: %d of %d annotations kept; lidar points per crop %s; NOCS points per crop %s" %
          (len(kept), n, [int(x[0].shape[0]) for x in st["lidar"]], [int(x[0].shape[0]) for x in st["nocs_3d"]]))
    assert len(kept) >= n // 2, "the synthetic frame should give most annotations a RANSAC pose"
    # by hand
    sizes, intr, off = zip(*[rtools.adjust_intrinsics_crop(K_orig, torch.Tensor(a["depth"].shape), a["bbox"], 32 ** 2) for a in annos])
    depths = [torch.from_numpy(a["depth"]) for a in annos]
    lidar = FR.reproject_many([a["color"] for a in annos], depths, off, filter=False)
    resized = [F.interpolate(a["nocs_pred"].unsqueeze(0), size=a["depth"].shape, mode="nearest").squeeze(0) for a in annos]
    nocs3d = FR.reproject_many(resized, depths, off, filter=True)
    surf = FR.surfaces_many(dec16, grid, latents)
    poses = PoseEstimator("kabsch", 2.0).estimate_many([(surf[i][0], surf[i][1], nocs3d[i][0], nocs3d[i][1]) for i in range(n)], seed=7)
    params = FR.init_params_many(poses, [s[0] for s in surf], [p[0] for p in nocs3d], [a["bbox"] for a in annos], K_orig, latents)
    keep = [i for i in range(n) if params[i] is not None]
    refined = OP.optimize_many([(params[i], annos[i]["nocs_pred"], lidar[i][0].cpu().numpy(), intr[i].to(DEV), sizes[i]) for i in keep], iters, dec16,
                               grid, DEV, W8)
    labels = FR.labels_many(dec16, grid, refined, p_WC, [annos[i]["bbox"] for i in keep])
    hand = FR.frame_dict(labels)
    assert keep == kept and [p is None for p in poses] == [p is None for p in st["poses"]]
    for i in range(n):
        assert torch.equal(lidar[i][0], st["lidar"][i][0]) and torch.equal(nocs3d[i][0], st["nocs_3d"][i][0])
    for a, b in zip(refined, st["params"]):
        for k in ("yaw", "trans", "scale", "latent"):
            assert torch.equal(a[k], b[k]), k
    assert hand["name"] == est["name"] == ["Car"] * len(kept)
    for k in FR.NECESSARY_KEYS:
        assert hand[k].dtype == est[k].dtype and hand[k].tobytes() == est[k].tobytes(), k
    assert est["location"].shape == (len(kept), 3) and np.isfinite(est["location"]).all() and np.isfinite(est["dimensions"]).all()
    # the evaluator takes the dict as a frame's estimations
    gt = {k: (list(v) if k == "name" else np.array(v, dtype=np.float64)) for k, v in est.items()}
    gt["name"] = np.asarray(gt["name"])
    gt["occluded"], gt["truncated"] = np.zeros(len(kept), np.int64), np.zeros(len(kept))
    from tests import _eval_golden as GD
    g17 = GD.load()                                   # (the class table and thresholds of the evaluator's golden: the reference's constants)
    ev = D3.Detection3DEvaluator(D3.clean_kitti_data, GD.id_to_name(g17), g17["overlap_thresholds"], g17["dist_thresholds"], compute_nuscenes=False,
                                 coordinate_frame=D3.CoordinateFrame.CAMERA)
    text, result = ev.evaluate_detection_3d([gt], [est], ["Car"], difficulties=[0])
    print(text)
    assert isinstance(text, str) and isinstance(result, dict) and len(result) > 0
