"""The synthetic bootstrap crops without a GPU: the numpy restatement (tests/_synth_ref.py) against what can be said without it -- the
analytic shading of a sphere, the occlusion rules within and across scenes --, the header csrc/synth_cells.h compiled for the host and
compared with the restatement bit for bit (once more under the address and undefined-behaviour sanitizers), the scene draws, and the
agreement of header, ctypes table and library on the new exports."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import _export_ref as ER
from tests import _synth_cases as SC
from tests import _synth_ref as SR
from tests import _verify_ref as VR
from tests._util import build_host_program

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
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


@pytest.fixture(scope="module")
def sphere():
    b, centre, radius = SC.sphere_batch()
    return b, restate(b)[0], centre, radius


# ---- the restatement against what can be said without it -------------------------------------------------------------------------------------

def test_sphere_shading_equals_the_analytic_lambert_term(sphere):
    """A sphere of radius r at z = 10 r whose mesh carries the exact vertex normals (p - c) / |p - c|, ks = 0, white: at every covered pixel
    whose ray meets the analytic sphere at Y with n_true . v >= 0.3, byte / 255 is ambient + kd max(0, n_true . l) within

        kd (asin(h / rho) + delta tan(theta) / rho) + 0.5 / 255,

    h the longest edge of the mesh, delta = max over the vertices of ||p - c| - r| plus the sagitta h^2 / (8 (r - dv)) of a chord of length h
    (how far the mesh's surface is from the sphere), rho = r - delta, tan(theta) = sqrt(1 - 0.3^2) / 0.3:
      * the ray meets the winning triangle at X, within h of each of its vertices p_i, which lie at least rho from c: the direction of each
        p_i - c, i.e. each vertex normal, is within asin(h / rho) of the direction of X - c, and so is the normalised positive combination
        of the three that the shader forms                                                                   (normal deviation of order h / r)
      * X and Y lie on one ray with |X - c| within delta of r; the ray makes the angle theta with the normal, so |X - Y| <= delta / cos(theta)
        and its part across the radial direction is at most delta tan(theta): the directions of X - c and Y - c differ by at most
        delta tan(theta) / rho
      * max(0, n . l) is 1-Lipschitz in n for a unit l, kd scales it, the albedo is 1; the byte adds half a step; the float64 arithmetic
        nothing at this scale.
    The pixels left out -- covered, but no analytic hit with n_true . v >= 0.3: the rim -- are at most 10 % of the covered ones (n . v < 0.3
    is 0.3^2 = 9 % of a distant sphere's disc)."""
    b, r, c, rad = sphere
    K, (W, H) = b["K"], b["size"]
    v, f = (np.asarray(a) for a in b["meshes"][0])
    P = v.astype(np.float64)[f]
    h = max(np.linalg.norm(P[:, i] - P[:, (i + 1) % 3], axis=1).max() for i in range(3))
    dv = np.abs(np.linalg.norm(v.astype(np.float64) - c, axis=1) - rad).max()
    delta = dv + h * h / (8.0 * (rad - dv))
    rho = rad - delta
    light, amb, kd = b["light"][0, :3], b["light"][0, 3], b["light"][0, 4]
    bound = kd * (np.arcsin(h / rho) + delta * (np.sqrt(1 - 0.09) / 0.3) / rho) + 0.5 / 255.0
    ys, xs = np.mgrid[0:H, 0:W]
    d = np.stack([(xs - K[2]) / K[0], (ys - K[3]) / K[1], np.ones(xs.shape)], -1)
    d = d / np.linalg.norm(d, axis=-1)[..., None]
    bq = (d * c).sum(-1)
    disc = bq * bq - ((c * c).sum() - rad * rad)
    hit = disc > 0
    t = bq - np.sqrt(np.where(hit, disc, 0.0))
    n_true = (t[..., None] * d - c) / rad
    ndv = -(n_true * d).sum(-1)
    want = amb + kd * np.maximum(0.0, (n_true * light).sum(-1))
    covered = r["mask"] != 0
    use = covered & hit & (ndv >= 0.3)
    got = r["rgb"].astype(np.float64) / 255.0
    err = np.abs(got[use] - want[use][:, None])
    rim = covered & ~use
    print("sphere: %d covered pixels, %d compared, rim %d (%.2f %%); h = %.4g, r = %.4g, delta = %.3g; max |byte / 255 - analytic| %.4g, bound %.4g"
          % (covered.sum(), use.sum(), rim.sum(), 100.0 * rim.sum() / covered.sum(), h, rad, delta, err.max(), bound))
    assert covered.sum() > 1000 and want[use].max() - want[use].min() > 0.5            # lit and unlit sides are both in sight
    assert rim.sum() <= 0.10 * covered.sum()
    assert err.max() <= bound
    assert (r["rgb"][..., 0] == r["rgb"][..., 1]).all() and (r["rgb"][..., 1] == r["rgb"][..., 2]).all() and r["flag"] == 0
    # the interpolated normal itself, for the record: against the same angle
    nn = r["normal"][use]
    ang = np.arccos(np.clip((nn * n_true[use]).sum(-1), -1, 1))
    print("normal: max angle %.4g, bound %.4g" % (ang.max(), (bound - 0.5 / 255.0) / kd))
    assert ang.max() <= (bound - 0.5 / 255.0) / kd


def test_owner_rules(batches, refs):
    # scene == NULL is the export's owner
    for name in ("occluder_at_another_offset", "occluder_window_short", "depth_tie", "one_pixel_box_and_whole_window"):
        rs = refs[name]
        want = ER.owner([r["mask"] for r in rs], [r["depth"] for r in rs], batches[name]["windows"])
        for r, w in zip(rs, want):
            assert r["owner"].dtype == np.int32 and r["owner"].tobytes() == w.tobytes(), name
    # two identical meshes in one scene: the lower index owns wherever both windows hold the pixel
    b = batches["one_pixel_box_and_whole_window"]
    a0, a1 = refs["one_pixel_box_and_whole_window"]
    l, t, r_, bt = b["windows"][1]
    sub = a0["mask"][t:bt, l:r_] != 0
    assert sub.sum() > 300 and np.array_equal(a1["mask"] != 0, sub)
    assert (a0["owner"][a0["mask"] != 0] == 0).all() and (a1["owner"][sub] == 0).all() and (a1["owner"][~sub] == -1).all()
    # the same two in different scenes: each owns itself, and each one's rgb is its solo render
    two = dict(b, scene=[0, 1], light=np.concatenate([b["light"], b["light"]]), ramp=np.concatenate([b["ramp"], b["ramp"]]))
    s0, s1 = restate(two)
    assert (s0["owner"][s0["mask"] != 0] == 0).all() and (s1["owner"][s1["mask"] != 0] == 1).all()
    for i, s in enumerate((s0, s1)):
        solo = dict(b, meshes=b["meshes"][i:i + 1], normals=b["normals"][i:i + 1], windows=b["windows"][i:i + 1], boxes=b["boxes"][i:i + 1],
                    paint=b["paint"][i:i + 1])
        (want,) = restate(solo)
        assert s["rgb"].tobytes() == want["rgb"].tobytes() and s["rgb"].any()
    assert a1["rgb"].tobytes() != s1["rgb"].tobytes()                                     # (in one scene it shows the other's paint)
    # scenes that overlap in pixel space do not see each other; within scene 0 the near triangle hides the far one
    far, other, near = refs["two_scenes"]
    wl, wt, wr, wb = batches["two_scenes"]["windows"][2]
    nm = np.zeros(far["mask"].shape, bool)
    nm[wt:wb, wl:wr] = near["mask"] != 0
    fm = far["mask"] != 0
    assert (fm & nm).sum() > 100 and np.array_equal(far["owner"], np.where(fm, np.where(nm, 2, 0), -1))
    assert (other["owner"][other["mask"] != 0] == 1).all() and (other["mask"] != 0).sum() > 100


def test_background_and_paint(batches, refs):
    b, (far, other, near) = batches["two_scenes"], refs["two_scenes"]
    # scene 1 shows image 1 exactly where nothing of it covers; scene 0 (index 7: outside the images) its ramp
    l, t, r, bt = b["boxes"][1]
    free = other["mask"][t - b["windows"][1][1]:bt - b["windows"][1][1], l - b["windows"][1][0]:r - b["windows"][1][0]] == 0
    assert free.sum() > 100 and (other["rgb"][free] == b["bgs"][1][t:bt, l:r][free]).all()
    l, t, r, bt = b["boxes"][0]
    free = far["mask"][t:bt, l:r] == 0
    ys, xs = np.nonzero(free)
    assert (far["rgb"][free] == SR.ramp_bytes(b["ramp"][0], SC.H, xs + l, ys + t)).all() and np.isnan(far["val"][free]).all()
    # the ramp: without noise it runs from the top colour to the bottom colour; the noise stays within amp / 2
    ramp = np.array([10, 200, 30, 250, 20, 90, 0, 5], np.int32)
    col = SR.ramp_bytes(ramp, 48, np.zeros(48, np.int64), np.arange(48))
    assert col[0].tolist() == [10, 200, 30] and col[47].tolist() == [250, 20, 90] and col[1].tolist() == [10 + 240 // 47, 200 - 180 // 47, 30 + 60 // 47]
    ramp[6] = 40
    noisy = SR.ramp_bytes(ramp, 48, np.arange(48), np.arange(48)).astype(np.int64)
    d = noisy - SR.ramp_bytes(np.where(np.arange(8) == 6, 0, ramp), 48, np.arange(48), np.arange(48))
    assert d.min() >= -20 and d.max() <= 19 and len(np.unique(d)) > 10
    assert SR.ramp_bytes(ramp, 1, np.arange(5), np.zeros(5, np.int64)).shape == (5, 3)          # one row: the denominator is 1
    # zero and NaN normals: the colour is albedo * ambient
    z = refs["zero_and_nan_normal"][0]
    bz = batches["zero_and_nan_normal"]
    seen = ~np.isnan(z["val"][..., 0])
    flat = ER.byte(255.0 * (bz["paint"][0, :3] * bz["light"][0, 3]))
    assert seen.sum() > 500 and (z["rgb"][seen] == flat).all() and z["flag"] == 0
    # shin 0, shin 7, ks = 0 under one light: the same diffuse term; the highlight narrows with shin and vanishes with ks = 0
    s0, s7, k0 = (r["val"] for r in refs["shin_0_7_and_ks_0"])
    m = ~np.isnan(s0[..., 0])
    assert m.sum() > 500 and (s0[m] >= s7[m]).all() and (s7[m] >= k0[m]).all() and (s0[m] > k0[m]).any()


# ---- the header on the host --------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    return build_host_program(tmp_path_factory.mktemp("synth_host"), "synth_host/synth_host.cpp", "synth_host")


def run_host(exe, b, tmp, qoff=None):
    B = len(b["meshes"])
    W, H = b["size"]
    vs, fs = [m[0] for m in b["meshes"]], [m[1] for m in b["meshes"]]
    wins, boxes = np.asarray(b["windows"], np.int32).reshape(-1, 4), np.asarray(b["boxes"], np.int32).reshape(-1, 4)
    voff = np.concatenate([[0], np.cumsum([len(v) for v in vs])]).astype(np.int64)
    toff = np.concatenate([[0], np.cumsum([len(f) for f in fs])]).astype(np.int64)
    P = int(((wins[:, 2] - wins[:, 0]) * (wins[:, 3] - wins[:, 1])).sum())
    areas = (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])
    Q = int(areas.sum())
    S, NBG = len(b["light"]), 0 if b["bgs"] is None else len(b["bgs"])
    src, dst = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(src, "wb") as fh:
        fh.write(np.array([B, W, H, S, NBG, int(b["scene"] is not None), int(b["triangles"] is not None), int(qoff is not None)], np.int32).tobytes())
        fh.write(np.array([0.1], np.float32).tobytes() + np.asarray(b["K"], np.float64).tobytes())
        parts = [voff, toff, wins, boxes]
        if b["scene"] is not None:
            parts.append(np.asarray(b["scene"], np.int32))
        if qoff is not None:
            parts.append(np.asarray(qoff, np.int64))
        parts += [np.asarray(b["paint"], np.float64), np.asarray(b["light"], np.float64), np.asarray(b["ramp"], np.int32)]
        if NBG:
            parts += [np.asarray(b["bg_index"], np.int32), np.stack(b["bgs"]).astype(np.uint8)]
        parts += [np.concatenate(vs).astype(np.float32), np.concatenate(b["normals"]).astype(np.float32), np.concatenate(fs).astype(np.int32)]
        for a in parts:
            fh.write(np.ascontiguousarray(a).tobytes())
        if b["triangles"] is not None:
            ras = [VR.raster(vs[i], fs[i], b["K"], wins[i], 0.1)[2] for i in range(B)]
            fh.write(np.concatenate([np.asarray(ras[i] if t is None else t, np.int32).reshape(-1) for i, t in enumerate(b["triangles"])]).tobytes())
    r = subprocess.run([exe, src, dst], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    raw = open(dst, "rb").read()
    o, out = 0, []
    for dt, n in ((np.int32, P), (np.uint8, 3 * Q), (np.int32, B)):
        out.append(np.frombuffer(raw, dt, n, o))
        o += n * np.dtype(dt).itemsize
    assert o == len(raw)
    return out, areas


def check_host(out, areas, rs, name):
    owner, rgb, flags = out
    po = qo = 0
    for i, r in enumerate(rs):
        assert owner[po:po + r["owner"].size].tobytes() == r["owner"].tobytes(), name
        po += r["owner"].size
        n = 3 * int(areas[i])
        assert rgb[qo:qo + n].tobytes() == r["rgb"].tobytes(), (name, i)
        qo += n
        assert flags[i] == r["flag"], (name, i)


def check_all(exe, tmp, batches, refs):
    ran = {}
    for name, b in batches.items():
        out, areas = run_host(exe, b, tmp)
        check_host(out, areas, refs[name], name)
        ran[name] = out[2].tolist()
    for name in INVALID_FIRST:                       # flag bit 1, zeros, and the annotation beside it -- in another scene -- untouched
        assert ran[name] == [SR.FLAG_INVALID, 0] and not refs[name][0]["rgb"].any() and refs[name][1]["rgb"].any(), name
    assert all(f == [0] * len(f) for n, f in ran.items() if n not in INVALID_FIRST)
    # an offset table that does not fit: both annotations flagged, every byte zero; a last offset beyond Q: that annotation alone
    b, want = batches["occluder_at_another_offset"], refs["occluder_at_another_offset"]
    q = [0, 64 * 48, 64 * 48 + 26 * 24]
    (owner, rgb, flags), areas = run_host(exe, b, tmp, qoff=[0, q[1] - 1, q[2]])
    assert flags.tolist() == [SR.FLAG_INVALID] * 2 and not rgb.any()
    (owner, rgb, flags), areas = run_host(exe, b, tmp, qoff=[0, q[1], q[2] + 5])
    assert flags.tolist() == [0, SR.FLAG_INVALID] and rgb[:3 * q[1]].tobytes() == want[0]["rgb"].tobytes() and not rgb[3 * q[1]:].any()
    return ran


def test_header_on_the_host_reproduces_the_restatement(host_program, tmp_path, batches, refs, sphere):
    check_all(host_program, str(tmp_path), batches, refs)
    out, areas = run_host(host_program, sphere[0], str(tmp_path))
    check_host(out, areas, [sphere[1]], "sphere")


def test_header_on_the_host_under_the_sanitizers(tmp_path, batches, refs):
    """exact-size buffers: an index outside a window, a box, a mesh, a table or a background image is an error here"""
    exe = build_host_program(tmp_path, "synth_host/synth_host.cpp", "synth_host_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    ran = check_all(exe, str(tmp_path), batches, refs)
    assert ran["empty_window"] == [0] and ran["empty_mesh"] == [0] and ran["one_row_image"] == [0]


# ---- the scene draws ------------------------------------------------------------------------------------------------------------------------------

def test_draw_scenes():
    import torch
    from sdflabel_amd import synth
    K, size = (720.0, 710.0, 600.5, 180.25), (1242, 375)
    kw = dict(max_objects=4, scale_range=(1.2, 2.0), z_near=6.0, z_far=30.0, border=0.1, n_backgrounds=3, jitter=0.15, shin_range=(1, 5))
    a = synth.draw_scenes(torch.Generator().manual_seed(11), 6, 5, K, size, **kw)
    g = torch.Generator().manual_seed(11)
    torch.rand(7, generator=g)                                                            # the generator's state does not matter, its seed does
    b = synth.draw_scenes(g, 9, 5, K, size, **kw)
    assert a == b[:6] and len(b) == 9                                                     # the same bits; unchanged when n_scenes grows
    assert synth.draw_scenes(torch.Generator().manual_seed(11), 2, 5, K, size, first_scene=4, **kw) == a[4:6]
    other = synth.draw_scenes(torch.Generator().manual_seed(12), 6, 5, K, size, **kw)
    assert all(x != y for x, y in zip(a, other))
    n_obj, blends = [], 0
    for s in b:
        n_obj.append(len(s["objects"]))
        l = np.asarray(s["light"])
        assert abs((l * l).sum() - 1.0) < 1e-12 and l[1] < 0 and l[2] < 0 and 0.15 <= s["ambient"] <= 0.4 and 0.5 <= s["kd"] <= 0.9
        assert s["background"] in (0, 1, 2) and len(s["ramp"]) == 8 and all(0 <= x <= 255 for x in s["ramp"][:6]) and 0 <= s["ramp"][6] <= 48
        for o in s["objects"]:
            assert 0.1 * size[0] <= o["u"] <= 0.9 * size[0] and 0.1 * size[1] <= o["v"] <= 0.9 * size[1]          # the centre is inside the image
            assert -np.pi <= o["yaw"] < np.pi and 1.2 <= o["scale"] <= 2.0 and 6.0 <= o["z"] <= 30.0
            assert 1 <= o["shin"] <= 5 and all(abs(j) <= 0.15 for j in o["jitter"]) and all(0.1 <= x <= 0.9 for x in o["albedo"])
            T = synth._cam_T(o["yaw"], o["trans"], o["scale"])
            corners = synth._cube_corners(T, np.float32(o["scale"]))
            assert corners[:, 2].min() > 0.1                                              # every cube corner beyond z_min
            centre = T[:3, 3]
            assert abs(720.0 * centre[0] / centre[2] + 600.5 - o["u"]) < 1e-3 and abs(710.0 * centre[1] / centre[2] + 180.25 - o["v"]) < 1e-3
            l_, t_, r_, b_ = synth.cube_window(T, np.float32(o["scale"]), K, size)
            assert 0 <= l_ < r_ <= size[0] and 0 <= t_ < b_ <= size[1] and l_ <= o["u"] < r_ and t_ <= o["v"] < b_
            blends += isinstance(o["latent"], tuple)
            idx = o["latent"][:2] if isinstance(o["latent"], tuple) else (o["latent"],)
            assert all(0 <= i < 5 for i in idx)
    assert 1 <= min(n_obj) and max(n_obj) <= 4 and len(set(n_obj)) > 1 and blends > 0
    with pytest.raises(ValueError):                                                       # no room beyond z_min
        synth.draw_scenes(torch.Generator().manual_seed(1), 1, 5, K, size, scale_range=(30.0, 31.0), z_near=6.0, z_far=7.0)
    # the crop's box: the tight box moved by the jitter, clipped to the window, never empty
    assert synth.jittered_box((10, 10, 30, 20), (0.1, -0.2, 0.25, 0.0), (0, 0, 33, 48)) == (8, 12, 33, 20)
    assert synth.jittered_box((10, 10, 12, 12), (-0.9, -0.9, -0.9, -0.9), (0, 0, 64, 48)) == (10, 10, 12, 12)


# ---- header, ctypes table, library, Python side ------------------------------------------------------------------------------------------------

def test_abi_has_the_synth_entry_points():
    from sdflabel_amd import _lib
    header = open(os.path.join(ROOT, "include", "sdfr.h")).read()
    h = _lib.lib()
    for name in ("sdfr_synth_owner", "sdfr_synth_shade"):
        assert name in _lib.EXPORTS and hasattr(h, name) and re.search(r"\bint %s\(" % name, header), name
    assert int(re.search(r"#define SDFR_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION == h.sdfr_version() >= 414
    build = open(os.path.join(ROOT, "sdflabel_amd", "csrc", "build.sh")).read()
    assert re.search(r"-ffp-contract=off -c \"\$HERE/synth\.hip\"", build)


def test_argument_checks_come_before_any_launch():
    import ctypes
    from sdflabel_amd import _lib
    h = _lib.lib()
    k = (ctypes.c_double * 4)(8, 8, 32, 24)
    N = None
    assert h.sdfr_synth_owner(N, N, N, N, 10, N, 1, 64, 48, N, N) == -1 and b"NULL" in h.sdfr_last_error()
    assert h.sdfr_synth_owner(N, N, N, N, 0, N, 0, 64, 48, N, N) == 0
    assert h.sdfr_synth_owner(N, N, N, N, 64 * 48 + 1, N, 1, 64, 48, N, N) == -1 and b"out of range" in h.sdfr_last_error()

    def shade(V=0, T=0, P=0, Q=0, S=1, NBG=0, B=1, K=k, z=0.1):
        return h.sdfr_synth_shade(N, V, N, T, N, N, N, N, N, P, N, N, N, N, N, Q, N, N, S, N, N, NBG, N, B, 64, 48, K, z, N, N, N)
    assert shade() == -1 and b"NULL" in h.sdfr_last_error()
    assert shade(B=0) == 0
    assert shade(S=0) == -1 and b"scene" in h.sdfr_last_error()
    assert shade(NBG=2) == -1 and b"background" in h.sdfr_last_error()
    assert shade(K=None) == -1 and b"intrinsics" in h.sdfr_last_error()
    assert shade(z=-1.0) == -1
    assert shade(P=10, Q=11) == -1 and b"out of range" in h.sdfr_last_error()


def test_python_side_without_a_gpu(tmp_path):
    import torch
    from sdflabel_amd import synth
    from sdflabel_amd.mesh import Mesh
    v = torch.tensor([[0.0, 0, 0], [0.5, 0, 0], [0, 0.5, 0]])
    scene = [{"index": 0, "light": [0, -0.6, -0.8], "ambient": 0.2, "kd": 0.7, "background": None, "ramp": [0] * 8,
              "objects": [{"latent": 0, "yaw": 0.3, "scale": 1.5, "trans": [0.0, 0.0, 8.0], "albedo": [0.5] * 3, "ks": 0.1, "shin": 3, "jitter": [0] * 4}]}]
    T = synth._cam_T(0.3, [0.0, 0.0, 8.0], 1.5)
    lat = torch.zeros((1, 3))
    bare = Mesh(v, torch.zeros((1, 3), dtype=torch.int32), scale=1.5, cam_T=T)
    with pytest.raises(ValueError) as e:
        synth.scenes_many(None, lat, scene, SC.K_ODD, (SC.W, SC.H), meshes=([bare], lat))    # a mesh without normals
    assert "normals" in str(e.value)
    with pytest.raises(ValueError):
        synth.scenes_many(None, lat, scene, SC.K_ODD, (SC.W, SC.H), meshes=([], lat))
    with pytest.raises(ValueError):                                                       # a cube corner behind z_min
        synth.cube_window(synth._cam_T(0.0, [0.0, 0.0, 0.5], 1.5), 1.5, SC.K_ODD, (SC.W, SC.H))
    assert synth.scenes_many(None, lat, [], SC.K_ODD, (SC.W, SC.H)) == ([], {"kept": [], "dropped": [], "area": []})
    from sdflabel_amd.pipelines.synth_crops import bootstrap_crops
    with pytest.raises(ValueError):
        bootstrap_crops(None, lat, tmp_path / "crops", 0, SC.K_ODD, (SC.W, SC.H))
