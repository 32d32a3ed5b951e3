"""The training-crop export without a GPU: the numpy restatement (tests/_export_ref.py) against what can be said without it -- the
unprojection identity on the sphere, the analytic ray-box intersection of a posed cube, the occlusion rules, the loader's mask --, the
header csrc/crop_cells.h compiled for the host and compared with the restatement bit for bit (once more under the address and
undefined-behaviour sanitizers), the writer's round trip through datasets.crops.Crops, and the agreement of header, ctypes table and
library on the new exports."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

from tests import _export_cases as EC
from tests import _export_ref as ER
from tests import _verify_cases as VC
from tests import _verify_ref as VR
from tests._util import build_host_program

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def restate(b):
    return ER.export(b["meshes"], b["attrs"], b["K"], b["windows"], b["boxes"], 0.1, b["occlusion"], b["colors"], b["triangles"])


@pytest.fixture(scope="module")
def batches():
    return EC.batches()


@pytest.fixture(scope="module")
def refs(batches):
    """name -> the restatement's result per annotation; computed once, never modified"""
    return {n: restate(b) for n, b in batches.items()}


@pytest.fixture(scope="module")
def sphere():
    b, scale, yaw, trans = EC.sphere_batch()
    return b, restate(b)[0], scale, yaw, trans


# ---- the restatement against what can be said without it -------------------------------------------------------------------------------------

def unprojection_errors(uvw, mask, depth, K, window, pose):
    """|decoded bytes - point_x(pixel unprojected at the raster's depth)| per covered pixel and coordinate"""
    ys, xs = np.nonzero(mask)
    d = depth[ys, xs].astype(np.float64)
    px, py = xs + float(window[0]), ys + float(window[1])
    pc = np.stack([(px - K[2]) / K[0] * d, (py - K[3]) / K[1] * d, d], 1).astype(np.float32)
    x, _ = VR.point_x(pc, pose)
    dec = uvw[ys, xs].astype(np.float64) / 127.5 - 1.0
    return np.abs(dec - x.astype(np.float64)), x


def test_sphere_bytes_satisfy_the_unprojection_identity(sphere):
    """every covered pixel, decoded as byte / 127.5 - 1, is the lattice point its own ray and depth give, within half a quantisation step
    (1 / 255, exact) plus the float32 term ER.shade_bound derives"""
    b, r, scale, yaw, trans = sphere
    pose = VR.pose_row(np.cos(np.float32(yaw)), np.sin(np.float32(yaw)), trans, scale)
    err, x = unprojection_errors(r["uvw"], r["mask"], r["depth"], b["K"], b["windows"][0], pose)
    bound = ER.shade_bound(scale, trans)
    # the unquantised values, for the record
    ys, xs = np.nonzero(r["mask"])
    tr = r["triangle"][ys, xs]
    v, f = b["meshes"][0]
    P = np.asarray(v, np.float32)[np.asarray(f)[tr]]
    u = np.stack([VR.project(b["K"][0], b["K"][2], P[:, i, 0], P[:, i, 2]) for i in range(3)], 1)
    w = np.stack([VR.project(b["K"][1], b["K"][3], P[:, i, 1], P[:, i, 2]) for i in range(3)], 1)
    val, c = ER.shade_values((u, w, P[:, :, 2].astype(np.float64)), xs, ys, b["attrs"][0][np.asarray(f)[tr]])
    raw = np.abs(c - x.astype(np.float64)).max()
    zero = int((ER.byte(val) == 0).all(1).sum())
    print("sphere: %d covered pixels; unquantised |c - x| max %.3g (float32 bound %.3g); quantised max %.9g = 1/255 %+.3g; all-zero pixels %d; "
          "nearest rounding boundary %.3g" % (len(ys), raw, bound, err.max(), err.max() - 1 / 255.0, zero,
                                              np.abs(val - np.floor(val) - 0.5).min()))
    assert len(ys) > 1000 and r["counts"].tolist() == [VC.W * VC.H, len(ys), len(ys), 0]
    assert raw <= bound
    assert err.max() <= 1.0 / 255.0 + bound
    assert zero == 0


def analytic_cube(K, h, scale, trans):
    """val float64 [H][W][3] and hit bool [H][W] of the cube [-h, h]^3 of the lattice frame posed by diag(1, -1, 1) scale a + trans: the
    slab intersection of every pixel's ray, in float64"""
    ys, xs = np.mgrid[0:VC.H, 0:VC.W]
    d = np.stack([(xs - K[2]) / K[0], (ys - K[3]) / K[1], np.ones(xs.shape)], -1)        # camera ray lambda d
    s = np.array([1.0, -1.0, 1.0])
    o = -np.asarray(trans, np.float64) * s / scale                                        # lattice point = o + lambda dl
    dl = d * s / scale
    with np.errstate(all="ignore"):
        t0, t1 = (-h - o) / dl, (h - o) / dl
    lo, hi = np.minimum(t0, t1), np.maximum(t0, t1)
    par = dl == 0.0
    inside = (o >= -h) & (o <= h)
    lo = np.where(par, np.where(inside, -np.inf, np.inf), lo)
    hi = np.where(par, np.where(inside, np.inf, -np.inf), hi)
    near, far = lo.max(-1), hi.min(-1)
    hit = (near <= far + 1e-12) & (near > 0)
    with np.errstate(all="ignore"):
        a = o + np.where(hit, near, 0.0)[..., None] * dl
    return (a + 1.0) * 127.5, hit


def test_posed_cube_equals_the_analytic_ray_box_intersection(batches, refs):
    b, r = batches["posed_cube"], refs["posed_cube"][0]
    val, hit = analytic_cube(b["K"], **EC.POSE_CUBE)
    mask = r["mask"] != 0
    assert np.array_equal(mask, hit) and mask.sum() > 1000
    faces_seen = int((np.bincount(r["triangle"][mask] // 2, minlength=6) >= 50).sum())
    want = ER.byte(val)
    close = (np.abs(val - np.floor(val) - 0.5) <= 1e-6)                                 # the analytic value sits on a rounding boundary
    got = r["uvw"].astype(np.int64)
    diff = np.abs(got - want.astype(np.int64))
    excepted = (close & mask[..., None]).any(-1)
    share = excepted.sum() / float(mask.sum())
    print("posed cube: %d covered pixels, %d faces in sight, %d pixels (%.3f %%) within 1e-6 of a rounding boundary, max byte difference %d there, "
          "%d elsewhere" % (mask.sum(), faces_seen, excepted.sum(), 100 * share, diff[excepted].max() if excepted.any() else 0,
                            diff[mask & ~excepted].max()))
    assert faces_seen == 3
    assert share <= 0.01
    assert (diff[mask][~close[mask]] == 0).all() and (diff[mask] <= 1).all()
    assert (got[~mask] == 0).all() and (got[mask].sum(-1) > 0).all()


def test_occlusion_cases(batches, refs):
    far, near = refs["near_over_far"]
    fm, nm = far["mask"] != 0, near["mask"] != 0
    assert (fm & nm).sum() > 100
    assert np.array_equal(far["owner"], np.where(fm, np.where(nm, 1, 0), -1))            # near (Z = 1) over far (Z = 2)
    assert np.array_equal(near["owner"], np.where(nm, 1, -1))
    assert (far["uvw"][fm & nm] == 0).all() and (far["uvw"][fm & ~nm].sum(-1) > 0).all()
    assert far["counts"].tolist() == [VC.W * VC.H, int(fm.sum()), int((fm & ~nm).sum()), 0]
    # an exact depth tie: the lower index wins
    a, b = refs["depth_tie"]
    wa, wb = batches["depth_tie"]["windows"]
    am, bm = np.zeros((VC.H, VC.W), bool), np.zeros((VC.H, VC.W), bool)
    am[wa[1]:wa[3], wa[0]:wa[2]] = a["mask"] != 0
    bm[wb[1]:wb[3], wb[0]:wb[2]] = b["mask"] != 0
    both = am & bm
    assert both.sum() > 50 and (a["depth"][a["mask"] != 0] == 2).all() and (b["depth"][b["mask"] != 0] == 2).all()
    assert (a["owner"][a["mask"] != 0] == 0).all()
    ob = np.full((VC.H, VC.W), -9)
    ob[wb[1]:wb[3], wb[0]:wb[2]] = b["owner"]
    assert (ob[both] == 0).all() and (ob[bm & ~am] == 1).all()
    # an occluder whose window does not reach the pixel is not seen
    far2, near2 = refs["occluder_window_short"]
    wl, wt, wr, wb_ = batches["occluder_window_short"]["windows"][1]
    inwin = np.zeros((VC.H, VC.W), bool)
    inwin[wt:wb_, wl:wr] = True
    assert (fm & nm & ~inwin).sum() > 50                                                 # the near triangle would cover these, outside its window
    assert (far2["owner"][fm & nm & ~inwin] == 0).all() and (far2["owner"][fm & nm & inwin] == 1).all()
    assert far2["counts"][2] == int((fm & ~(nm & inwin)).sum())
    # occlusion off: every covered pixel is shaded, and the bytes are those of the annotation alone
    off = refs["occlusion_off"][0]
    bb = batches["occlusion_off"]
    solo = ER.export(bb["meshes"][:1], bb["attrs"][:1], bb["K"], bb["windows"][:1], bb["boxes"][:1], 0.1, False)[0]
    assert off["owner"] is None and off["uvw"].tobytes() == solo["uvw"].tobytes() and (off["uvw"][fm].sum(-1) > 0).all()
    assert off["counts"].tolist() == [VC.W * VC.H, int(fm.sum()), int(fm.sum()), 0]


def test_loader_mask_is_the_set_of_labelled_pixels(batches, refs, sphere):
    """inside the box: rendered mask and owner == self  <=>  u + v + w > 0"""
    n = 0
    for name, rs in list(refs.items()) + [("sphere", [sphere[1]])]:
        b = batches[name] if name != "sphere" else sphere[0]
        for i, r in enumerate(rs):
            if r["counts"][3] & ER.FLAG_INVALID:
                assert not r["uvw"].any(), name
                continue
            l, t = b["windows"][i][:2]
            bl, bt, br, bb = b["boxes"][i]
            sl = (slice(bt - t, bb - t), slice(bl - l, br - l))
            seen = (r["mask"][sl] != 0) if r["owner"] is None else (r["mask"][sl] != 0) & (r["owner"][sl] == i)
            assert np.array_equal(r["uvw"].astype(np.int64).sum(-1) > 0, seen), name
            assert r["counts"][2] == seen.sum(), name
            n += int(seen.sum())
    nan = refs["nan_vertex"][0]["uvw"]
    assert (nan[..., 0] == 0).all() and (nan[..., 1:].max() > 0)                         # a NaN value: byte 0
    zero = refs["zero_bytes"][0]["uvw"]
    assert (zero[10, 10:21] == [0, 0, 1]).all() and (zero[11, 10:20, 2] > 1).all() and not zero[..., :2].any()      # (0, 0, 0) -> (0, 0, 1)
    assert n > 5000


def test_rgb_bytes():
    k = np.arange(256, dtype=np.float32) / np.float32(255.0)
    bgr = np.stack([k, k[::-1], np.roll(k, 7)], 1)
    got = ER.rgb_bytes(bgr)
    assert got[:, 2].tolist() == list(range(256)) and got[:, 1].tolist() == list(range(255, -1, -1))         # k / 255 returns k; BGR -> RGB
    odd = np.array([[np.nan, -0.5, 1.5], [np.inf, -np.inf, 0.5 / 255], [1.5 / 255, 2.5 / 255, 1.0]], np.float32)
    assert ER.rgb_bytes(odd).tolist() == [[255, 0, 0], [0, 0, 255], [255, 2, 2]]                            # ties to even: 0.5 -> 0, 1.5 -> 2, 2.5 -> 2


# ---- the header on the host --------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    return build_host_program(tmp_path_factory.mktemp("export_host"), "export_host/export_host.cpp", "export_host")


def run_host(exe, b, tmp):
    B = len(b["meshes"])
    vs, fs = [m[0] for m in b["meshes"]], [m[1] for m in b["meshes"]]
    wins, boxes = np.asarray(b["windows"], np.int32).reshape(-1, 4), np.asarray(b["boxes"], np.int32).reshape(-1, 4)
    voff = np.concatenate([[0], np.cumsum([len(v) for v in vs])]).astype(np.int64)
    toff = np.concatenate([[0], np.cumsum([len(f) for f in fs])]).astype(np.int64)
    P = int(((wins[:, 2] - wins[:, 0]) * (wins[:, 3] - wins[:, 1])).sum())
    areas = (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])
    Q = int(areas.sum())
    src, dst = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(src, "wb") as fh:
        fh.write(np.array([B, VC.W, VC.H, int(b["occlusion"]), int(b["colors"] is not None), int(b["triangles"] is not None)], np.int32).tobytes())
        fh.write(np.array([0.1], np.float32).tobytes() + np.asarray(b["K"], np.float64).tobytes())
        for a in (voff, toff, wins, boxes, np.concatenate(vs).astype(np.float32), np.concatenate(b["attrs"]).astype(np.float32),
                  np.concatenate(fs).astype(np.int32)):
            fh.write(np.ascontiguousarray(a).tobytes())
        if b["colors"] is not None:
            fh.write(np.concatenate([np.asarray(c, np.float32).reshape(-1) for c in b["colors"]]).tobytes())
        if b["triangles"] is not None:
            ras = [VR.raster(vs[i], fs[i], b["K"], wins[i], 0.1)[2] for i in range(B)]
            fh.write(np.concatenate([np.asarray(ras[i] if t is None else t, np.int32).reshape(-1) for i, t in enumerate(b["triangles"])]).tobytes())
    r = subprocess.run([exe, src, dst], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    raw = open(dst, "rb").read()
    o, out = 0, []
    for dt, n in ((np.int32, P if b["occlusion"] else 0), (np.uint8, 3 * Q), (np.uint8, 3 * Q if b["colors"] is not None else 0), (np.int32, B),
                  (np.int32, 4 * B)):
        out.append(np.frombuffer(raw, dt, n, o))
        o += n * np.dtype(dt).itemsize
    assert o == len(raw)
    return out, areas


def check_host(out, areas, rs, name):
    owner, uvw, rgb, flags, counts = out
    po = qo = 0
    for i, r in enumerate(rs):
        if r["owner"] is not None:
            assert owner[po:po + r["owner"].size].tobytes() == r["owner"].tobytes(), name
            po += r["owner"].size
        n = 3 * int(areas[i])
        assert uvw[qo:qo + n].tobytes() == r["uvw"].tobytes(), name
        if r["rgb"] is not None:
            assert rgb[qo:qo + n].tobytes() == r["rgb"].tobytes(), name
        qo += n
        assert counts[4 * i:4 * i + 4].tolist() == r["counts"].tolist() and flags[i] == r["counts"][3], name


def test_header_on_the_host_reproduces_the_restatement(host_program, tmp_path, batches, refs, sphere):
    for name, b in batches.items():
        out, areas = run_host(host_program, b, str(tmp_path))
        check_host(out, areas, refs[name], name)
    out, areas = run_host(host_program, sphere[0], str(tmp_path))
    check_host(out, areas, [sphere[1]], "sphere")


def test_header_on_the_host_under_the_sanitizers(tmp_path, batches, refs):
    """exact-size buffers: an index outside a window, a box, a mesh or a colour crop is an error here"""
    exe = build_host_program(tmp_path, "export_host/export_host.cpp", "export_host_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    ran = {}
    for name, b in batches.items():
        out, areas = run_host(exe, b, str(tmp_path))
        check_host(out, areas, refs[name], name)
        ran[name] = out[3].tolist()
    # the cases in which only the predicates the kernels share keep the reads inside the buffers: triangle indices 7 and -3 for a mesh of one
    # triangle, a box that leaves its window (its offsets then fit no window pixel), an empty window, a mesh without triangles
    assert ran["bad_triangle_index"] == [ER.FLAG_INVALID, 0] and ran["box_outside_window"] == [ER.FLAG_INVALID, 0]
    assert ran["empty_window"] == [0] and ran["empty_mesh"] == [0]


# ---- the writer ------------------------------------------------------------------------------------------------------------------------------------

def _host_crop(rng, h, w, box):
    from sdflabel_amd.export import Crop
    return Crop(rng.integers(0, 256, (h, w, 3)).astype(np.uint8), rng.integers(0, 256, (h, w, 3)).astype(np.uint8), box, box,
                np.array([h * w, 0, 0, 0], np.int32), 0)


def test_crop_writer_round_trip_append_and_crash(tmp_path):
    pytest.importorskip("PIL")
    import torch
    from sdflabel_amd.datasets.crops import Crops
    from sdflabel_amd.export import CropWriter, crop_intrinsics
    rng = np.random.default_rng(5)
    path = tmp_path / "crops"
    K = np.array([[720.0, 0, 600.5], [0, 710.0, 180.25], [0, 0, 1]])
    crops = [_host_crop(rng, 17, 23, (100, 50, 123, 67)), _host_crop(rng, 9, 31, (7, 3, 38, 12)), _host_crop(rng, 12, 12, (0, 0, 12, 12))]
    lats = [rng.standard_normal(3).astype(np.float32) for _ in crops]
    poses = [np.eye(4) + rng.standard_normal((4, 4)) for _ in crops]

    def check(ds, i, c, lat, pose):
        s = ds[i]
        assert s["rgb"].tobytes() == c.rgb.tobytes() and s["uvw"].tobytes() == c.uvw.tobytes() and s["rgb"].shape == c.rgb.shape
        assert s["latent"].numpy().tobytes() == lat.tobytes()
        want_k = K.copy()
        want_k[0, 2] -= c.box[0]
        want_k[1, 2] -= c.box[1]
        assert np.array_equal(crop_intrinsics(K, c.box), want_k)
        assert s["intrinsics"].numpy().tobytes() == want_k.astype(np.float32).tobytes()
        assert s["pose"].numpy().tobytes() == pose.astype(np.float32).tobytes()
        assert s["crop_size"].tolist() == [c.rgb.shape[1], c.rgb.shape[0]]

    with CropWriter(path) as w:
        assert w.add(crops[0], lats[0], K, poses[0], name="Car") == 0
        assert w.add(crops[1], torch.from_numpy(lats[1]), (720.0, 710.0, 600.5, 180.25), torch.from_numpy(poses[1])) == 1
    ds = Crops(str(path))
    assert len(ds) == 2
    check(ds, 0, crops[0], lats[0], poses[0])
    check(ds, 1, crops[1], lats[1], poses[1])
    gt = json.load(open(path / "crops.json"))
    assert sorted(gt) == ["0", "1"] and gt["0"][0]["name"] == "Car" and sorted(gt["1"][0]) == ["extrinsics", "intrinsics", "latent"]
    assert sorted(os.listdir(path)) == ["00000_rgb.png", "00000_uvw.png", "00001_rgb.png", "00001_uvw.png", "crops.json"]
    # appending continues the index
    with CropWriter(path) as w:
        assert len(w) == 2 and w.add(crops[2], lats[2], K, poses[2]) == 2
    ds = Crops(str(path))
    assert len(ds) == 3
    for i in range(3):
        check(ds, i, crops[i], lats[i], poses[i])
    # a crash before close() leaves the old crops.json intact
    before = open(path / "crops.json", "rb").read()
    with pytest.raises(RuntimeError):
        with CropWriter(path) as w:
            w.add(crops[0], lats[0], K, poses[0])
            raise RuntimeError("the run dies here")
    assert open(path / "crops.json", "rb").read() == before and len(Crops(str(path))) == 3
    w = CropWriter(path)
    w.add(crops[0], lats[0], K, poses[0])
    del w                                                                                 # never closed
    assert open(path / "crops.json", "rb").read() == before
    assert not [n for n in os.listdir(path) if n.endswith(".tmp")]
    # refusals
    w = CropWriter(path)
    with pytest.raises(ValueError):
        w.add(_host_crop(rng, 0, 5, (0, 0, 5, 0)), lats[0], K, poses[0])
    with pytest.raises(TypeError):
        w.add(crops[0], lats[0], K, poses[0], bad=object())
    assert w.next == 3 and len(w) == 3
    w.close()
    with pytest.raises(ValueError):
        w.add(crops[0], lats[0], K, poses[0])


# ---- header, ctypes table, library, Python side ------------------------------------------------------------------------------------------------

def test_abi_has_the_export_entry_points():
    from sdflabel_amd import _lib
    header = open(os.path.join(ROOT, "include", "sdfr.h")).read()
    h = _lib.lib()
    for name in ("sdfr_crop_owner", "sdfr_crop_export", "sdfr_crop_counts"):
        assert name in _lib.EXPORTS and hasattr(h, name) and re.search(r"\bint %s\(" % name, header), name
    assert int(re.search(r"#define SDFR_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION == h.sdfr_version() >= 413
    build = open(os.path.join(ROOT, "sdflabel_amd", "csrc", "build.sh")).read()
    assert re.search(r"-ffp-contract=off -c \"\$HERE/crops\.hip\"", build)


def test_argument_checks_come_before_any_launch():
    import ctypes
    from sdflabel_amd import _lib
    h = _lib.lib()
    k = (ctypes.c_double * 4)(8, 8, 32, 24)
    N = None
    assert h.sdfr_crop_owner(N, N, N, N, 10, 1, 64, 48, N, N) == -1 and b"NULL" in h.sdfr_last_error()
    assert h.sdfr_crop_owner(N, N, N, N, 0, 0, 64, 48, N, N) == 0
    assert h.sdfr_crop_owner(N, N, N, N, 64 * 48 + 1, 1, 64, 48, N, N) == -1 and b"out of range" in h.sdfr_last_error()
    assert h.sdfr_crop_owner(N, N, N, N, 0, 1, 0, 48, N, N) == -1

    def export(V=0, T=0, P=0, Q=0, B=1, K=k, z=0.1):
        return h.sdfr_crop_export(N, V, N, T, N, N, N, N, N, P, N, N, N, N, Q, N, B, 64, 48, K, z, N, N, N, N)
    assert export() == -1 and b"NULL" in h.sdfr_last_error()
    assert export(B=0) == 0
    assert export(K=None) == -1 and b"intrinsics" in h.sdfr_last_error()
    assert export(z=-1.0) == -1
    assert export(P=10, Q=11) == -1 and b"out of range" in h.sdfr_last_error()            # boxes lie inside windows: Q <= P
    assert export(P=64 * 48 + 1) == -1
    assert h.sdfr_crop_counts(N, N, N, N, 0, N, N, 0, N, 2, 64, 48, N, N) == -1 and b"NULL" in h.sdfr_last_error()
    assert h.sdfr_crop_counts(N, N, N, N, 0, N, N, 0, N, 0, 64, 48, N, N) == 0
    assert h.sdfr_crop_counts(N, N, N, N, 5, N, N, 6, N, 1, 64, 48, N, N) == -1


def test_python_side_without_a_gpu():
    import torch
    from sdflabel_amd import _lib
    from sdflabel_amd import export as E
    from sdflabel_amd.mesh import Mesh
    from sdflabel_amd.pipelines.export_crops import export_frame
    from sdflabel_amd.pipelines.frame import refine_frame
    v = torch.tensor([[0.0, 0, 0], [0.5, 0, 0], [0, 0.5, 0]])
    m = Mesh(v, torch.zeros((1, 3), dtype=torch.int32), scale=2.0, cam_T=np.diag([1.0, -1.0, 1.0, 1.0]))
    assert m.lattice_vertices is None
    c = m.to_camera()
    assert c.frame == "camera" and c.lattice_vertices is m.vertices and c.to_camera() is c       # the lattice vertices ride along, same order
    assert torch.equal(c.vertices, torch.tensor([[0.0, 0, 0], [1.0, 0, 0], [0, -1.0, 0]]))
    box = [[10, 5, 30, 21]]
    with pytest.raises(ValueError):
        E.crops_many([m], VC.K8, box, (VC.W, VC.H))                                        # a lattice-frame mesh
    with pytest.raises(ValueError):
        E.crops_many([c], VC.K8, box + box, (VC.W, VC.H))
    with pytest.raises(ValueError):
        E.crops_many([c], VC.K8, box, (VC.W, VC.H), margin=-0.1)
    with pytest.raises(ValueError):
        E.crops_many([Mesh(v, m.faces, frame="camera")], VC.K8, box, (VC.W, VC.H))         # no attributes
    with pytest.raises(ValueError):
        E.crops_many([c], VC.K8, box, (VC.W, VC.H), colors=[np.zeros((3, 3, 3), np.float32)])
    with pytest.raises(_lib.SdfrError):
        E.crops_many([c], VC.K8, box, (VC.W, VC.H))                                        # no CPU fallback
    assert E.crops_many([], VC.K8, [], (VC.W, VC.H)) == []
    with pytest.raises(ValueError):
        refine_frame([], None, None, [], None, None, 1, {}, crops=True)                    # needs return_stages
    with pytest.raises(ValueError):
        export_frame({}, None)
    with pytest.raises(ValueError):
        export_frame({"crops": []}, None)                                                  # only_ok without verdicts
    assert export_frame({"crops": []}, None, only_ok=False) == []
