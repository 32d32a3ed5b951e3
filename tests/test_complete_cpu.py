"""Shape completion from one view without a GPU: the numpy restatement (tests/_complete_ref.py) against torch float64 autograd +
torch.optim.Adam on mixed exact / one-sided / satisfied / invalid rows, csrc/complete_cells.h compiled into a host program
(tests/complete_host/complete_host.cpp) against the restatement bit for bit -- also under ASan/UBSan with exact-size buffers and broken
tables --, cpl_row = enc_row at lo == hi in every bit, analytic checks of the view rows on a sphere, exports / header / binding, argument
checks, the .npz round trip and the calibration of the trajectory bound of tests/test_gpu_complete.py on the float32 emulation.
"""
import copy
import os
import re
import struct
import subprocess

import numpy as np
import pytest
import torch

from sdflabel_amd import _lib
from sdflabel_amd import complete as C
from sdflabel_amd.sdf_samples import SdfSamples
from tests import _complete_cases as CC
from tests import _complete_ref as CR
from tests import _complete_traj as CT
from tests import _encode_ref as ER
from tests import _encode_traj as ET
from tests import _prior_train_cases as PC
from tests._prior_train_loop import plain_forward
from tests._util import build_host_program

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement's loop against torch ------------------------------------------------------------------------------------------------

def _torch_fit(dec, samples, soff, z0, iters, k, lr, lr_step, lr_factor, clamp, code_reg, unit):
    """float64 autograd + torch.optim.Adam on the first k rows of every shape.  A row's loss is the distance from the clamped prediction to
    the clamped interval, relu(cl - cp) + relu(cp - ch); a shape's loss is the sum over its usable rows divided by their number (the
    satisfied ones count); the total is the SUM over shapes, so a shape's gradient is its own."""
    dec = copy.deepcopy(dec).double()
    for p in dec.parameters():
        p.requires_grad_(False)
    z = torch.tensor(np.asarray(z0, np.float64), requires_grad=True)
    opt = torch.optim.Adam([z], lr=lr)
    B = z.shape[0]
    rows = torch.tensor(np.stack([np.asarray(samples, np.float64)[int(soff[b]):int(soff[b]) + k] for b in range(B)]))      # [B][k][5]
    ok = (rows[:, :, 3] <= rows[:, :, 4]) & (torch.isfinite(rows[:, :, 3]) | torch.isfinite(rows[:, :, 4]))
    lo, hi = torch.nan_to_num(rows[:, :, 3], nan=0.0).clamp(-clamp, clamp), torch.nan_to_num(rows[:, :, 4], nan=0.0).clamp(-clamp, clamp)
    losses = []
    for it in range(iters):
        opt.param_groups[0]["lr"] = lr * lr_factor ** (it // lr_step)
        zn = z / z.norm(dim=1, keepdim=True) if unit else z
        inputs = torch.cat([zn.repeat_interleave(k, 0), rows[:, :, :3].reshape(-1, 3)], 1)
        cp = plain_forward(dec, inputs)[:, 0].reshape(B, k).clamp(-clamp, clamp)
        dist = torch.relu(lo - cp) + torch.relu(cp - hi)
        per = torch.where(ok, dist, torch.zeros_like(dist)).sum(1) / ok.sum(1)
        loss = per.sum() if unit else (per + code_reg * z.norm(dim=1)).sum()
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        losses.append(per.detach().numpy().copy())
    return z.detach().numpy(), np.array(losses)


@pytest.mark.parametrize("name", ["w128", "lat8"])
@pytest.mark.parametrize("unit", [True, False])
def test_restatement_loop_equals_torch_float64_autograd_and_adam(name, unit):
    dec, net = PC.decoders()[name], PC.net(name)
    samples, soff, z0, k = CC.fit_case(name, seed=3, B=3, k=66)
    kinds = np.arange(k) % 6
    ok = np.isfinite(samples[:k, 3])
    assert (samples[:k, 3] == samples[:k, 4])[kinds < 2].all() and (samples[:k, 3] < samples[:k, 4])[(kinds >= 2) & (kinds < 5)].all() and not ok[kinds == 5].any()
    kw = dict(lr=5e-3, lr_step=5, lr_factor=0.1, clamp=ET.CLAMPS[name], code_reg=1e-4)
    ref = CR.loop(ET.decoder64(net), samples, soff, z0, 10, k, False, unit=unit, ft=np.float64, **kw)
    z_t, losses = _torch_fit(dec, samples, soff, z0, 10, k, unit=unit, **kw)
    assert np.abs(ref["z"] - z_t).max() <= 1e-12, float(np.abs(ref["z"] - z_t).max())
    assert np.abs(ref["history"] - losses).max() <= 1e-12
    assert np.abs(ref["z"] - z0).max() > 1e-3                                   # ten steps moved the latents
    keep = np.isfinite(samples[:, 3])                                           # (the exact fit has no way to leave a row out)
    exact = ER.loop(ET.decoder64(net), np.where(keep[:, None], samples[:, :4], 0), soff, z0, 10, k, False, unit=unit, ft=np.float64, **kw)
    assert np.abs(exact["z"] - ref["z"]).max() > 1e-4                           # and the intervals matter: ten steps of the exact fit on the
    #                                                                             lower bounds end elsewhere


# ---- the header on the host -----------------------------------------------------------------------------------------------------------------

def _f32_bits(x):
    return struct.unpack("<I", struct.pack("<f", float(x)))[0]


def _f64_bits(x):
    return struct.unpack("<q", struct.pack("<d", float(x)))[0]


def _run(exe, mode, tmp, head, arrays, expect=0):
    src, dst = os.path.join(str(tmp), "in.bin"), os.path.join(str(tmp), "out.bin")
    with open(src, "wb") as f:
        f.write(np.asarray(list(head) + [0] * (10 - len(head)), np.int64).tobytes())
        for a in arrays:
            f.write(np.ascontiguousarray(a).tobytes())
    r = subprocess.run([exe, mode, src, dst], capture_output=True, text=True)
    assert r.returncode == expect, (r.returncode, r.stderr[-3000:])
    return open(dst, "rb").read()


def _split(blob, specs):
    out, at = [], 0
    for dtype, shape in specs:
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        out.append(np.frombuffer(blob, dtype=dtype, count=int(np.prod(shape)), offset=at).reshape(shape))
        at += n
    assert at == len(blob)
    return out


def same_bits(a, b, what=""):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    assert np.array_equal(a.view(u), b.view(u)), (what, int((a.view(u) != b.view(u)).sum()))


def host_row(exe, tmp, p, lo, hi, clamp):
    n = len(p)
    blob = _run(exe, "row", tmp, [n, _f32_bits(clamp)], [np.asarray(a, np.float32) for a in (p, lo, hi)])
    out = _split(blob, [(np.float64, (n,)), (np.float32, (n,)), (np.int32, (n,))] * 3)
    return out[:3], out[3:6], out[6:]


def host_view(exe, tmp, pts, nrm, ptoff, pose, origin, F, eta, s_max, seed, shape0=0, N=None):
    N = len(pts) if N is None else N
    B = len(pose)
    arrays = [np.asarray(ptoff, np.int64), pose, origin, np.asarray(pts, np.float32)[:N]] + ([np.asarray(nrm, np.float64)[:N]] if nrm is not None else [])
    blob = _run(exe, "view", tmp, [N, B, F, shape0, seed, _f64_bits(eta), _f64_bits(s_max), int(nrm is not None)], arrays)
    return _split(blob, [(np.float32, (N * (3 + F), 5)), (np.int32, (B,))])


def host_rows(exe, tmp, samples, soff, B, k, draw, seed, it, z, unit, S=None, shape0=0):
    L = z.shape[1]
    S = len(samples) if S is None else S
    blob = _run(exe, "rows", tmp, [S, B, k, draw, seed, it, L, unit, shape0], [np.asarray(soff, np.int64), np.asarray(samples, np.float32)[:S], z])
    return _split(blob, [(np.float32, (B * k, L + 3)), (np.float32, (B * k,)), (np.float32, (B * k,)), (np.float32, (B, L)), (np.int32, (B,))])


def host_reduce(exe, tmp, pred, lo, hi, J, L, B, k, clamp, flags):
    blob = _run(exe, "reduce", tmp, [B, k, L, J.shape[1], _f32_bits(clamp)], [pred, lo, hi, J, flags])
    ch = (k + ER.CHUNK - 1) // ER.CHUNK
    loss, g, part, fl = _split(blob, [(np.float64, (B,)), (np.float64, (B, L)), (np.float64, (B, ch, L + 2)), (np.int32, (B,))])
    return loss, g, fl, part


def row_grid():
    """every (p, t) of a grid with +-0, +-clamp and its neighbours, values beyond the clamp, +-inf and NaN, for three clamps"""
    out = []
    for clamp in (0.1, 1.0, np.float32(0.3)):
        c = np.float32(clamp)
        v = np.array([0.0, -0.0, c, -c, np.nextafter(c, np.float32(1)), np.nextafter(c, np.float32(0)), np.nextafter(-c, np.float32(-1)),
                      np.nextafter(-c, np.float32(0)), 0.03, -0.07, 2 * c, -3 * c, 1e-45, -1e-45, 3e38, -3e38, np.inf, -np.inf, np.nan], np.float32)
        p, t = np.meshgrid(v, v, indexing="ij")
        out.append((clamp, p.reshape(-1).copy(), t.reshape(-1).copy()))
    return out


def _host_checks(exe, tmp):
    # the row rule: cpl_row(p, t, t) = enc_row(p, t) in every bit, on the host program and in the restatement; intervals = the restatement
    for clamp, p, t in row_grid():
        hi = np.where(np.arange(len(t)) % 2 == 0, t + np.float32(0.05), np.float32(np.inf)).astype(np.float32)
        got, at_t, enc = host_row(exe, tmp, p, t, hi, clamp)
        for a, b, n in zip(at_t, enc, ("e", "w", "ok")):
            same_bits(a, b, ("cpl_row(p, t, t) against enc_row(p, t)", clamp, n))
        e, w, ok = ER.row_rule(p, t, clamp)
        for a, b, n in zip(enc, (e, w, ok.astype(np.int32)), ("e", "w", "ok")):
            same_bits(a, b, ("enc_row against its restatement", clamp, n))
        e, w, ok = CR.row_rule(p, t, t, clamp)
        for a, b, n in zip(at_t, (e, w, ok.astype(np.int32)), ("e", "w", "ok")):
            same_bits(a, b, ("restatement at lo == hi", clamp, n))
        e, w, ok = CR.row_rule(p, t, hi, clamp)
        for a, b, n in zip(got, (e, w, ok.astype(np.int32)), ("e", "w", "ok")):
            same_bits(a, b, ("intervals", clamp, n))
        assert ok.any() and not ok.all() and (e[ok] == 0).any() and (e[ok] > 0).any()
    # the views
    for case in CC.view_cases():
        B, counts, F, normals, special = case
        pts, ptoff, pose, origin, nrm = CC.view_case(*case)
        for shape0 in (0, 9):
            got = host_view(exe, tmp, pts, nrm, ptoff, pose, origin, F, CC.ETA, CC.S_MAX, CC.SEED, shape0)
            want = CR.view_rows(pts, nrm, ptoff, pose, origin, F, CC.ETA, CC.S_MAX, CC.SEED, shape0)
            same_bits(got[0], want[0], (case, "rows")); same_bits(got[1], want[1], (case, "flags"))
        _view_case_properties(case, want)
    # broken tables: flagged, invalid rows, nothing read through them (the sanitizer build watches the reads)
    case = (3, (65, 65, 65), 4, "all", None)
    pts, ptoff, pose, origin, nrm = CC.view_case(*case)
    for broken in CC.BROKEN_PTOFF:
        for N in (195, 100):
            got = host_view(exe, tmp, pts, nrm, broken, pose, origin, 4, CC.ETA, CC.S_MAX, CC.SEED, N=N)
            want = CR.view_rows(pts[:N], nrm[:N], broken, pose, origin, 4, CC.ETA, CC.S_MAX, CC.SEED, N=N)
            same_bits(got[0], want[0], (broken, N)); same_bits(got[1], want[1], (broken, N))
            bad = [a < 0 or e < a or e > N for a, e in zip(broken[:-1], broken[1:])]
            assert [bool(f & CR.BAD_TABLE) for f in want[1]] == bad, (broken, N)
            nobody = np.array([CR.owner(broken, 3, N, g) < 0 for g in range(N)])
            assert not np.isfinite(want[0].reshape(N, 7, 5)[nobody, :, 3]).any()
    # the interval rows and the reduce
    for case in CC.rows_cases():
        B, counts, k, draw, L, unit = case
        samples, soff, z = CC.rows_case(*case)
        got = host_rows(exe, tmp, samples, soff, B, k, draw, CC.SEED, 17, z, unit, shape0=2)
        want = CR.rows(samples, soff, B, k, draw, CC.SEED, 17, z, unit, shape0=2)
        for g, w, n in zip(got, want, ("inputs", "lo", "hi", "zn", "flags")):
            same_bits(g, w, (case, n))
    samples, soff, z = CC.rows_case(3, (65, 0, 72), 65, 0, 3, 1)
    for broken, S in (([0, -4, 75, 115], None), ([0, 80, 75, 115], None), ([0, 65, 65, 999], None), ([0, 65, 65, 137], 100)):
        got = host_rows(exe, tmp, samples, broken, 3, 64, 1, CC.SEED, 0, z, 1, S=S)
        want = CR.rows(samples[:S], broken, 3, 64, 1, CC.SEED, 0, z, 1, S=S)
        for g, w in zip(got, want):
            same_bits(g, w, broken)
        assert (want[4] & ER.BAD_TABLE).any()
    for case in CC.reduce_cases():
        B, k, L, Js = case
        pred, lo, hi, J, flags = CC.reduce_case(*case)
        got = host_reduce(exe, tmp, pred, lo, hi, J, L, B, k, CC.CLAMP, flags)
        want = CR.reduce(pred, lo, hi, J, L, B, k, CC.CLAMP, flags)
        for g, w, n in zip(got, want, ("loss", "g_zn", "flags", "part")):
            same_bits(g, w, (case, n))
        assert np.isfinite(want[0]).all() and np.isfinite(want[1][0]).all()
        if B >= 2:
            assert want[2][1] & ER.NO_ROWS and want[0][1] == 0 and not want[1][1].any()
        # at lo == hi the reduce is the encoder's
        got = host_reduce(exe, tmp, pred, lo, lo, J, L, B, k, CC.CLAMP, flags)
        want = ER.reduce(pred, lo, J, L, B, k, CC.CLAMP, flags)
        for g, w, n in zip(got, want, ("loss", "g_zn", "flags", "part")):
            same_bits(g, w, (case, "lo == hi", n))


def _view_case_properties(case, want):
    """what each case was built to show, on the restatement's rows"""
    B, counts, F, normals, special = case
    rows, flags = want
    P = 3 + F
    N = sum(counts)
    valid = np.isfinite(rows[:, 3]).reshape(N, P) if N else np.zeros((0, P), bool)
    assert (np.abs(rows[:, :3]) <= 1).all() and (rows[~valid.reshape(-1), :3] == 0).all()
    if N >= 65:
        assert valid[:, 0].any() and not valid[:, 0].all()                          # points inside the cube, and points that leave it
    if normals == "none":
        assert not valid[:, 1:3].any()
    elif N >= 65 and special is None:
        assert valid[:, 1].any() and (valid[:, 0] & ~valid[:, 1]).any() == (normals == "holes" or bool((valid[:, 0] & ~valid[:, 1]).any()))
    if special == "scale0":
        assert flags.tolist() == [0, CR.BAD_POSE, CR.BAD_POSE] and not valid[65:].any() and valid[:65, 0].any()
    else:
        assert not flags.any()
    if special == "on_sensor":
        on = np.nonzero(valid[:, 0] & ~valid[:, 3:].any(1))[0]
        assert len(on) >= 1 and valid[on[0], 1]                                      # the point on the sensor: no ray, its other rows stand
    if F and N >= 65 and special != "scale0":
        free = rows.reshape(N, P, 5)[:, 3:]
        v = valid[:, 3:]
        assert v.any() and (free[v][:, 3] == 0).all() and (free[v][:, 4] >= 0).all() and (free[v][:, 4] <= np.float32(CC.S_MAX)).all()
        if F > 1:
            s = np.where(v, free[:, :, 4], np.nan)
            with np.errstate(invalid="ignore"):
                assert not (np.diff(s, axis=1) < 0).any()                            # stratified: slot f lies behind slot f - 1 on the ray


def test_complete_cells_on_the_host_equal_the_restatement_bit_for_bit(tmp_path):
    _host_checks(build_host_program(tmp_path, "complete_host/complete_host.cpp", "complete_host"), tmp_path)


def test_complete_cells_host_program_under_sanitizers(tmp_path):
    _host_checks(build_host_program(tmp_path, "complete_host/complete_host.cpp", "complete_host_san",
                                    ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]), tmp_path)


def test_verify_point_x_keeps_its_bits_after_the_float64_part_was_factored_out():
    """slot 0 of a view row is verify_point_x's position: the same float64 operations, rounded once (tests/_verify_ref.py restates it)"""
    from tests import _verify_ref as VR
    pts, ptoff, pose, origin, nrm = CC.view_case(1, (257,), 4, "all", None)
    rows, _ = CR.view_rows(pts, nrm, ptoff, pose, origin, 0, CC.ETA, CC.S_MAX, CC.SEED)
    x, in_cube = VR.point_x(pts, pose[0])
    rows = rows[0::3]                                                            # slot 0 of every point (F = 0: three slots a point)
    assert in_cube.any() and not in_cube.all()
    same_bits(rows[in_cube.astype(bool), :3], x[in_cube.astype(bool)])
    assert not np.isfinite(rows[~in_cube.astype(bool), 3]).any()


# ---- a sphere seen from outside -----------------------------------------------------------------------------------------------------------------

R_SPHERE = 0.6


@pytest.fixture(scope="module")
def sphere_view():
    """2000 points of the sphere |x| = R_SPHERE in the lattice frame that face a sensor outside it, in the camera frame of one pose; the
    outward normals, in the camera frame too"""
    rng = np.random.default_rng(11)
    yaw = np.float32(0.7)
    pose = np.array([[np.cos(yaw), np.sin(yaw), 0.4, -0.1, 3.0, 1.7]], np.float32)
    c, s, t, sc = float(pose[0, 0]), float(pose[0, 1]), pose[0, 2:5].astype(np.float64), float(pose[0, 5])
    sensor_x = CR.lattice_x(np.zeros(3, np.float32), pose[0])                    # the camera centre in the lattice frame: about 3 units away
    v = rng.standard_normal((8000, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    v = v[(v * (sensor_x - R_SPHERE * v)).sum(1) > 0.05][:2000]                   # facing the sensor, away from the silhouette
    def to_cam(x, with_t):
        xs = x * np.array([1.0, -1.0, 1.0])
        r = np.stack([c * xs[:, 0] + s * xs[:, 2], xs[:, 1], -s * xs[:, 0] + c * xs[:, 2]], 1)
        return sc * (r + t) if with_t else r
    pts = to_cam(R_SPHERE * v, True).astype(np.float32)
    F = 8
    rows, flags = CR.view_rows(pts, to_cam(v, False), np.array([0, len(pts)]), pose, np.zeros(3, np.float32), F, CC.ETA, CC.S_MAX, CC.SEED)
    # float32 rounding: a camera coordinate is off by at most 2^-24 |p|, so the hit point by sqrt(3) 2^-24 max|p| / scale in the lattice frame;
    # a stored position by sqrt(3) 2^-24 (coordinates <= 1); a stored bound by 2^-24 s_max
    tol = np.sqrt(3) * 2.0 ** -24 * (np.abs(pts).max() / sc + 1.0) + 2.0 ** -24 * CC.S_MAX
    return rows.reshape(len(pts), 3 + F, 5), flags, tol


def test_free_space_rows_of_a_sphere_hold_its_true_distance(sphere_view):
    rows, flags, tol = sphere_view
    assert not flags.any() and np.isfinite(rows[:, :, 3]).all()                                 # every slot valid
    free = rows[:, 3:].reshape(-1, 5).astype(np.float64)
    dist = np.linalg.norm(free[:, :3], axis=1) - R_SPHERE
    assert (free[:, 3] == 0).all() and (dist >= free[:, 3] - tol).all() and (dist <= free[:, 4] + tol).all()
    assert (dist < free[:, 4] - 10 * tol).mean() > 0.5 and free[:, 4].max() > 0.9 * CC.S_MAX      # and the upper bound is a bound, not the value
    assert tol < 1e-6                                                              # (a few float32 ulps of a coordinate near 6)


def test_normal_rows_of_a_sphere_lie_eta_off_it(sphere_view):
    rows, _, tol = sphere_view
    fe = np.float32(CC.ETA)
    out, inn = rows[:, 1].astype(np.float64), rows[:, 2].astype(np.float64)
    assert (rows[:, 1, 3] == fe).all() and (rows[:, 1, 4] == fe).all() and (rows[:, 2, 3] == -fe).all() and (rows[:, 2, 4] == -fe).all()
    assert np.abs(np.linalg.norm(out[:, :3], axis=1) - (R_SPHERE + CC.ETA)).max() <= tol
    assert np.abs(np.linalg.norm(inn[:, :3], axis=1) - (R_SPHERE - CC.ETA)).max() <= tol
    assert np.abs(np.linalg.norm(rows[:, 0, :3].astype(np.float64), axis=1) - R_SPHERE).max() <= tol


def test_stratified_draws_are_uniform_within_five_sigma():
    n, bins = 1 << 16, 64
    for shape, f in ((0, 0), (65534, 63)):
        u = _u_points(shape, f, n)
        assert u.min() >= 0 and u.max() < 1
        h = np.bincount((u * bins).astype(np.int64), minlength=bins)
        sigma = np.sqrt(n * (1.0 / bins) * (1 - 1.0 / bins))
        assert np.abs(h - n / bins).max() <= 5 * sigma, h
    a = _u_points(3, 1, 1000)
    assert np.array_equal(a, _u_points(3, 1, 1000))
    for other in (_u_points(4, 1, 1000), _u_points(3, 2, 1000), _u_points(3, 1, 1000, seed=CC.SEED + 1)):
        assert (a != other).mean() > 0.99


def _u_points(shape, f, n, seed=CC.SEED):
    """u of slot f of points 0 .. n - 1 of one shape (u_of is vectorised over slots; its key is linear in the point, so shift by hand)"""
    i = np.arange(n, dtype=np.uint64)
    key = (np.uint64(shape) << np.uint64(40)) | (i << np.uint64(8)) | np.uint64(f)
    with np.errstate(over="ignore"):
        h = ER.mix64(np.uint64(seed & 0xFFFFFFFFFFFFFFFF) ^ ER.mix64(key * ER.GOLDEN + np.uint64(1)))
    u = (h >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    assert u[7] == CR.u_of(seed, shape, 7, np.array([f]))[0]
    return u


# ---- exports, header, binding -------------------------------------------------------------------------------------------------------------

NAMES = ("sdfr_view_samples", "sdfr_bound_rows", "sdfr_bound_reduce")


def test_exports_header_and_binding_agree():
    header = open(os.path.join(ROOT, "include", "sdfr.h")).read()
    assert _lib.ABI_VERSION >= 419 and int(re.search(r"#define SDFR_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION
    assert "419: shape completion" in header
    body = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    h = _lib.lib()
    assert h.sdfr_version() == _lib.ABI_VERSION
    for name in NAMES:
        assert name in _lib.EXPORTS and hasattr(h, name) and re.search(r"\bint %s\(" % name, body), name
    cells = open(os.path.join(ROOT, "sdflabel_amd", "csrc", "complete_cells.h")).read()
    for name, val in (("CPL_MAX_FREE", CR.MAX_FREE), ("CPL_BAD_POSE", CR.BAD_POSE), ("CPL_BAD_TABLE", CR.BAD_TABLE), ("CPL_ROW", 5)):
        assert int(re.search(r"#define %s (\d+)" % name, cells).group(1)) == val, name
    assert (C.BAD_POSE, C.BAD_TABLE, C.MAX_FREE) == (CR.BAD_POSE, CR.BAD_TABLE, CR.MAX_FREE)
    assert "train_mix64" in cells and "0xBF58476D1CE4E5B9" not in cells and "verify_point_x64" in cells
    # one copy of the summation order: the reduce kernels live in one header, instantiated by both translation units
    enc, cpl = (open(os.path.join(ROOT, "sdflabel_amd", "csrc", n)).read() for n in ("encode.hip", "complete.hip"))
    assert "enc_tree_step" not in enc and "enc_tree_step" not in cpl and "encode_kernels.h" in enc and "encode_kernels.h" in cpl
    assert "complete.hip" in open(os.path.join(ROOT, "sdflabel_amd", "csrc", "build.sh")).read()


def test_c_argument_checks_need_no_gpu():
    h = _lib.lib()
    d, inv = 4096, -1            # never dereferenced: every call below is refused before a launch
    assert h.sdfr_view_samples(d, d, 10, d, 1, d, d, 0, 65, 0.01, 0.5, 0, d, d, None) == inv and b"free-space" in h.sdfr_last_error()
    assert h.sdfr_view_samples(d, d, 10, d, 1, d, d, 0, -1, 0.01, 0.5, 0, d, d, None) == inv
    assert h.sdfr_view_samples(d, d, 10, None, 1, d, d, 0, 4, 0.01, 0.5, 0, d, d, None) == inv and b"NULL" in h.sdfr_last_error()
    assert h.sdfr_view_samples(None, d, 10, d, 1, d, d, 0, 4, 0.01, 0.5, 0, d, d, None) == inv
    assert h.sdfr_view_samples(d, d, 10, d, 0, d, d, 0, 4, 0.01, 0.5, 0, d, d, None) == inv and b"without a shape" in h.sdfr_last_error()
    assert h.sdfr_view_samples(d, d, 10, d, 1, d, d, 0, 4, float("nan"), 0.5, 0, d, d, None) == inv and b"eta" in h.sdfr_last_error()
    assert h.sdfr_view_samples(d, d, 10, d, 1, d, d, 0, 4, 0.01, -1.0, 0, d, d, None) == inv
    assert h.sdfr_view_samples(d, d, 10, d, 2, d, d, 65534, 4, 0.01, 0.5, 0, d, d, None) == inv and b"shape0" in h.sdfr_last_error()
    assert h.sdfr_view_samples(d, d, (1 << 32) + 1, d, 1, d, d, 0, 4, 0.01, 0.5, 0, d, d, None) == inv and b"2^32" in h.sdfr_last_error()
    assert h.sdfr_view_samples(d, d, 0, d, 0, d, d, 0, 4, 0.01, 0.5, 0, d, d, None) == 0
    assert h.sdfr_bound_rows(d, 10, None, 1, 0, 5, 0, 0, 0, d, 3, 1, d, d, d, d, d, None) == inv and b"sdfr_bound_rows: NULL" in h.sdfr_last_error()
    assert h.sdfr_bound_rows(d, 10, d, 1, 0, 5, 0, 0, 0, d, 3, 1, d, d, None, d, d, None) == inv and b"NULL" in h.sdfr_last_error()
    assert h.sdfr_bound_rows(d, 10, d, 1, 0, 0, 0, 0, 0, d, 3, 1, d, d, d, d, d, None) == inv and b"k = 0" in h.sdfr_last_error()
    assert h.sdfr_bound_rows(d, 10, d, 1, 0, 5, 0, 0, 0, d, 257, 1, d, d, d, d, d, None) == inv and b"latent size" in h.sdfr_last_error()
    assert h.sdfr_bound_rows(d, 10, d, 0, 0, 5, 0, 0, 0, d, 3, 1, d, d, d, d, d, None) == 0
    assert h.sdfr_bound_reduce(d, d, d, d, 2, 3, 1, 5, 0.1, d, 1 << 20, d, d, d, None) == inv and b"stride" in h.sdfr_last_error()
    assert h.sdfr_bound_reduce(d, d, d, d, 6, 3, 1, 5, 0.1, d, 39, d, d, d, None) == inv and b"workspace" in h.sdfr_last_error()
    assert h.sdfr_bound_reduce(d, d, d, d, 6, 3, 1, 5, 0.0, d, 40, d, d, d, None) == inv and b"clamp" in h.sdfr_last_error()
    assert h.sdfr_bound_reduce(d, d, None, d, 6, 3, 1, 5, 0.1, d, 40, d, d, d, None) == inv and b"sdfr_bound_reduce: NULL" in h.sdfr_last_error()
    assert h.sdfr_bound_reduce(d, d, d, d, 6, 3, 0, 5, 0.1, d, 0, d, d, d, None) == 0


def test_python_argument_checks_come_before_any_launch():
    dec = PC.decoders()["w128"]                                                    # on the CPU
    s = C.BoundSamples(torch.zeros((10, 5)))
    with pytest.raises(ValueError):
        C.fit_many(dec, [s], iters=-1)
    with pytest.raises(ValueError):
        C.fit_many(dec, [s], clamp=0.0)
    with pytest.raises(ValueError):
        C.fit_many(dec, [C.BoundSamples(torch.zeros((10, 4)))])                     # exact rows go through from_sdf
    with pytest.raises(ValueError):
        C.fit_many(dec, [s], init=torch.zeros((1, 8)))
    with pytest.raises(_lib.SdfrError):
        C.fit_many(dec, s)                                                         # a CPU decoder, CPU rows
    p = {"yaw": torch.zeros(1), "trans": torch.zeros(3), "scale": torch.ones(1), "latent": torch.zeros(3)}
    cloud = np.zeros((4, 3), np.float32)
    with pytest.raises(ValueError):
        C.view_samples_many([p], [cloud, cloud])
    with pytest.raises(ValueError):
        C.view_samples_many([p], [cloud], free_rows=65)
    with pytest.raises(ValueError):
        C.view_samples_many([p], [cloud], s_max=-1.0)
    with pytest.raises(ValueError):
        C.view_samples_many([p], [cloud], eta=float("nan"))
    with pytest.raises(ValueError):
        C.view_samples_many([p], [cloud], normals=[])
    with pytest.raises(_lib.SdfrError):
        C.view_samples_many([p], [cloud], _device="cpu")
    with pytest.raises(_lib.SdfrError):
        C.complete_many(dec, [p], [cloud])
    assert C.view_samples_many([], []) == []
    assert "as recalled" in C.view_samples_many.__doc__.lower() and "as recalled" in C.__doc__.lower()


def test_bound_samples_round_trip_from_sdf_and_concat(tmp_path):
    rng = np.random.default_rng(3)
    rows = rng.uniform(-1, 1, (12, 5)).astype(np.float32)
    rows[3, 3:] = np.nan
    rows[4, 4] = np.inf
    s = C.BoundSamples(torch.from_numpy(rows))
    s.save(str(tmp_path / "view.npz"))
    z = np.load(str(tmp_path / "view.npz"))
    assert list(z.keys()) == ["rows"] and z["rows"].dtype == np.float32 and z["rows"].shape == (12, 5)
    back = C.BoundSamples.load(str(tmp_path / "view.npz"))
    same_bits(back.numpy(), rows)
    assert len(back) == 12 and back.flags is None
    exact = SdfSamples(torch.from_numpy(rows[:, :4].copy()))
    b = C.BoundSamples.from_sdf(exact)
    same_bits(b.numpy()[:, :4], rows[:, :4]); same_bits(b.numpy()[:, 4], rows[:, 3])
    both = C.BoundSamples.concat(s, exact)
    assert len(both) == 24
    same_bits(both.numpy()[:12], rows); same_bits(both.numpy()[12:], b.numpy())
    same_bits(C.BoundSamples.concat([s, b]).numpy(), both.numpy())
    with pytest.raises(ValueError):
        C.BoundSamples.from_sdf(s)
    with pytest.raises(ValueError):
        C.BoundSamples.concat()


def test_refine_frame_asks_for_stages_with_complete():
    from sdflabel_amd.pipelines.frame import refine_frame
    with pytest.raises(ValueError, match="complete needs return_stages"):
        refine_frame([], None, type("G", (), {"points": torch.zeros((1, 3))})(), [], None, None, 1, {}, complete=True)


# ---- the trajectory cases and their bound -----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def trajectories():
    """name -> (float64 run with its kink margins, float32 emulation run); computed once"""
    return {name: CC.cpu_runs(name) for name in ET.NAMES}


@pytest.mark.parametrize("name", ET.NAMES)
def test_float64_run_admits_every_row_of_the_trajectory_cases(trajectories, name):
    ref, _ = trajectories[name]
    assert ref["margin"].shape == (ET.STEPS, ET.B * ET.K)
    assert ref["margin"].min() > 1.0, float(ref["margin"].min())                 # no row within m = 100 fwd_tol of a kink on any step
    assert np.isinf(ref["margin"]).sum() == ET.STEPS * ET.B * (ET.K // 6)        # the invalid rows, and only they, are outside the rule
    assert not ref["flags"].any() and np.abs(ref["z"] - ref["z0"]).max() > 1e-3


@pytest.mark.parametrize("name", ET.NAMES)
def test_trajectory_bound_is_four_times_the_emulations_worst_deviation(trajectories, name):
    ref, emu = trajectories[name]
    worst = max(float(np.abs(a - b).max()) for a, b in zip(emu["zs"], ref["zs"]))
    print("%s: emulation deviates %.3e from float64 over %d steps; bound %.3e" % (name, worst, ET.STEPS, CC.TRAJECTORY_BOUND[name]))
    assert worst > 0
    assert 4 * worst <= CC.TRAJECTORY_BOUND[name] <= 4 * worst * 1.05, (worst, CC.TRAJECTORY_BOUND[name])


def test_completion_case_reference_lowers_the_loss_and_the_whole_shapes_residual():
    """the end-to-end case of tests/test_gpu_complete.py in float64, at the seed chosen here on the CPU (seed 0, the first tried)"""
    case, ref = CT.completion_case(), CT.completion_reference()
    h = ref["history"]
    print("completion: float64 loss %.4e -> %.4e; residual on the whole shape %.4e -> %.4e; cosine to the true latent %.4f; %d points, %d rows"
          % (h[0], h[-1], ref["residual_start"], ref["residual_end"], ref["cosine"], len(case["cloud"]), len(case["rows4"])))
    assert not ref["flags"].any() and len(h) == CT.COMPLETION["iters"]
    assert h[-1] < h[0], (h[0], h[-1])
    assert ref["residual_end"] < ref["residual_start"], (ref["residual_end"], ref["residual_start"])
    rows = case["rows4"].reshape(len(case["cloud"]), 7, 5)
    free = np.isfinite(rows[:, 3:, 3])
    assert np.isfinite(rows[:, :3, 3]).all() and free.any() and not free.all()       # the cloud lies inside the cube; some rays leave it
    assert (np.diff(free.astype(int), axis=1) <= 0).all()                              # a ray that has left the cube does not come back
    # the cloud stands for observed surface points: every vertex must lie closer to the shape than the offset eta of the normal rows,
    # or the signs of those rows would mean nothing
    assert np.abs(CT._values(case["z_true"][0], case["vertices"])[0]).max() < CT.COMPLETION["eta"]
