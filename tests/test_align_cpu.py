"""The pose-and-shape fit to one view without a GPU: the numpy restatement (tests/_align_ref.py) against torch float64 autograd +
torch.optim.Adam with each of yaw, trans, scale and latent frozen in turn, its six gradient formulas against central differences,
csrc/align_cells.h compiled into a host program (tests/align_host/align_host.cpp) against the restatement bit for bit -- also under
ASan/UBSan with exact-size buffers and broken tables --, the identity with the completion's reduce at scale 1, exports / header / binding,
argument checks, the calibration of the trajectory bound of tests/test_gpu_align.py on the float32 emulation, and the recovery of a pose
from the completion fixture's cloud in float64.
"""
import copy
import os
import re

import numpy as np
import pytest
import torch

from sdflabel_amd import _lib
from tests import _align_cases as AC
from tests import _align_ref as AR
from tests import _align_traj as AT
from tests import _complete_ref as CR
from tests import _encode_ref as ER
from tests import _encode_traj as ET
from tests import _prior_train_cases as PC
from tests._prior_train_loop import plain_forward
from tests._util import build_host_program
from tests.test_complete_cpu import _f32_bits, _f64_bits, _run, _split, same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement's loop against torch ------------------------------------------------------------------------------------------------

def _torch_loss(dec, zn, th, q, lo, hi, ok_rows, clamp):
    """per-shape loss [B] written from x(theta), scale * f and the interval distance.  zn [B][L], th: five [B] tensors (yaw, tx, ty, tz,
    scale), q [B][k][3]; a row whose x leaves the cube is left out for this evaluation (the mask is a constant)."""
    yaw, tx, ty, tz, sc = (t[:, None] for t in th)
    B, k = q.shape[:2]
    c, sn = torch.cos(yaw), torch.sin(yaw)
    q0, q1, q2 = q[:, :, 0] / sc - tx, q[:, :, 1] / sc - ty, q[:, :, 2] / sc - tz
    x = torch.stack([c * q0 - sn * q2, -q1, sn * q0 + c * q2], 2)
    inside = (x.detach().abs() <= 1).all(2)
    x = torch.where(inside[:, :, None], x, torch.zeros_like(x))
    inputs = torch.cat([zn.repeat_interleave(k, 0), x.reshape(-1, 3)], 1)
    cp = (sc * plain_forward(dec, inputs)[:, 0].reshape(B, k)).clamp(-clamp, clamp)
    dist = torch.relu(lo - cp) + torch.relu(cp - hi)
    ok = ok_rows & inside
    return torch.where(ok, dist, torch.zeros_like(dist)).sum(1) / ok.sum(1), inside


def _torch_fit(dec, samples, soff, z0, theta0, iters, k, lr, lr_pose, lr_step, lr_factor, clamp, code_reg, unit):
    """float64 autograd + torch.optim.Adam on the first k rows of every shape; one parameter group per learning rate, a rate of 0 frozen.
    The total is the SUM over shapes, so a shape's gradient is its own."""
    dec = copy.deepcopy(dec).double()
    for p in dec.parameters():
        p.requires_grad_(False)
    z = torch.tensor(np.asarray(z0, np.float64), requires_grad=lr != 0)
    th = [torch.tensor(np.asarray(theta0, np.float64)[:, i].copy(), requires_grad=lr_pose[i] != 0) for i in range(5)]
    groups = [{"params": [p], "lr": r, "base": r} for p, r in zip([z] + th, [lr] + list(lr_pose)) if r != 0]
    opt = torch.optim.Adam(groups)
    B = z.shape[0]
    rows = torch.tensor(np.stack([np.asarray(samples, np.float64)[int(soff[b]):int(soff[b]) + k] for b in range(B)]))      # [B][k][5]
    ok = (rows[:, :, 3] <= rows[:, :, 4]) & (torch.isfinite(rows[:, :, 3]) | torch.isfinite(rows[:, :, 4]))
    lo, hi = torch.nan_to_num(rows[:, :, 3], nan=0.0).clamp(-clamp, clamp), torch.nan_to_num(rows[:, :, 4], nan=0.0).clamp(-clamp, clamp)
    losses = []
    for it in range(iters):
        for grp in opt.param_groups:
            grp["lr"] = grp["base"] * lr_factor ** (it // lr_step)
        zn = z / z.norm(dim=1, keepdim=True) if unit else z
        per, _ = _torch_loss(dec, zn, th, rows[:, :, :3], lo, hi, ok, clamp)
        loss = per.sum() if unit else (per + code_reg * z.norm(dim=1)).sum()
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        losses.append(per.detach().numpy().copy())
    return z.detach().numpy(), np.stack([t.detach().numpy() for t in th], 1), np.array(losses)


FROZEN = {None: {}, "yaw": {0: 0.0}, "trans": {1: 0.0, 2: 0.0, 3: 0.0}, "scale": {4: 0.0}, "latent": {}}


@pytest.mark.parametrize("name,unit,frozen", [("w128", u, f) for u in (True, False) for f in FROZEN] + [("lat8", True, None), ("lat8", False, None)],
                         ids=lambda v: "all" if v is None else ("no_" + v if v in FROZEN else str(v)))
def test_restatement_loop_equals_torch_float64_autograd_and_adam(name, unit, frozen):
    dec, net = PC.decoders()[name], PC.net(name)
    samples, soff, z0, theta0, k, clamp = AC.fit_case(name, 3, 3, 66)
    lr_pose = [0.0 if i in FROZEN[frozen] else r for i, r in enumerate((4e-3, 3e-3, 2e-3, 3e-3, 5e-3))]
    kw = dict(lr=0.0 if frozen == "latent" else 5e-3, lr_pose=lr_pose, lr_step=5, lr_factor=0.1, clamp=clamp, code_reg=1e-4)
    seen = {}

    def watch(it, inputs, pred, lo, hi, J, pose):
        if it == 0:
            seen.update(pm=np.repeat(pose[:, 5], k) * pred, lo=lo, hi=hi)

    ref = AR.loop(ET.decoder64(net), samples, soff, z0, theta0, 10, k, False, unit=unit, ft=np.float64, watch=watch, **kw)
    # the mix at the start: exact, one-sided, satisfied and invalid rows, and exactly one row with usable bounds that leaves the cube
    kinds = np.arange(k) % 6
    given = np.isfinite(samples[:k, 3])
    assert (samples[:k, 3] == samples[:k, 4])[kinds < 2].all() and (samples[:k, 3] < samples[:k, 4])[(kinds >= 2) & (kinds < 5)].all() and not given[kinds == 5].any()
    left = given & ~np.isfinite(seen["lo"][:k])
    assert left[AC.OUTSIDE_ROW] and 1 <= left.sum() <= 3                         # (the start is off the true pose: a row next to a face may leave too)
    e, w, ok = CR.row_rule(seen["pm"], seen["lo"], seen["hi"], clamp)
    assert (w[:k][kinds < 4] != 0).sum() > k // 3 and (ok[:k] & (e[:k] == 0))[kinds == 4].any()
    z_t, th_t, losses = _torch_fit(dec, samples, soff, z0, theta0, 10, k, unit=unit, **kw)
    assert np.abs(ref["z"] - z_t).max() <= 1e-12, float(np.abs(ref["z"] - z_t).max())
    assert np.abs(ref["theta"] - th_t).max() <= 1e-12, float(np.abs(ref["theta"] - th_t).max())
    assert np.abs(ref["history"] - losses).max() <= 1e-12
    moved = np.abs(ref["theta"] - theta0.astype(np.float64)).max(0)
    for i in range(5):
        assert (moved[i] == 0) if lr_pose[i] == 0 else (moved[i] > 1e-4), (i, moved)
    assert (np.abs(ref["z"] - z0).max() == 0) if frozen == "latent" else (np.abs(ref["z"] - z0).max() > 1e-3)
    assert not ref["flags"].any()


def test_gradient_formulas_agree_with_central_differences_of_the_float64_loss():
    name = "w128"
    dec = copy.deepcopy(PC.decoders()[name]).double()
    net = PC.net(name)
    samples, soff, z0, theta0, k, clamp = AC.fit_case(name, 3, 3, 66)
    B, L = z0.shape
    zn = ER.normalised(z0.astype(np.float64), True, np.float64)
    theta = theta0.astype(np.float64)
    rows = torch.tensor(np.stack([samples[int(soff[b]):int(soff[b]) + k].astype(np.float64) for b in range(B)]))
    ok = (rows[:, :, 3] <= rows[:, :, 4]) & (torch.isfinite(rows[:, :, 3]) | torch.isfinite(rows[:, :, 4]))
    lo, hi = torch.nan_to_num(rows[:, :, 3], nan=0.0).clamp(-clamp, clamp), torch.nan_to_num(rows[:, :, 4], nan=0.0).clamp(-clamp, clamp)

    def loss_at(zn_, theta_):
        with torch.no_grad():
            per, inside = _torch_loss(dec, torch.tensor(zn_), [torch.tensor(theta_[:, i].copy()) for i in range(5)], rows[:, :, :3], lo, hi, ok, clamp)
        return per.numpy(), inside.numpy()

    # the analytic gradient: the restatement's float64 reduce on the float64 decoder's values
    pose = AR.pose_row(theta, np.float64)
    cam = rows[:, :, :3].reshape(-1, 3).numpy()
    x = AR.lattice_x(cam, np.repeat(pose, k, 0))
    inside = (np.abs(x) <= 1).all(1)
    inputs = np.concatenate([np.repeat(zn, k, 0), np.where(inside[:, None], x, 0.0)], 1)
    pred, J = ET.decoder64(net)(inputs)
    lo_r, hi_r = (np.where(inside, rows[:, :, c].reshape(-1).numpy(), np.nan) for c in (3, 4))
    _, g, _ = AR.reduce64(pred, lo_r, hi_r, J, cam, pose, L, B, k, clamp, np.zeros(B, np.int32))
    base, inside0 = loss_at(zn, theta)
    h = 1e-6
    worst = 0.0
    for col in range(L + 5):
        plus_z, minus_z, plus_t, minus_t = zn.copy(), zn.copy(), theta.copy(), theta.copy()
        if col < L:
            plus_z[:, col] += h
            minus_z[:, col] -= h
        else:
            plus_t[:, col - L] += h
            minus_t[:, col - L] -= h
        (lp, ip), (lm, im) = loss_at(plus_z, plus_t), loss_at(minus_z, minus_t)
        assert (ip == inside0).all() and (im == inside0).all()                  # no row crossed a face inside the stencil
        fd = (lp - lm) / (2 * h)
        rel = np.abs(fd - g[:, col]).max() / max(np.abs(g[:, col]).max(), 1e-12)
        worst = max(worst, rel)
        assert np.abs(g[:, col]).max() > 1e-4, col                              # every column carries a gradient
    # central differences with h = 1e-6 on a piecewise-linear loss: truncation 0 away from kinks, rounding 1e-16 / 1e-6 = 1e-10 absolute on
    # gradients of 1e-3 .. 1; a row that crosses a kink inside the stencil adds |slope change| h / k.  1e-5 relative is the "5 digits" of
    # the fit's statement
    print("gradient formulas against central differences: worst relative difference %.3e" % worst)
    assert worst <= 1e-5, worst


# ---- the header on the host -----------------------------------------------------------------------------------------------------------------

def host_samples(exe, tmp, pts, nrm, ptoff, origin, F, eta, s_max, seed, shape0=0, N=None):
    N = len(pts) if N is None else N
    B = len(ptoff) - 1
    arrays = [np.asarray(ptoff, np.int64), origin, np.asarray(pts, np.float32)[:N]] + ([np.asarray(nrm, np.float64)[:N]] if nrm is not None else [])
    blob = _run(exe, "samples", tmp, [N, B, F, shape0, seed, _f64_bits(eta), _f64_bits(s_max), int(nrm is not None)], arrays)
    return _split(blob, [(np.float32, (N * (3 + F), 5)), (np.int32, (B,))])


def host_rows(exe, tmp, samples, soff, B, k, draw, seed, it, z, unit, pose, S=None, shape0=0):
    L = z.shape[1]
    S = len(samples) if S is None else S
    blob = _run(exe, "rows", tmp, [S, B, k, draw, seed, it, L, unit, shape0], [np.asarray(soff, np.int64), np.asarray(samples, np.float32)[:S], z, pose])
    return _split(blob, [(np.float32, (B * k, L + 3)), (np.float32, (B * k, 3)), (np.float32, (B * k,)), (np.float32, (B * k,)), (np.float32, (B, L)),
                         (np.int32, (B,))])


def host_reduce(exe, tmp, pred, lo, hi, J, cam, pose, L, B, k, clamp, flags):
    blob = _run(exe, "reduce", tmp, [B, k, L, J.shape[1], _f32_bits(clamp)], [pred, lo, hi, J, cam, pose, flags])
    ch = (k + ER.CHUNK - 1) // ER.CHUNK
    loss, g, part, fl = _split(blob, [(np.float64, (B,)), (np.float64, (B, L + 5)), (np.float64, (B, ch, L + 7)), (np.int32, (B,))])
    return loss, g, fl, part


def host_step(exe, tmp, z, m, v, theta, tm, tv, pose, g, flags, unit, code_reg, lr, lr_pose, t):
    B, L = z.shape
    blob = _run(exe, "step", tmp, [B, L, unit, t, _f32_bits(code_reg), _f32_bits(lr)], [np.asarray(lr_pose, np.float32), z, m, v, theta, tm, tv, pose, g, flags])
    return _split(blob, [(np.float32, (B, L))] * 3 + [(np.float32, (B, 5))] * 3 + [(np.float32, (B, 6)), (np.int32, (B,))])


def same_step(got, want, what):
    """every word of a step bit for bit, but the cos / sin words of the pose rows: within one float32 ulp"""
    for g, w, n in zip(got, want, ("z", "m", "v", "theta", "tm", "tv", "pose", "flags")):
        if n == "pose":
            same_bits(g[:, 2:], w[:, 2:], (what, n))
            assert (np.abs(g[:, :2].view(np.int32).astype(np.int64) - w[:, :2].view(np.int32).astype(np.int64)) <= 1).all(), (what, "cos / sin")
        else:
            same_bits(g, w, (what, n))


def check_step_case(case, want):
    """what each step case was built to show, on the restatement's result"""
    B, L, unit, t, rates = case
    z, m, v, theta, tm, tv, pose, g, flags, code_reg, lr, lr_pose = AC.step_case(*case)
    skipped = (want[7] & ER.SKIPPED) != 0
    assert not skipped[0] and (want[3][0] != theta[0]).any() == (rates != "frozen_pose")
    for b in np.nonzero(skipped)[0]:
        for a, w in zip((z, m, v, theta, tm, tv, pose), want[:7]):
            same_bits(np.array(a[b]), w[b], (case, "skipped shape kept", b))
    for i in range(5):
        if lr_pose[i] == 0:
            same_bits(want[3][:, i], np.array(theta[:, i])); same_bits(want[4][:, i], np.array(tm[:, i])); same_bits(want[5][:, i], np.array(tv[:, i]))
    if lr == 0:
        same_bits(want[0], np.array(z)); same_bits(want[1], np.array(m))
    if B == 3:
        assert skipped[2] == (lr_pose[4] != 0)                                      # the scale that would turn negative
    if B == 5:
        assert skipped[1:].all()                                                    # an infinite scale gradient, empty, NaN, overflow
    assert np.isfinite(want[6][~skipped]).all() and (want[6][~skipped, 5] > 0).all()


def _host_checks(exe, tmp):
    # the observation rows
    for case in AC.sample_cases():
        B, counts, F, normals, special = case
        pts, ptoff, origin, nrm = AC.sample_case(*case)
        for shape0 in (0, 9):
            got = host_samples(exe, tmp, pts, nrm, ptoff, origin, F, AC.ETA, AC.S_MAX, AC.SEED, shape0)
            want = AR.sample_rows(pts, nrm, ptoff, origin, F, AC.ETA, AC.S_MAX, AC.SEED, shape0)
            same_bits(got[0], want[0], (case, "rows")); same_bits(got[1], want[1], (case, "flags"))
        _sample_case_properties(case, want)
    pts, ptoff, origin, nrm = AC.sample_case(3, (65, 65, 65), 4, "holes", "bad_points")
    for broken in AC.BROKEN_PTOFF:
        for N in (195, 100):
            got = host_samples(exe, tmp, pts, nrm, broken, origin, 4, AC.ETA, AC.S_MAX, AC.SEED, N=N)
            want = AR.sample_rows(pts[:N], nrm[:N], broken, origin, 4, AC.ETA, AC.S_MAX, AC.SEED, N=N)
            same_bits(got[0], want[0], (broken, N)); same_bits(got[1], want[1], (broken, N))
            bad = [a < 0 or e < a or e > N for a, e in zip(broken[:-1], broken[1:])]
            assert [bool(f & CR.BAD_TABLE) for f in want[1]] == bad, (broken, N)
            nobody = np.array([CR.owner(broken, 3, N, g) < 0 for g in range(N)])
            assert not np.isfinite(want[0].reshape(N, 7, 5)[nobody, :, 3]).any()
    # the iteration's rows
    for case in AC.rows_cases():
        B, counts, k, draw, L, unit, bad_pose = case
        samples, soff, z, pose = AC.rows_case(*case)
        got = host_rows(exe, tmp, samples, soff, B, k, draw, AC.SEED, 17, z, unit, pose, shape0=2)
        want = AR.rows(samples, soff, B, k, draw, AC.SEED, 17, z, unit, pose, shape0=2)
        for g, w, n in zip(got, want, ("inputs", "cam", "lo", "hi", "zn", "flags")):
            same_bits(g, w, (case, n))
        _rows_case_properties(case, want)
    samples, soff, z, pose = AC.rows_case(3, (65, 0, 72), 65, 0, 8, 0, 2)
    for broken, S in AC.BROKEN_SOFF[:4]:
        got = host_rows(exe, tmp, samples, broken, 3, 64, 1, AC.SEED, 0, z, 0, pose, S=S)
        want = AR.rows(samples[:S], broken, 3, 64, 1, AC.SEED, 0, z, 0, pose, S=S)
        for g, w in zip(got, want):
            same_bits(g, w, broken)
        assert (want[5] & ER.BAD_TABLE).any()
    # the reduce
    for case in AC.reduce_cases():
        B, k, L, Js, bad_pose = case
        pred, lo, hi, J, cam, pose, flags = AC.reduce_case(*case)
        got = host_reduce(exe, tmp, pred, lo, hi, J, cam, pose, L, B, k, AC.CLAMP, flags)
        want = AR.reduce(pred, lo, hi, J, cam, pose, L, B, k, AC.CLAMP, flags)
        for g, w, n in zip(got, want, ("loss", "g", "flags", "part")):
            same_bits(g, w, (case, n))
        _reduce_case_properties(case, want)
        # at scale == 1 the loss and the latent columns are the completion's reduce in every bit
        pred, lo, hi, J, cam, pose, flags = AC.reduce_case(B, k, L, Js, -1, unit_scale=True)
        got = host_reduce(exe, tmp, pred, lo, hi, J, cam, pose, L, B, k, CR_CLAMP, flags)
        cpl = CR.reduce(pred, lo, hi, J, L, B, k, CR_CLAMP, flags)
        same_bits(got[0], cpl[0], (case, "scale 1", "loss")); same_bits(got[1][:, :L], cpl[1], (case, "scale 1", "g_zn"))
        same_bits(got[2], cpl[2], (case, "scale 1", "flags")); same_bits(got[3][:, :, :L], cpl[3][:, :, :L], (case, "scale 1", "part"))
        same_bits(got[3][:, :, L + 5:], cpl[3][:, :, L:], (case, "scale 1", "part: loss and count"))
    # the step
    for case in AC.step_cases():
        B, L, unit, t, rates = case
        z, m, v, theta, tm, tv, pose, g, flags, code_reg, lr, lr_pose = AC.step_case(*case)
        got = host_step(exe, tmp, z, m, v, theta, tm, tv, pose, g, flags, unit, code_reg, lr, lr_pose, t)
        want = AR.step(z, m, v, theta, tm, tv, pose, g, flags, unit, code_reg, lr, lr_pose, t)
        same_step(got, want, case)
        check_step_case(case, want)


CR_CLAMP = 0.1                               # the completion's own clamp, for the scale-1 identity


def _sample_case_properties(case, want):
    B, counts, F, normals, special = case
    rows, flags = want
    P, N = 3 + F, sum(counts)
    valid = np.isfinite(rows[:, 3]).reshape(N, P) if N else np.zeros((0, P), bool)
    assert not flags.any() and (rows[~valid.reshape(-1), :3] == 0).all()
    if special == "bad_points":
        assert not valid[[3, 70, 140]].any() and valid[:, 0].sum() == N - 3
    elif N:
        assert valid[:, 0].all()                                                     # no cube in the camera frame: every finite point stands
    if normals == "none":
        assert not valid[:, 1:3].any()
    elif normals == "holes" and N >= 65:
        assert valid[:, 1].any() and (valid[:, 0] & ~valid[:, 1]).any()
    if special == "on_sensor":
        on = np.nonzero(valid[:, 0] & ~valid[:, 3:].any(1))[0]
        assert len(on) >= 1 and valid[on[0], 1]
    if F and N >= 65:
        free = rows.reshape(N, P, 5)[:, 3:]
        v = valid[:, 3:]
        assert v.any() and (free[v][:, 3] == 0).all() and (free[v][:, 4] >= 0).all() and (free[v][:, 4] <= np.float32(AC.S_MAX)).all()
        if F > 1:
            with np.errstate(invalid="ignore"):
                assert not (np.diff(np.where(v, free[:, :, 4], np.nan), axis=1) < 0).any()


def _rows_case_properties(case, want):
    B, counts, k, draw, L, unit, bad_pose = case
    inputs, cam, lo, hi, zn, flags = want
    samples, soff, z, pose = AC.rows_case(*case)
    assert (np.abs(inputs[:, L:]) <= 1).all()
    if B == 3:
        assert flags[1] == ER.EMPTY and not inputs[k:2 * k].any() and not cam[k:2 * k].any()
    for b in range(B):
        sl = slice(b * k, (b + 1) * k)
        if b == bad_pose:
            assert flags[b] == AR.BAD_POSE and not np.isfinite(lo[sl]).any() and not inputs[sl, L:].any() and cam[sl].any()
        elif counts[b]:
            assert flags[b] == 0
            if k >= 63:
                given = np.isfinite(lo[sl])
                assert given.any() and (~given & (inputs[sl, L:] == 0).all(1)).any()       # rows that stay and rows that leave the cube
    if not draw and bad_pose != 0:
        assert inputs[0, L] == 1.0 and np.isfinite(lo[0])                             # the row on the face stays
        if k > 1:
            assert not inputs[1, L:].any() and np.isnan(lo[1]) and (cam[1] == AC.BEYOND).all()    # one float32 step beyond: left out


def _reduce_case_properties(case, want):
    B, k, L, Js, bad_pose = case
    loss, g, flags, part = want
    for b in range(B):
        if b == bad_pose or (B >= 2 and b == 1):
            assert flags[b] & ER.NO_ROWS and loss[b] == 0 and not g[b].any()
        else:
            assert not flags[b] & ER.NO_ROWS and np.isfinite(loss[b])
    if bad_pose != 0:
        assert np.isfinite(g[0, :L]).all() and (k < 8 or g[0].any())


def test_align_cells_on_the_host_equal_the_restatement_bit_for_bit(tmp_path):
    _host_checks(build_host_program(tmp_path, "align_host/align_host.cpp", "align_host"), tmp_path)


def test_align_cells_host_program_under_sanitizers(tmp_path):
    _host_checks(build_host_program(tmp_path, "align_host/align_host.cpp", "align_host_san",
                                    ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]), tmp_path)


def test_restatement_at_identity_pose_and_exact_rows_is_the_completions_reduce_in_every_bit():
    """lo == hi, scale == 1, identity pose: the loss and the latent gradient of _complete_ref.reduce, and of the encoder's"""
    for B, k, L, Js in ((3, 65, 3, 6), (1, 1025, 40, 43), (3, 2049, 8, 16)):
        pred, lo, hi, J, cam, pose, flags = (np.array(a) for a in AC.reduce_case(B, k, L, Js, -1, unit_scale=True))
        pose[:] = [1, 0, 0, 0, 0, 1]
        got = AR.reduce(pred, lo, lo, J, cam, pose, L, B, k, CR_CLAMP, flags)
        for want in (CR.reduce(pred, lo, lo, J, L, B, k, CR_CLAMP, flags), ER.reduce(pred, lo, J, L, B, k, CR_CLAMP, flags)):
            same_bits(got[0], want[0], "loss"); same_bits(got[1][:, :L], want[1], "g_zn"); same_bits(got[2], want[2], "flags")
        assert np.isfinite(got[1][0, :L]).all() and (got[1][0, L:] != 0).all()          # and the pose columns are there


# ---- exports, header, binding -------------------------------------------------------------------------------------------------------------

NAMES = ("sdfr_align_samples", "sdfr_align_rows", "sdfr_align_reduce", "sdfr_align_step")


def test_exports_header_and_binding_agree():
    from sdflabel_amd import align as A
    header = open(os.path.join(ROOT, "include", "sdfr.h")).read()
    assert _lib.ABI_VERSION >= 420 and int(re.search(r"#define SDFR_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION
    assert "420: pose and shape fitted to one view" in header
    body = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    h = _lib.lib()
    assert h.sdfr_version() == _lib.ABI_VERSION
    for name in NAMES:
        assert name in _lib.EXPORTS and hasattr(h, name) and re.search(r"\bint %s\(" % name, body), name
        args = re.search(r"\bint %s\((.*?)\);" % name, body, flags=re.S).group(1)
        assert len(args.split(",")) == len(_lib._PROTOS[name][1]), name
    assert "sdfr_align_ws_bytes" in _lib.EXPORTS and re.search(r"\bint64_t sdfr_align_ws_bytes\(", body)
    assert h.sdfr_align_ws_bytes(3, 2049, 8) == 3 * 3 * (8 + 7) * 8 and h.sdfr_align_ws_bytes(1, 0, 8) == -1 and h.sdfr_align_ws_bytes(1, 5, 257) == -1
    cells = open(os.path.join(ROOT, "sdflabel_amd", "csrc", "align_cells.h")).read()
    for name, val in (("ALN_ROW", 5), ("ALN_POSE", AR.POSE), ("ALN_BAD_POSE", AR.BAD_POSE)):
        assert int(re.search(r"#define %s (\d+)" % name, cells).group(1)) == val, name
    assert (A.BAD_POSE, A.BAD_TABLE) == (AR.BAD_POSE, CR.BAD_TABLE)
    assert "verify_point_x" in cells and "complete_cells.h" in cells and "train_mix64" not in cells
    # one copy of the summation order: the reduce kernels live in one header, instantiated by the three translation units
    units = [open(os.path.join(ROOT, "sdflabel_amd", "csrc", n)).read() for n in ("encode.hip", "complete.hip", "align.hip")]
    assert all("enc_tree_step" not in u and "ENC_SLOT_ROWS" not in u and "encode_kernels.h" in u for u in units)
    assert "align.hip" in open(os.path.join(ROOT, "sdflabel_amd", "csrc", "build.sh")).read()


def test_c_argument_checks_need_no_gpu():
    import ctypes
    h = _lib.lib()
    d, inv = 4096, -1            # never dereferenced: every call below is refused before a launch
    rates = (ctypes.c_float * 5)(1e-2, 1e-2, 1e-2, 1e-2, 0.0)
    assert h.sdfr_align_samples(d, d, 10, d, 1, d, 0, 65, 0.02, 1.0, 0, d, d, None) == inv and b"free-space" in h.sdfr_last_error()
    assert h.sdfr_align_samples(d, d, 10, None, 1, d, 0, 4, 0.02, 1.0, 0, d, d, None) == inv and b"NULL" in h.sdfr_last_error()
    assert h.sdfr_align_samples(d, d, 10, d, 0, d, 0, 4, 0.02, 1.0, 0, d, d, None) == inv and b"without a shape" in h.sdfr_last_error()
    assert h.sdfr_align_samples(d, d, 10, d, 1, d, 0, 4, float("inf"), 1.0, 0, d, d, None) == inv and b"eta" in h.sdfr_last_error()
    assert h.sdfr_align_samples(d, d, 10, d, 1, d, 0, 4, 0.02, -1.0, 0, d, d, None) == inv
    assert h.sdfr_align_samples(d, d, 10, d, 2, d, 65534, 4, 0.02, 1.0, 0, d, d, None) == inv and b"shape0" in h.sdfr_last_error()
    assert h.sdfr_align_samples(d, d, (1 << 32) + 1, d, 1, d, 0, 4, 0.02, 1.0, 0, d, d, None) == inv and b"2^32" in h.sdfr_last_error()
    assert h.sdfr_align_samples(d, d, 0, d, 0, d, 0, 4, 0.02, 1.0, 0, d, d, None) == 0
    assert h.sdfr_align_rows(d, 10, d, 1, 0, 5, 0, 0, 0, d, 3, 1, None, d, d, d, d, d, d, None) == inv and b"sdfr_align_rows: NULL" in h.sdfr_last_error()
    assert h.sdfr_align_rows(d, 10, d, 1, 0, 5, 0, 0, 0, d, 3, 1, d, d, None, d, d, d, d, None) == inv and b"NULL" in h.sdfr_last_error()
    assert h.sdfr_align_rows(d, 10, d, 1, 0, 0, 0, 0, 0, d, 3, 1, d, d, d, d, d, d, d, None) == inv and b"k = 0" in h.sdfr_last_error()
    assert h.sdfr_align_rows(d, 10, d, 1, 0, 5, 0, 0, 0, d, 257, 1, d, d, d, d, d, d, d, None) == inv and b"latent size" in h.sdfr_last_error()
    assert h.sdfr_align_rows(d, 10, d, 1, 0, 5, 0, 0, 1 << 24, d, 3, 1, d, d, d, d, d, d, d, None) == inv and b"iter" in h.sdfr_last_error()
    assert h.sdfr_align_rows(d, 10, d, 0, 0, 5, 0, 0, 0, d, 3, 1, d, d, d, d, d, d, d, None) == 0
    assert h.sdfr_align_reduce(d, d, d, d, 5, d, d, 3, 1, 5, 0.2, d, 1 << 20, d, d, d, None) == inv and b"stride" in h.sdfr_last_error()
    assert h.sdfr_align_reduce(d, d, d, d, 6, d, d, 3, 1, 5, 0.2, d, 79, d, d, d, None) == inv and b"sdfr_align_ws_bytes" in h.sdfr_last_error()
    assert h.sdfr_align_reduce(d, d, d, d, 6, d, d, 3, 1, 5, 0.0, d, 80, d, d, d, None) == inv and b"clamp" in h.sdfr_last_error()
    assert h.sdfr_align_reduce(d, d, d, d, 6, None, d, 3, 1, 5, 0.2, d, 80, d, d, d, None) == inv and b"sdfr_align_reduce: NULL" in h.sdfr_last_error()
    assert h.sdfr_align_reduce(d, d, d, d, 6, d, d, 3, 0, 5, 0.2, d, 0, d, d, d, None) == 0
    assert h.sdfr_bound_reduce(d, d, d, d, 6, 3, 1, 5, 0.1, d, 39, d, d, d, None) == inv and b"sdfr_encode_ws_bytes" in h.sdfr_last_error()
    assert h.sdfr_align_step(d, d, d, 3, 1, 1, d, d, d, d, d, d, d, 1e-4, 5e-3, None, 1, None, 0, None) == inv and b"NULL" in h.sdfr_last_error()
    assert h.sdfr_align_step(d, d, d, 3, 1, 1, d, d, d, d, d, d, d, 1e-4, 5e-3, rates, 0, None, 0, None) == inv and b"starts at 1" in h.sdfr_last_error()
    assert h.sdfr_align_step(d, d, d, 3, 2, 1, d, d, d, d, d, d, d, 1e-4, 5e-3, rates, 1, d, 1, None) == inv and b"history_stride" in h.sdfr_last_error()
    rates[2] = float("nan")
    assert h.sdfr_align_step(d, d, d, 3, 1, 1, d, d, d, d, d, d, d, 1e-4, 5e-3, rates, 1, None, 0, None) == inv and b"non-finite" in h.sdfr_last_error()
    rates[2] = 0.0
    assert h.sdfr_align_step(d, d, d, 3, 0, 1, d, d, d, d, d, d, d, 1e-4, 5e-3, rates, 1, None, 0, None) == 0


def test_python_argument_checks_come_before_any_launch():
    from sdflabel_amd import align as A
    dec = PC.decoders()["w128"]                                                    # on the CPU
    p = {"yaw": torch.zeros(1), "trans": torch.zeros(3), "scale": torch.ones(1), "latent": torch.zeros(3)}
    cloud = np.zeros((4, 3), np.float32)
    for bad in (dict(iters=-1), dict(clamp=0.0), dict(rows_per_iter=0), dict(fit=("yaw", "roll")), dict(fit=()), dict(lr_pose=float("nan")),
                dict(lr_pose={"yaw": 1e-2, "pitch": 1e-2}), dict(lr_step=0), dict(free_rows=65), dict(s_max=-1.0), dict(eta=float("nan"))):
        with pytest.raises(ValueError):
            A.align_many(dec, [p], [cloud], **bad)
    with pytest.raises(ValueError):
        A.align_many(dec, [p], [cloud, cloud])
    with pytest.raises(ValueError):
        A.align_many(dec, [dict(p, latent=torch.zeros(8))], [cloud])
    with pytest.raises(ValueError):
        A.align_many(dec, [p], [cloud], normals=[])
    with pytest.raises(_lib.SdfrError, match="no CPU fallback"):
        A.align_many(dec, [p], [cloud])                                            # a CPU decoder
    with pytest.raises(ValueError):
        A.align_samples_many([cloud, cloud], normals=[cloud])
    with pytest.raises(ValueError):
        A.align_samples_many([cloud], free_rows=-1)
    with pytest.raises(_lib.SdfrError):
        A.align_samples_many([cloud], _device="cpu")
    assert A.align_samples_many([]) == []
    assert "camera-frame" in A.align_samples_many.__doc__ and "metric" in A.align_samples_many.__doc__
    assert "degenera" in A.align_many.__doc__ and "WITHOUT A CLAIMED OPERATING POINT" in A.__doc__


def test_refine_frame_asks_for_stages_with_align():
    from sdflabel_amd.pipelines.frame import refine_frame
    with pytest.raises(ValueError, match="align needs return_stages"):
        refine_frame([], None, type("G", (), {"points": torch.zeros((1, 3))})(), [], None, None, 1, {}, align=True)


# ---- the trajectory cases and their bound -----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def trajectories():
    """name -> (float64 run with its kink margins, float32 emulation run); computed once"""
    return {name: AC.cpu_runs(name) for name in ET.NAMES}


@pytest.mark.parametrize("name", ET.NAMES)
def test_float64_run_admits_every_row_of_the_trajectory_cases(trajectories, name):
    ref, _ = trajectories[name]
    assert ref["margin"].shape == (ET.STEPS, ET.B * ET.K) and ref["face"].shape == (ET.STEPS, ET.B * ET.K)
    assert ref["margin"].min() > 1.0, float(ref["margin"].min())                 # no row within 100 fwd_tol of a kink of the loss on any step
    assert ref["face"].min() > 1.0, float(ref["face"].min())                     # nor within 100 roundings of a face of the cube
    out = np.isinf(ref["margin"])                                                # outside the rule: the invalid rows, the row moved out of the cube,
    planted = np.tile(np.arange(ET.K) % 6 == 5, ET.B)                            # and the few the start's offset carries over a face
    planted[AC.OUTSIDE_ROW] = True
    assert out[:, planted].all() and out[:, ~planted].mean() < 0.1, (out[:, planted].all(), out[:, ~planted].mean())
    assert not ref["flags"].any() and np.abs(ref["z"] - ref["z0"]).max() > 1e-3 and (np.abs(ref["theta"] - ref["theta0"]).max(0) > 1e-3).all()


@pytest.mark.parametrize("name", ET.NAMES)
def test_trajectory_bound_is_four_times_the_emulations_worst_deviation(trajectories, name):
    ref, emu = trajectories[name]
    worst = AC.deviation(emu["trace"], ref["trace"])
    print("%s: emulation deviates %.3e from float64 over %d steps; bound %.3e" % (name, worst, ET.STEPS, AC.TRAJECTORY_BOUND[name]))
    assert worst > 0
    assert 4 * worst <= AC.TRAJECTORY_BOUND[name] <= 4 * worst * 1.05, (worst, AC.TRAJECTORY_BOUND[name])


def test_recovery_case_reference_lowers_the_loss_and_recovers_the_pose():
    """the end-to-end case of tests/test_gpu_align.py in float64: the completion fixture's cloud, the true latent, yaw and trans fitted from
    a start that is off in all four"""
    ref = AT.recovery_reference()
    h, err0, err1 = ref["history"], ref["error_start"], ref["error_end"]
    print("recovery: float64 loss %.4e -> %.4e; |error| in yaw, tx, ty, tz %s -> %s (seed %d)" % (h[0], h[-1], err0, err1, AT.RECOVERY["seed"]))
    assert not ref["flags"].any() and len(h) == AT.RECOVERY["iters"]
    assert h[-1] < h[0], (h[0], h[-1])
    assert (err0 > 0).all() and (err1 < 0.25 * err0).all(), (err0, err1)
    assert ref["theta"][0, 4] == np.float64(np.float32(AT.RECOVERY["scale"]))     # the scale was not fitted
