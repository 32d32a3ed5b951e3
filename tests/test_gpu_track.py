"""GPU tests of the joint fit of one shape to several views (csrc/track.hip, sdflabel_amd/track.py, sdflabel_amd/pipelines/sequence.py):
sdfr_track_step against the numpy restatement (tests/_track_ref.py) bit for bit between guard words, a track of one view against
sdfr_align_step, independence of the batch, align_tracks against align_many and against the restatement on the device's own decoder values,
staging, the calibrated trajectory bound, host traffic, the three-view case and label_sequence.
"""
import ctypes

import numpy as np
import pytest
import torch

from sdflabel_amd import _lib
from sdflabel_amd import align as A
from sdflabel_amd import track as T
from tests import _align_cases as AC
from tests import _align_ref as AR
from tests import _encode_ref as ER
from tests import _encode_traj as ET
from tests import _prior_train_cases as PC
from tests import _track_cases as TC
from tests import _track_ref as TR
from tests.test_gpu_align import ONE_CLAMP, ONE_RATES, _bound_samples, _params, dev_step
from tests.test_gpu_encode import DEV, Guarded, count_syncs, device_pred_and_J, gpu_decoder, same_bits, shapes_of, st
from tests._track_traj import NAMES as TRAJ_NAMES
from tests.test_track_cpu import same_track_step

pytestmark = pytest.mark.gpu

FLOATS = ("z", "m", "v", "scale", "sm", "sv", "theta", "tm", "tv", "pose", "z_view")


def dev_track_step(c):
    """sdfr_track_step on guarded device copies of a case dict (tests/_track_cases.step_case's keys); a dict of every array after the call"""
    Tn, L, V, t = c["T"], c["L"], c["V"], c["t"]
    f = {k: Guarded(np.array(c[k], np.float32)) for k in FLOATS}
    voff, g, vl = Guarded(np.asarray(c["voff"], np.int64)), Guarded(np.asarray(c["g"], np.float64)), Guarded(np.asarray(c["view_loss"], np.float64))
    vf, ls, tf = Guarded(np.asarray(c["vflags"], np.int32).copy()), Guarded(np.asarray(c["loss"], np.float64).copy()), Guarded(np.asarray(c["tflags"], np.int32).copy())
    w = None if c["weight"] is None else Guarded(np.asarray(c["weight"], np.float32))
    stride = Tn + 2
    hist = Guarded(t * stride, torch.float32)
    hist.t[(t - 1) * stride:(t - 1) * stride + Tn] = torch.from_numpy(np.asarray(c["loss"]).astype(np.float32)).to(DEV)
    rates = (ctypes.c_float * 5)(*[float(r) for r in c["lr_pose"]])
    P = lambda x: x.t.data_ptr()
    _lib.check(_lib.lib().sdfr_track_step(P(f["z"]), P(f["m"]), P(f["v"]), L, Tn, c["unit"], P(f["scale"]), P(f["sm"]), P(f["sv"]), c["share"], P(voff), V,
                                          P(w) if w else None, P(f["theta"]), P(f["tm"]), P(f["tv"]), P(f["pose"]), P(f["z_view"]), P(g), P(vl), P(vf), P(ls), P(tf),
                                          float(c["code_reg"]), float(c["lr"]), rates, t, P(hist), stride, st()), "sdfr_track_step")
    torch.cuda.synchronize()
    for x in list(f.values()) + [voff, g, vl, vf, ls, tf, hist] + ([w] if w else []):
        assert x.intact()
    same_bits(g.numpy(), np.asarray(c["g"], np.float64).reshape(-1), "g is read only")
    same_bits(voff.numpy(), np.asarray(c["voff"], np.int64), "voff is read only")
    out = {"z": f["z"].numpy((Tn, L)), "m": f["m"].numpy((Tn, L)), "v": f["v"].numpy((Tn, L)), "scale": f["scale"].numpy(), "sm": f["sm"].numpy(),
           "sv": f["sv"].numpy(), "theta": f["theta"].numpy((V, 5)), "tm": f["tm"].numpy((V, 5)), "tv": f["tv"].numpy((V, 5)), "pose": f["pose"].numpy((V, 6)),
           "z_view": f["z_view"].numpy((V, L)), "vflags": vf.numpy(), "loss": ls.numpy(), "tflags": tf.numpy()}
    h = hist.numpy((t, stride))
    out["history"] = h[t - 1, :Tn].copy()
    h[t - 1, :Tn] = hist.sent
    assert (h == hist.sent).all()                                               # nothing but the track words of row t - 1
    return out


@pytest.mark.parametrize("case", TC.step_cases(), ids=TC.case_id)
def test_track_step_kernel_equals_the_restatement(case):
    c = TC.step_case(*case)
    want = TC.restate(c)
    same_track_step(dev_track_step(c), want, TC.case_id(case))
    TC.check_step_case(case, want)


@pytest.mark.parametrize("share", [0, 1])
def test_a_track_of_one_view_is_sdfr_align_step_in_every_bit(share):
    for case in AC.step_cases():
        B, L, unit, t, rates = case
        z, m, v, theta, tm, tv, pose, g, flags, code_reg, lr, lr_pose = AC.step_case(*case)
        g = np.array(g)
        g[0, 0], g[0, L + 1] = -0.0, -0.0
        loss = np.linspace(0.01, 0.02, B)
        want, _ = dev_step(z, m, v, theta, tm, tv, pose, g, flags, unit, code_reg, lr, lr_pose, t, loss=loss)
        stm, stv = np.array(tm), np.array(tv)
        if share:
            stm[:, 4], stv[:, 4] = 7.0, 7.0
        c = dict(z=z, m=m, v=v, scale=np.array(theta[:, 4]), sm=np.array(tm[:, 4]), sv=np.array(tv[:, 4]), voff=np.arange(B + 1), weight=None, theta=theta, tm=stm,
                 tv=stv, pose=pose, z_view=np.zeros_like(z), g=g, view_loss=loss, vflags=flags, loss=np.zeros(B), tflags=np.zeros(B, np.int32), code_reg=code_reg,
                 lr=lr, lr_pose=lr_pose, share=share, unit=unit, t=t, L=L, T=B, V=B)
        got = dev_track_step(c)
        gtm, gtv = got["tm"].copy(), got["tv"].copy()
        if share:
            assert (gtm[:, 4] == 7.0).all() and (gtv[:, 4] == 7.0).all()
            gtm[:, 4], gtv[:, 4] = got["sm"], got["sv"]
        for a, b, n in zip((got["z"], got["m"], got["v"], got["theta"], gtm, gtv, got["pose"], got["vflags"]), want, ("z", "m", "v", "theta", "tm", "tv", "pose", "flags")):
            same_bits(a, b, (case, share, n))                                    # (the same device: cos and sin too)
        stepped = (want[7] & 4) == 0
        assert stepped.any() and (got["tflags"][stepped] == 0).all() and (got["tflags"][~stepped] != 0).all()
        same_bits(got["loss"][stepped], loss[stepped], "loss")


def _tracks_of(c, order):
    """the case dict with its tracks in another order (views moved with them)"""
    voff = c["voff"]
    views = np.concatenate([np.arange(voff[t], voff[t + 1]) for t in order]).astype(np.int64)
    out = dict(c)
    for k in ("z", "m", "v", "scale", "sm", "sv", "loss", "tflags"):
        out[k] = np.asarray(c[k])[order]
    for k in ("theta", "tm", "tv", "pose", "z_view", "g", "view_loss", "vflags") + (("weight",) if c["weight"] is not None else ()):
        out[k] = np.asarray(c[k])[views]
    out["voff"] = np.concatenate([[0], np.cumsum([voff[t + 1] - voff[t] for t in order])]).astype(np.int64)
    out["T"], out["V"] = len(order), len(views)
    return out, views


def test_a_tracks_results_do_not_depend_on_the_batch_and_repeat():
    for case in (((1, 2, 5), 8, 1, 7, 1, "given", None), ((1, 2, 5), 40, 1, 1, 0, "zero", None)):
        c = TC.step_case(*case)
        whole = dev_track_step(c)
        again = dev_track_step(c)
        for k in TR.KEYS:
            same_bits(whole[k], again[k], ("twice", k))
        voff = c["voff"]
        for order in ([2, 0, 1], [1], [2]):
            moved_case, views = _tracks_of(c, order)
            moved = dev_track_step(moved_case)
            for k in ("z", "m", "v", "scale", "sm", "sv", "loss", "tflags", "history"):
                same_bits(whole[k][order], moved[k], (order, k))
            for k in ("theta", "tm", "tv", "pose", "z_view", "vflags"):
                same_bits(whole[k][views], moved[k], (order, k))


# ---- align_tracks ----------------------------------------------------------------------------------------------------------------------------

def _tracks(voff, z0, scale0, theta0):
    """align_tracks's input from a table, the tracks' start latents and scales and the views' start poses"""
    dev = lambda a: torch.as_tensor(np.array(a, np.float32)).reshape(-1).to(DEV)
    return [{"latent": dev(z0[t]), "scale": dev([scale0[t]]),
             "views": [{"yaw": dev(theta0[v, 0:1]), "trans": dev(theta0[v, 1:4]), "scale": dev(theta0[v, 4:5])} for v in range(int(voff[t]), int(voff[t + 1]))]}
            for t in range(len(voff) - 1)]


ALL = ("yaw", "trans", "scale", "latent")


@pytest.mark.parametrize("share", [True, False])
@pytest.mark.parametrize("name", ["asset", "f16"])
def test_align_tracks_with_one_view_per_track_is_align_many_in_every_bit(name, share):
    dec = gpu_decoder(name)
    B, k = 3, 64
    samples, soff, z0, theta0, k, clamp = AC.fit_case("asset", 1, B, k)
    kw = dict(iters=5, rows_per_iter=k, clamp=clamp, history=True, fit=ALL, lr=5e-3, lr_pose=1e-2, lr_step=3, seed=5)
    one = A.align_many(dec, [_params(theta0[b], z0[b]) for b in range(B)], None, samples=_bound_samples(samples, soff), **kw)
    out = T.align_tracks(dec, _tracks(np.arange(B + 1), z0, theta0[:, 4], theta0), samples=_bound_samples(samples, soff), share_scale=share, **kw)
    for a, b, n in ((out.raw_latents, one.raw_latents, "raw"), (out.latents, one.latents, "latents"), (out.theta, one.theta, "theta"), (out.loss, one.loss, "loss"),
                    (out.view_loss, one.loss, "view loss"), (out.history, one.history, "history"), (out.view_flags, one.flags, "flags")):
        same_bits(a.cpu().numpy(), b.cpu().numpy(), (name, share, n))
    same_bits(out.scale.cpu().numpy(), (one.theta if share else torch.from_numpy(np.array(theta0)))[:, 4].cpu().numpy(), "scale")
    assert not out.flags.any() and not one.flags.any() and out.voff == [0, 1, 2, 3]
    assert (one.theta.cpu().numpy() != theta0).all() and (one.raw_latents.cpu().numpy() != z0).any()
    p = out.params[1][0]
    assert [tuple(p[key].shape) for key in ALL] == [(1,), (3,), (1,), (int(dec.latent_size),)]
    assert p["latent"].data_ptr() == out.latents[1].data_ptr() and p["scale"].data_ptr() == (out.scale[1:] if share else out.theta[1, 4:]).data_ptr()


def _three_views(L, n=200):
    """three views over two tracks on random lattice rows, as test_gpu_align's one-iteration case builds its shapes"""
    lat, soff, z_all = shapes_of(L, 3, n)
    rng = np.random.default_rng(177 + L)
    theta, _ = AC.random_poses(rng, 3)
    voff = np.array(TC.FIT_VOFF, np.int64)
    own = TR.track_of(voff)
    scale0 = theta[voff[:-1], 4].copy()
    theta[:, 4] = scale0[own]
    pose = AR.pose_row(theta)
    samples = np.zeros((3 * n, 5), np.float32)
    for b in range(3):
        sl = slice(b * n, (b + 1) * n)
        samples[sl, :3] = AC.to_camera(1.1 * lat[sl, :3].astype(np.float64), pose[b]).astype(np.float32)      # some rows leave the cube
        samples[sl, 3] = theta[b, 4] * lat[sl, 3]
        samples[sl, 4] = samples[sl, 3] + np.where(np.arange(n) % 3 == 0, 0, 0.05).astype(np.float32)
    return samples, soff, voff, z_all[voff[:-1]], scale0, theta


@pytest.mark.parametrize("name", ["asset", "lat8", "f16", "ln"])
def test_one_iteration_equals_the_restatement_on_the_devices_own_decoder_values(name):
    dec = gpu_decoder(name)
    L, n = int(dec.latent_size), 200
    samples, soff, voff, z0, scale0, theta = _three_views(L, n)
    own = TR.track_of(voff)
    w = np.array(TC.FIT_WEIGHTS, np.float32)
    kw = dict(iters=1, rows_per_iter=n, clamp=ONE_CLAMP, seed=11, history=True, draw=False, weights=w, **ONE_RATES)
    out = T.align_tracks(dec, _tracks(voff, z0, scale0, theta), samples=_bound_samples(samples, soff), **kw)
    pose0 = AR.pose_row(theta)
    z_view = z0[own]
    inputs, cam, lo, hi, _, vflags = AR.rows(samples, soff, 3, n, False, 11, 0, z_view, True, pose0)
    assert np.isnan(lo).any() and np.isfinite(lo).mean() > 0.5
    pred, J = device_pred_and_J(dec, inputs)
    vloss, g, vflags, _ = AR.reduce(pred, lo, hi, J, cam, pose0, L, 3, n, ONE_CLAMP, vflags)
    zt, zv = np.zeros_like(z0), np.zeros_like(theta)
    want = TR.step(z0, zt, zt, scale0, np.zeros_like(scale0), np.zeros_like(scale0), 1, voff, w, theta, zv, zv, pose0, z_view, g, vloss, vflags, True, 1e-4, 5e-3,
                   (4e-3, 3e-3, 3e-3, 3e-3, 5e-3), 1)
    assert not want["tflags"].any() and not want["vflags"].any() and (np.abs(g).min(1) > 0).all()
    same_bits(out.raw_latents.cpu().numpy(), want["z"], name)
    same_bits(out.theta.cpu().numpy(), want["theta"], name)
    same_bits(out.scale.cpu().numpy(), want["scale"], name)
    same_bits(out.latents.cpu().numpy(), ER.normalised(want["z"], True), name)
    same_bits(out.loss.cpu().numpy(), want["loss"], name)
    same_bits(out.view_loss.cpu().numpy(), vloss, name)
    same_bits(out.history.cpu().numpy(), want["loss"].astype(np.float32)[None], name)
    assert out.flags.cpu().numpy().tolist() == [0, 0] and out.view_flags.cpu().numpy().tolist() == [0, 0, 0]
    assert (want["z"] != z0).any() and (want["scale"] != scale0).all() and (want["theta"][:, :4] != theta[:, :4]).all()
    assert [len(p) for p in out.params] == [2, 1] and out.params[0][1]["latent"].data_ptr() == out.latents[0].data_ptr()


def test_staging_one_track_per_group_gives_the_bits_of_all_at_once():
    dec = gpu_decoder("asset")
    L, n = int(dec.latent_size), 200
    samples, soff, voff, z0, scale0, theta = _three_views(L, n)
    for draw, k in ((False, n), (True, 128)):
        kw = dict(iters=3, rows_per_iter=k, clamp=ONE_CLAMP, seed=11, history=True, draw=draw, weights=list(TC.FIT_WEIGHTS), **ONE_RATES)
        whole = T.align_tracks(dec, _tracks(voff, z0, scale0, theta), samples=_bound_samples(samples, soff), **kw)
        staged = T.align_tracks(dec, _tracks(voff, z0, scale0, theta), samples=_bound_samples(samples, soff), staging_bytes=1, **kw)
        for key in ("raw_latents", "latents", "scale", "theta", "loss", "view_loss", "flags", "view_flags", "history"):
            same_bits(getattr(whole, key).cpu().numpy(), getattr(staged, key).cpu().numpy(), (draw, key))
        assert not whole.flags.any() and (whole.raw_latents.cpu().numpy() != z0).any()


def test_no_host_traffic_in_twenty_iterations():
    dec = gpu_decoder("w128")
    L, n = int(dec.latent_size), 200
    samples, soff, voff, z0, scale0, theta = _three_views(L, n)
    tracks, bound = _tracks(voff, z0, scale0, theta), _bound_samples(samples, soff)
    kw = dict(rows_per_iter=64, clamp=ONE_CLAMP, seed=3, history=True, weights=list(TC.FIT_WEIGHTS))
    T.align_tracks(dec, tracks, samples=bound, iters=2, **kw)                                            # the handle and the library are loaded
    syncs, out = count_syncs(lambda: T.align_tracks(dec, tracks, samples=bound, iters=20, **kw))
    assert syncs == 0, syncs
    assert all(getattr(out, key).is_cuda for key in ("latents", "raw_latents", "scale", "theta", "loss", "view_loss", "flags", "view_flags", "history"))
    assert tuple(out.history.shape) == (20, 2) and not out.flags.any()


@pytest.mark.parametrize("name", TRAJ_NAMES)
def test_ten_step_trajectory_stays_within_the_calibrated_bound_of_the_float64_loop(name):
    """Measured values: profiles/track_notes.md."""
    from tests import _track_traj as TT
    dec = gpu_decoder(name)
    case = TC.fit_case(name, TT.TRAJECTORY_SEED[name], TT.TRAJECTORY_K)
    samples, soff, voff, z0, scale0, theta0, w, k, clamp = case
    ref = TT.run(name, ET.decoder64(PC.net(name)), np.float64, case, ET.STEPS)                            # (admitted on the CPU)
    out = T.align_tracks(dec, _tracks(voff, z0, scale0, theta0), samples=_bound_samples(samples, soff), weights=w, iters=ET.STEPS, rows_per_iter=k, clamp=clamp,
                         history=True, fit=ALL, lr=AC.FIT["lr"], lr_pose=AC.FIT["lr_pose"][0], lr_step=AC.FIT["lr_step"], lr_factor=AC.FIT["lr_factor"],
                         code_reg=AC.FIT["code_reg"])
    dz = float(np.abs(out.raw_latents.cpu().numpy().astype(np.float64) - ref["z"]).max())
    dt = float(np.abs(out.theta.cpu().numpy().astype(np.float64) - ref["theta"]).max())
    dl = float(np.abs(out.history.cpu().numpy().astype(np.float64) - ref["history"]).max())
    print("%s: device deviates %.3e (latent) %.3e (pose) from float64 after %d steps (bound %.3e); loss history %.3e"
          % (name, dz, dt, ET.STEPS, TT.TRAJECTORY_BOUND[name], dl))
    assert not out.flags.any() and not out.view_flags.any()
    assert max(dz, dt) <= TT.TRAJECTORY_BOUND[name], (dz, dt, TT.TRAJECTORY_BOUND[name])


def test_three_views_of_the_completion_fixtures_shape():
    """The case of tests/_track_traj.py (built on the CPU; the seed chosen with the float64 loop).  The device's rows are the restatement's,
    the loss falls, and the last loss lies within a factor of two of the float64 run's.  The cosine to the true latent and the whole-shape
    residual are printed beside float64's, not asserted.  profiles/track_notes.md has the measured values."""
    from tests import _complete_traj as CT
    from tests import _track_traj as TT
    dec = gpu_decoder("asset")
    r, case, ref = TT.THREE, TT.three_case(), TT.three_reference()
    assert ref["history"][-1] < ref["history"][0]
    dev = lambda a: torch.as_tensor(np.array(a, np.float32)).reshape(-1).to(DEV)
    track = {"latent": dev(case["z0"][0]), "scale": dev(case["scale0"]),
             "views": [{"yaw": dev(case["theta0"][v, 0:1]), "trans": dev(case["theta0"][v, 1:4]), "cloud": np.array(case["clouds"][v]),
                        "normals": torch.from_numpy(np.array(case["normals"][v])).to(DEV)} for v in range(3)]}
    out = T.align_tracks(dec, [track], free_rows=r["free_rows"], eta=r["eta"], s_max=r["s_max"], seed=r["seed"], iters=r["iters"], rows_per_iter=r["rows"],
                         lr=r["lr"], lr_pose=r["lr_pose"], lr_step=r["lr_step"], lr_factor=r["lr_factor"], clamp=r["clamp"], history=True)
    same_bits(np.concatenate([s.numpy() for s in out.samples]), np.array(case["rows"]), "the device's rows are the restatement's")
    h = out.history.cpu().numpy()[:, 0]
    zn = out.latents.cpu().numpy().astype(np.float64)
    cosine = float((zn[0] * case["z_true"][0]).sum())
    residual = CT.residual(out.raw_latents.cpu().numpy()[0], CT.completion_case()["full"])
    print("three views: loss %.4e -> %.4e (float64 %.4e -> %.4e); cosine %.4f (float64 %.4f); residual %.4e (float64 %.4e, start %.4e); scale %.4f (float64 %.4f)"
          % (h[0], h[-1], ref["history"][0], ref["history"][-1], cosine, ref["cosine"], residual, ref["residual"], ref["residual_start"], float(out.scale[0]),
             ref["scale"][0]))
    assert int(out.flags[0]) == 0 and not out.view_flags.any() and all(int(s.flags) == 0 for s in out.samples)
    assert h[-1] < h[0], (h[0], h[-1])
    assert 0.5 * ref["history"][-1] <= h[-1] <= 2.0 * ref["history"][-1], (h[-1], ref["history"][-1])


# ---- label_sequence --------------------------------------------------------------------------------------------------------------------------------

EGO = ((0.0, (0.0, 0.0, 0.0)), (0.03, (0.6, 0.0, 1.5)), (-0.04, (-0.5, 0.0, 3.0)))           # yaw about the camera's y axis, translation: the road stays a plane


def _ego(yaw, t):
    """cam_to_world of an ego pose: the 4x4 that takes the moved camera's frame to the first camera's"""
    M = np.eye(4)
    c, s = np.cos(yaw), np.sin(yaw)
    M[:3, :3] = [[c, 0, s], [0, 1, 0], [-s, 0, c]]
    M[:3, 3] = t
    return M


def _same_labels(got, want, what):
    assert set(got) == set(want), what
    for k in want:
        assert (list(got[k]) == list(want[k])) if k == "name" else (got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes()), (what, k)


def test_label_sequence_on_the_planted_scene_under_three_ego_poses():
    import sdflabel_amd
    from sdflabel_amd import cluster as C
    from sdflabel_amd import frame as FR
    from sdflabel_amd.pipelines import scan, sequence
    from tests import _cluster_ref as CR
    from tests import _normals_ref as NR
    sc, s = CR.planted_scene(), CR.SCENE
    K, (w, h) = NR.KITTI_K, NR.KITTI_WH
    dec, grid = gpu_decoder("asset"), sdflabel_amd.Grid3D(40, DEV)
    p_WC = np.eye(4)
    p_WC[:3, 3] = [0.1, -0.2, 0.3]
    world = np.array(sc["points"], np.float64)
    c2w = [_ego(*e) for e in EGO]
    scans = [torch.from_numpy(((world - M[:3, 3]) @ M[:3, :3]).astype(np.float32)).to(DEV) for M in c2w]          # p_cam = R^T (p_world - t)
    lat = torch.from_numpy(np.array(sc["z_true"])).to(DEV)
    # the road removal takes the roofs with the road: the third object, seen end on, keeps one side 0.24 m thick, under the scene's own width gate
    # (tests/_cluster_ref.py on the CPU: clusters of 978, 954 and 688 points; the wall, 11.7 m long, stays rejected)
    ckw = dict(eps=s["eps"], min_points=s["min_points"], max_clusters=64, n_angles=s["n_angles"], scale=s["scale"], gates=dict(s["gates"], width=(0.2, 3.5)))
    akw = dict(iters=60, rows_per_iter=512, lr_step=40, seed=3)
    jkw = dict(iters=40, rows_per_iter=512, lr_step=30, seed=3, history=True)
    run = lambda: sequence.label_sequence(dec, grid, scans, K, w, h, p_WC, lat, cam_to_world=c2w, gate=2.0, cluster_kw=ckw, align_kw=akw, joint_kw=jkw)
    run()                                                                                                # the handle and the library are loaded
    syncs, (est, st) = count_syncs(run)
    counts = [len(p) for p in st["proposals"]]
    n_all = sum(counts)
    print("label_sequence: proposals per scan %s, %d tracks, %d synchronisations; joint loss %s -> %s" %
          (counts, len(st["tracks"]), syncs, st["joint"].history[0].cpu().numpy(), st["joint"].history[-1].cpu().numpy()))
    assert syncs == len(scans) + 1 + sum((a + 15) // 16 for a in counts), syncs                          # as label_sequence's docstring states
    # exactly the planted tracks: three objects, each seen in every scan, each track one object
    assert counts == [3, 3, 3] and len(st["tracks"]) == 3 and all([i for i, _ in tr] == [0, 1, 2] for tr in st["tracks"])
    for tr in st["tracks"]:
        who = set()
        for i, a in tr:
            info = st["proposals"][i].info[a]
            centre = c2w[i][:3, :3] @ info["centre"] + c2w[i][:3, 3]
            who.add(int(np.argmin([np.linalg.norm(centre - c) for _, c in sc["truth"]])))
            assert min(np.linalg.norm(centre - c) for _, c in sc["truth"]) < 1.5       # (a rectangle around one visible side sits off the centre)
        assert len(who) == 1
    assert all(e["track"].tolist() == a.tolist() and len(e["name"]) == 3 for e, a in zip(est, st["assigned"]))
    assert not st["joint"].flags.any() and st["joint"].voff == [0, 3, 6, 9]
    # the hand-written chain of its calls, the choices made on the host
    props = [C.proposals(p, FR.remove_road(p, K, w, h), latent=lat, **ckw) for p in scans]
    clouds = [c for p in props for c in p.clouds]
    fits = A.align_many(dec, [q for p in props for q in p.params] + [q for p in props for q in p.flipped], clouds + clouds, **akw)
    loss = fits.loss.cpu().numpy()
    second = np.array([(loss[n_all + a] < loss[a]) or (np.isnan(loss[a]) and not np.isnan(loss[n_all + a])) for a in range(n_all)], bool)
    row = np.arange(n_all) + n_all * second
    theta, raw = fits.theta[torch.from_numpy(row).to(DEV)], fits.raw_latents[torch.from_numpy(row).to(DEV)]
    centres = [np.array([q["centre"] for q in p.info]) @ M[:3, :3].T + M[:3, 3] for p, M in zip(props, c2w)]
    tracks, assigned = sequence.associate(centres, 2.0)
    assert tracks == st["tracks"]
    first = np.concatenate([[0], np.cumsum(counts)])
    views = [[int(first[i]) + a for i, a in tr] for tr in tracks]
    best = [v[int(np.argmin(np.where(np.isnan(loss[row[v]]), np.inf, loss[row[v]])))] for v in views]
    joint = T.align_tracks(dec, [{"latent": raw[best[t]], "scale": theta[best[t], 4:5],
                                  "views": [{"yaw": theta[a, 0:1], "trans": theta[a, 1:4], "cloud": clouds[a]} for a in views[t]]} for t in range(len(tracks))], **jkw)
    for key in ("raw_latents", "latents", "scale", "theta", "loss", "history"):
        assert torch.equal(getattr(joint, key), getattr(st["joint"], key)), key
    for i, p in enumerate(props):
        off = torch.tensor([int(p.offsets[q["cluster"]]) for q in p.info], dtype=torch.int64, device=DEV)
        cnt = torch.tensor([q["n"] for q in p.info], dtype=torch.int32, device=DEV)
        Kd = torch.from_numpy(np.tile(np.asarray(K, np.float32).reshape(1, 9), (len(p), 1))).to(DEV)
        uv = FR.point_extents(p.gathered, off, cnt, int(cnt.max()), len(p), K=Kd)[0][:, 6:10].cpu().numpy()
        bboxes = [np.array([np.clip(r[0], 0, w), np.clip(r[2], 0, h), np.clip(r[1], 0, w), np.clip(r[3], 0, h)], np.float32) for r in uv]
        params = []
        for a in range(len(p)):
            t = int(assigned[i][a])
            j = tracks[t].index((i, a))
            params.append(joint.params[t][j])
        want = FR.frame_dict(FR.labels_many(dec, grid, params, p_WC, bboxes))
        _same_labels({k: v for k, v in est[i].items() if k != "track"}, want, "scan %d" % i)
    # one scan, no joint iterations: label_scan in every bit
    one, st1 = sequence.label_sequence(dec, grid, scans[:1], K, w, h, p_WC, lat, cluster_kw=ckw, align_kw=akw, joint_kw={"iters": 0})
    want, _ = scan.label_scan(dec, grid, scans[0], K, w, h, p_WC, lat, cluster_kw=ckw, align_kw=akw)
    assert len(one) == 1 and one[0]["track"].tolist() == [0, 1, 2]
    _same_labels({k: v for k, v in one[0].items() if k != "track"}, want, "one scan")
