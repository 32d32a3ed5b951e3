"""The trajectory cases and the end-to-end case of the joint fit's tests, built on the CPU.

Trajectories: tests/_track_cases.fit_case (three views over two tracks) for ten steps, in float64 and in the float32 emulation, as
tests/_align_cases.cpu_runs handles the one-view fit; TRAJECTORY_BOUND is 4 x the worst deviation of the emulation from the float64 loop.

THREE VIEWS: the lattice mesh of tests/_complete_traj.completion_case() posed at three yaws about 2 pi / 3 apart, each view's cloud its
camera-facing vertices, the camera-frame observation rows from the restatement, the float64 joint run (tests/_track_ref.loop: one latent
and one scale over the three views, yaw and trans per view) from the antipodal latent and a start off in every pose parameter, and the
three float64 one-view runs (tests/_align_ref.loop, the same parameters free) from the same start.  About 3 x 300 rows x 150 iterations:
the float64 decoder costs about 0.1 ms a row.  THREE['seed'] is the first of the seeds 0, 1, ... whose float64 joint run lowers the loss
(profiles/track_notes.md lists what was tried).  tests/test_track_cpu.py checks the reference run; tests/test_gpu_track.py compares the
device with it.
"""
import functools

import numpy as np

from tests import _align_cases as AC
from tests import _align_ref as AR
from tests import _complete_traj as CT
from tests import _encode_traj as ET
from tests import _track_cases as TC
from tests import _track_ref as TR

# 4 x the worst deviation of the float32 CPU emulation from the float64 loop over the ten steps, in max(|z - z'|, |theta - theta'|)
# (profiles/track_notes.md has the measured values; tests/test_track_cpu.py re-measures them).  The seeds are the first of 1, 2, ... at which
# no row of the float64 run comes within 100 fwd_tol of a kink of the loss or within 100 roundings of a face of the cube -- three views of
# 96 rows over ten steps are half as many rows again as the one-view fit's cases hold, and fewer seeds pass (w128: seed 1 was refused;
# lat8: seeds 1 .. 13 were).
NAMES = ("w128", "lat8")
TRAJECTORY_BOUND = {"w128": 1.81e-6, "lat8": 1.66e-6}
TRAJECTORY_SEED = {"w128": 2, "lat8": 14}
TRAJECTORY_K = ET.K


def run(name, decoder, ft, case, iters, watch_margin=False):
    from tests import _prior_train_cases as PC
    samples, soff, voff, z0, scale0, theta0, w, k, clamp = case
    net = PC.net(name)
    margins, faces, trace = [], [], []

    def watch(it, inputs, pred, lo, hi, J, pose):
        if watch_margin:
            cam = np.concatenate([np.asarray(samples)[int(soff[b]):int(soff[b]) + k, :3] for b in range(len(pose))])       # draw off: the first k rows
            a, f = AC.kink_margin(net, inputs, pred, lo, hi, pose, cam, k, clamp)
            margins.append(a), faces.append(f)

    out = TR.loop(decoder, samples, soff, voff, z0, scale0, theta0, iters, k, False, weights=w, share=True, unit=True, ft=ft, watch=watch, trace=trace,
                  clamp=clamp, **AC.FIT)
    out["trace"] = trace
    if watch_margin:
        out["margin"], out["face"] = np.array(margins), np.array(faces)
    return out


def cpu_runs(name, seed=None, k=None):
    from tests import _prior_train_cases as PC
    net = PC.net(name)
    case = TC.fit_case(name, TRAJECTORY_SEED[name] if seed is None else seed, TRAJECTORY_K if k is None else k)
    ref = run(name, ET.decoder64(net), np.float64, case, ET.STEPS, watch_margin=True)
    emu = run(name, ET.decoder32(net), np.float32, case, ET.STEPS)
    return ref, emu


# ---- three views ---------------------------------------------------------------------------------------------------------------------------------

C = CT.COMPLETION
THREE = dict(yaws=(C["yaw"], C["yaw"] + 2.1, C["yaw"] + 4.2), trans=C["trans"], scale=C["scale"], offset=(0.12, 0.03, -0.02, -0.04, 0.1), free_rows=4, eta=0.02,
             s_max=1.0, seed=0, iters=150, rows=300, lr=2e-2, lr_pose=1e-2, lr_step=100, lr_factor=0.1, clamp=0.2)


@functools.lru_cache(maxsize=None)
def three_case(seed=None):
    """dict: clouds (three float32 [n_v][3]), normals (three float64 [n_v][3]), rows float32 [7 sum n_v][5] and soff (the views' rows, camera
    frame and metric), z_true float32 [1][3], z0 (the antipodal latent), theta_true and theta0 float32 [3][5], scale0 float32 [1]"""
    r = THREE
    case = CT.completion_case()
    v = case["vertices"].astype(np.float64)
    _, g = CT._values(case["z_true"][0], case["vertices"])
    n = g / np.linalg.norm(g, axis=1, keepdims=True)
    t, sc = np.asarray(r["trans"], np.float64), float(r["scale"])
    clouds, normals = [], []
    for yaw in r["yaws"]:
        cs, sn = float(np.cos(np.float32(yaw))), float(np.sin(np.float32(yaw)))

        def rot(x):                                                      # rot_yaw diag(1, -1, 1) x, as _complete_traj poses its shape
            xs = x * np.array([1.0, -1.0, 1.0])
            return np.stack([cs * xs[:, 0] + sn * xs[:, 2], xs[:, 1], -sn * xs[:, 0] + cs * xs[:, 2]], 1)

        cam, ncam = sc * (rot(v) + t), rot(n)
        facing = (ncam * cam).sum(1) < 0
        clouds.append(cam[facing].astype(np.float32)), normals.append(ncam[facing])
    ptoff = np.concatenate([[0], np.cumsum([len(c) for c in clouds])]).astype(np.int64)
    rows, flags = AR.sample_rows(np.concatenate(clouds), np.concatenate(normals), ptoff, np.zeros(3, np.float32), r["free_rows"], r["eta"], r["s_max"],
                                 r["seed"] if seed is None else seed)
    assert not flags.any() and np.isfinite(rows[:, 3]).all()
    true = np.array([[yaw, *r["trans"], r["scale"]] for yaw in r["yaws"]], np.float32)
    start = (true + np.asarray(r["offset"], np.float32)).astype(np.float32)
    out = {"rows": rows, "soff": ptoff * (3 + r["free_rows"]), "z_true": case["z_true"], "z0": -case["z_true"], "theta_true": true, "theta0": start,
           "scale0": start[:1, 4].copy()}
    for a in list(out.values()) + clouds + normals:
        a.setflags(write=False)
    out.update(clouds=tuple(clouds), normals=tuple(normals))
    return out


def _kw(r):
    return dict(lr=r["lr"], lr_pose=(r["lr_pose"],) * 5, lr_step=r["lr_step"], lr_factor=r["lr_factor"], clamp=r["clamp"], unit=True, ft=np.float64)


@functools.lru_cache(maxsize=None)
def three_reference(seed=None):
    """the float64 joint run: dict with history [iters] (the track's loss), z (raw), zn, scale, theta, flags, cosine (to the true latent) and
    residual (the whole-shape residual, _complete_traj.residual) at the start and at the end"""
    r = THREE
    seed = r["seed"] if seed is None else seed
    case = three_case(seed)
    full = CT.completion_case()["full"]
    run = TR.loop(CT._decoder(), case["rows"], case["soff"], np.array([0, 3], np.int64), case["z0"].astype(np.float64), case["scale0"].astype(np.float64),
                  case["theta0"].astype(np.float64), r["iters"], r["rows"], True, seed=seed, share=True, **_kw(r))
    return {"history": run["history"][:, 0], "z": run["z"], "zn": run["zn"], "scale": run["scale"], "theta": run["theta"], "tflags": run["tflags"],
            "vflags": run["vflags"], "cosine": float((run["zn"][0] * case["z_true"][0]).sum()), "residual_start": CT.residual(case["z0"], full),
            "residual": CT.residual(run["z"], full)}


@functools.lru_cache(maxsize=None)
def one_view_reference(view, seed=None):
    """the float64 one-view run of view `view` from the same start, the same parameters free (tests/_align_ref.loop): history, zn, theta,
    cosine and residual"""
    r = THREE
    seed = r["seed"] if seed is None else seed
    case = three_case(seed)
    full = CT.completion_case()["full"]
    a, e = int(case["soff"][view]), int(case["soff"][view + 1])
    run = AR.loop(CT._decoder(), case["rows"][a:e], np.array([0, e - a], np.int64), case["z0"].astype(np.float64), case["theta0"][view:view + 1].astype(np.float64),
                  r["iters"], r["rows"], True, seed=seed, **_kw(r))
    return {"history": run["history"][:, 0], "zn": run["zn"], "theta": run["theta"], "flags": run["flags"],
            "cosine": float((run["zn"][0] * case["z_true"][0]).sum()), "residual": CT.residual(run["z"], full)}
