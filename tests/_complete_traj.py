"""The end-to-end completion case of the shape-completion tests, built on the CPU: the asset decoder's shape at a known latent meshed at
R = 24 by the numpy restatement of the mesher (tests/_mesh_ref.py, on the float64 decoder's lattice values, polished by one Newton step as
mesh.meshes_many polishes), posed in front of the camera, its camera-facing vertices as the cloud, and the float64 reference run of the
completion from the antipodal latent (tests/_complete_ref.loop).  tests/test_complete_cpu.py checks the reference run and
tests/test_gpu_complete.py compares the device with it, as the encoder's recovery case is handled (tests/_encode_traj.RECOVERY).

COMPLETION['seed'] was chosen on the CPU: the first of the seeds 0, 1, ... whose float64 run lowers the loss and ends with a smaller
residual on the whole shape's samples than it starts with (profiles/complete_notes.md has every seed tried).
"""
import functools

import numpy as np

from tests import _complete_ref as CR
from tests import _encode_traj as ET
from tests import _mesh_ref as MR
from tests import _prior_train_cases as PC

COMPLETION = dict(R=24, z_true=(0.3, -0.5, 0.8), yaw=0.6, trans=(0.2, -0.1, 3.0), scale=1.8, free_rows=4, eta=0.01, s_max=0.5, seed=0,
                  iters=120, rows=2000, lr=2e-2, lr_step=80, lr_factor=0.1, clamp=0.1, n_full=6000)


def _decoder():
    return ET.decoder64(PC.net("asset"))


def _values(z, pts):
    """(sdf float64 [n], d sdf / d xyz float64 [n][3]) of the float64 decoder at unit latent z"""
    x = np.concatenate([np.repeat(np.asarray(z, np.float64)[None], len(pts), 0), np.asarray(pts, np.float64)], 1)
    out, J = _decoder()(x)
    return np.asarray(out, np.float64).reshape(-1), np.asarray(J, np.float64)[:, len(z):len(z) + 3]


@functools.lru_cache(maxsize=None)
def completion_case():
    """dict: z_true [1][3] float32 (unit), vertices float32 [V][3] and faces int32 [T][3] of the polished lattice-frame mesh, cloud float32
    [n][3] and normals float64 [n][3] in the camera frame (the vertices whose outward normal faces the camera centre), pose float32 [1][6],
    rows float32 [n (3 + F)][5] (the restatement's view rows of that cloud), full float32 [n_full][4]: samples of the WHOLE shape -- half
    uniform in the cube, half vertices moved by N(0, 0.05^2) -- with the float64 decoder's own value at z_true as their signed distance."""
    c = COMPLETION
    z = np.asarray(c["z_true"], np.float64)
    z_true = (z / np.linalg.norm(z)).astype(np.float32)
    R = c["R"]
    sdf, _ = _values(z_true, MR.lattice_points(R))
    v, f, _ = MR.extract(sdf.astype(np.float32).reshape(R, R, R))
    assert MR.is_closed(f) and MR.signed_volume(v.astype(np.float64), f) > 0
    val, g = _values(z_true, v)
    n = g / np.linalg.norm(g, axis=1, keepdims=True)
    v = (v.astype(np.float64) - val[:, None] * n).astype(np.float32)                 # the polish: one Newton step along the decoder's normal
    _, g = _values(z_true, v)
    n = g / np.linalg.norm(g, axis=1, keepdims=True)                                 # outward: the gradient of a signed distance
    yaw = np.float32(c["yaw"])
    cs, sn, t, sc = float(np.cos(yaw)), float(np.sin(yaw)), np.asarray(c["trans"], np.float64), float(c["scale"])

    def rot(x):                                                                      # rot_yaw diag(1, -1, 1) x
        xs = x * np.array([1.0, -1.0, 1.0])
        return np.stack([cs * xs[:, 0] + sn * xs[:, 2], xs[:, 1], -sn * xs[:, 0] + cs * xs[:, 2]], 1)

    cam, ncam = sc * (rot(v.astype(np.float64)) + t), rot(n)
    facing = (ncam * cam).sum(1) < 0                                                  # the sensor is the camera centre
    assert 0.25 < facing.mean() < 0.75
    cloud, normals = cam[facing].astype(np.float32), ncam[facing]
    pose = np.array([[np.float32(cs), np.float32(sn), t[0], t[1], t[2], sc]], np.float32)
    out = {"z_true": z_true[None], "vertices": v, "faces": f, "cloud": cloud, "normals": normals, "pose": pose}
    for F in (c["free_rows"], 0):
        out["rows%d" % F] = CR.view_rows(cloud, normals, np.array([0, len(cloud)], np.int64), pose, np.zeros(3, np.float32), F, c["eta"],
                                         c["s_max"], c["seed"])[0]
    rng = np.random.default_rng(5)
    half = c["n_full"] // 2
    pts = np.concatenate([rng.uniform(-1, 1, (half, 3)), v[rng.integers(0, len(v), c["n_full"] - half)] + rng.normal(0, 0.05, (c["n_full"] - half, 3))])
    pts = np.clip(pts, -1, 1).astype(np.float32)
    out["full"] = np.concatenate([pts, _values(z_true, pts)[0].astype(np.float32)[:, None]], 1)
    for a in out.values():
        a.setflags(write=False)
    return out


def residual(z, full, clamp=0.1):
    """sdf_samples.prior_residuals' first value in float64: mean |clamp(decoder(z / |z|, x)) - clamp(sdf)| over the whole shape's samples"""
    z = np.asarray(z, np.float64).reshape(-1)
    val, _ = _values(z / np.linalg.norm(z), full[:, :3])
    return float(np.abs(np.clip(val, -clamp, clamp) - np.clip(full[:, 3].astype(np.float64), -clamp, clamp)).mean())


@functools.lru_cache(maxsize=None)
def completion_reference(free_rows=None, seed=None):
    """the float64 run: dict with history [iters] (the loss before each step), z (raw), residual_start, residual_end"""
    c = COMPLETION
    case = completion_case()
    F = c["free_rows"] if free_rows is None else free_rows
    seed = c["seed"] if seed is None else seed
    rows = case["rows%d" % F] if seed == c["seed"] else CR.view_rows(case["cloud"], case["normals"], np.array([0, len(case["cloud"])], np.int64),
                                                                     case["pose"], np.zeros(3, np.float32), F, c["eta"], c["s_max"], seed)[0]
    z0 = -case["z_true"].astype(np.float64)
    run = CR.loop(_decoder(), rows, np.array([0, len(rows)], np.int64), z0, c["iters"], c["rows"], True, seed=seed, lr=c["lr"], lr_step=c["lr_step"],
                  lr_factor=c["lr_factor"], clamp=c["clamp"], code_reg=1e-4, unit=True, ft=np.float64)
    return {"history": run["history"][:, 0], "z": run["z"], "flags": run["flags"], "residual_start": residual(z0, case["full"]),
            "residual_end": residual(run["z"], case["full"]), "cosine": float((run["zn"][0] * case["z_true"][0]).sum())}
