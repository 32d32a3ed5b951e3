"""The end-to-end recovery case of the pose-and-shape fit's tests, built on the CPU: the cloud of the completion fixture
(tests/_complete_traj.completion_case(): the asset decoder's shape, 942 camera-facing points, true pose yaw 0.6, trans (0.2, -0.1, 3.0),
scale 1.8), its camera-frame observation rows from the restatement, and the float64 reference run (tests/_align_ref.loop) that fits yaw and
trans under the true latent from a start that is off in all four.  tests/test_align_cpu.py checks the reference run and
tests/test_gpu_align.py compares the device with it.

Rows are drawn (500 of the 6594 per iteration: the float64 decoder costs about 0.1 ms a row, and 200 iterations should stay under 20 s).
RECOVERY['seed'] was chosen on the CPU: the first of the seeds 0, 1, ... whose float64 run lowers the loss and ends with every fitted
parameter's error below a quarter of its starting error (profiles/align_notes.md lists the seeds tried).
"""
import functools

import numpy as np

from tests import _align_ref as AR
from tests import _complete_traj as CT

C = CT.COMPLETION
RECOVERY = dict(yaw=C["yaw"], trans=C["trans"], scale=C["scale"], offset=(0.12, 0.03, -0.02, -0.04), free_rows=4, eta=0.02, s_max=1.0, seed=0,
                iters=200, rows=500, lr_pose=1e-2, lr_step=100, lr_factor=0.1, clamp=0.2)


@functools.lru_cache(maxsize=None)
def recovery_case(seed=None):
    """dict: cloud float32 [n][3], normals float64 [n][3], rows float32 [7 n][5] (camera frame, metric), z_true float32 [1][3],
    theta_true and theta0 float32 [1][5]"""
    r = RECOVERY
    case = CT.completion_case()
    cloud, normals = case["cloud"], case["normals"]
    rows, flags = AR.sample_rows(cloud, normals, np.array([0, len(cloud)], np.int64), np.zeros(3, np.float32), r["free_rows"], r["eta"], r["s_max"],
                                 r["seed"] if seed is None else seed)
    assert not flags.any() and np.isfinite(rows[:, 3]).all()
    true = np.array([[r["yaw"], *r["trans"], r["scale"]]], np.float32)
    start = true.copy()
    start[0, :4] += np.asarray(r["offset"], np.float32)
    out = {"cloud": cloud, "normals": normals, "rows": rows, "z_true": case["z_true"], "theta_true": true, "theta0": start}
    for a in out.values():
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def recovery_reference(seed=None, rows_per_iter=None):
    """the float64 run: dict with history [iters], theta [1][5], flags, error_start and error_end [4] (|yaw, tx, ty, tz - truth|)"""
    r = RECOVERY
    seed = r["seed"] if seed is None else seed
    case = recovery_case(seed)
    rows = case["rows"]
    k = r["rows"] if rows_per_iter is None else rows_per_iter
    run = AR.loop(CT._decoder(), rows, np.array([0, len(rows)], np.int64), case["z_true"].astype(np.float64), case["theta0"].astype(np.float64),
                  r["iters"], k, k < len(rows), seed=seed, lr=0.0, lr_pose=(r["lr_pose"],) * 4 + (0.0,), lr_step=r["lr_step"], lr_factor=r["lr_factor"],
                  clamp=r["clamp"], unit=True, ft=np.float64)
    true = case["theta_true"].astype(np.float64)
    return {"history": run["history"][:, 0], "theta": run["theta"], "flags": run["flags"],
            "error_start": np.abs(case["theta0"].astype(np.float64) - true)[0, :4], "error_end": np.abs(run["theta"] - true)[0, :4]}
