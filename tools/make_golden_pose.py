"""G15: golden vectors of the reference's RANSAC pose initialisation (utils/pose.py:85-233, PoseEstimator.init_pose_3d).

Runs the reference's own code (tools/_ref_import.py: read-only, cv2 stubbed -- the kabsch / procrustes path never calls it) and records,
by wrapping np.random.choice and utils.pose.KDTree (nothing of the reference is restated):
  - the seed and every draw;
  - per hypothesis: colour gate, the colour KDTree's answers for its 4 scene points, inlier count (-1: not scored), the number of scene
    points within SLACK of either threshold;
  - the best hypothesis, the scene rows of its inliers with the colour KDTree's answers for them (the final query), and the final pose.
Model: surface points + NOCS of the committed synthetic decoder on the reference's Grid3D(40) (float32, and the float16 grid).
Scene: model points under a known yaw / translation, with position noise, 50 % outliers and NOCS noise.
A seed whose best count does not lead every other count by more than the recorded slack is refused and the next seed tried.  In scenes with
50 % outliers many hypotheses reach the full inlier count, so after six refusals the case is kept and marked decisive = 0; the tests
compare the best index and the final pose of every found case all the same (tests/test_gpu_pose.py), which holds as long as the device's
counts equal the reference's at the top.

usage: python tools/make_golden_pose.py      -> tests/golden/g15_pose_init.npz
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _ref_import  # noqa: E402

_ref_import.setup()
sys.modules["pyquaternion"].Quaternion = object

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import grid as ref_grid  # noqa: E402  (reference sdfrenderer/grid.py)
import deepsdf.workspace as ref_ws  # noqa: E402
import utils.pose as ref_pose  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "..", "tests", "golden", "g15_pose_init.npz")
ASSET = os.path.join(HERE, "..", "sdflabel_amd", "assets", "deepsdf_synth.pt")
SLACK = 1e-4
THR = 0.15
torch.set_num_threads(8)


def surface(precision, latent=(0.3, -0.5, 0.8)):
    dec, _ = ref_ws.setup_dsdf(ASSET, precision=precision)
    grid = ref_grid.Grid3D(40, "cpu", precision)
    lat = F.normalize(torch.tensor(latent, dtype=torch.float32), p=2, dim=0).to(precision)
    inputs = torch.cat([lat.expand(grid.points.size(0), -1), grid.points], 1)
    sdf, _ = dec(inputs)
    pts, nocs, _ = grid.get_surface_points(sdf)
    return pts.detach().numpy(), nocs.detach().numpy()


def yaw_matrix(yaw):
    c, s = np.cos(yaw), np.sin(yaw)
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])


def make_scene(model, mcls, n, rng, yaw, tra, scale, outlier=0.5, noise=0.005, nocs_noise=0.01):
    """scene = R (scale * model) + t (+ noise) for the inliers; outliers anywhere in the inliers' box with random colours"""
    n_in = n - int(round(outlier * n))
    sel = rng.choice(model.shape[0], n_in, replace=n_in > model.shape[0])
    p = (yaw_matrix(yaw) @ (scale * model[sel].astype(np.float64)).T).T + np.asarray(tra) + rng.normal(0, noise, (n_in, 3))
    c = mcls[sel].astype(np.float64) + rng.normal(0, nocs_noise, (n_in, 3))
    lo, hi = p.min(0) - 0.5, p.max(0) + 0.5
    po = rng.uniform(lo, hi, (n - n_in, 3))
    co = rng.uniform(0, 1, (n - n_in, 3))
    perm = rng.permutation(n)
    return np.concatenate([p, po])[perm].astype(np.float32), np.concatenate([c, co])[perm].astype(np.float32)


class Recorder:
    """wraps np.random.choice and utils.pose.KDTree for one init_pose_3d call"""

    def __init__(self):
        self.draws, self.gate, self.gate_cnn, self.counts, self.slack, self.final_cnn = [], [], [], [], [], None
        self.best_count, self.best_rows = 0, np.zeros(0, np.int64)
        self.trees = []

    def install(self):
        rec = self
        orig_choice = np.random.choice
        Base = ref_pose.KDTree

        class KD(Base):
            def __init__(self, data, *a, **k):
                super().__init__(data, *a, **k)
                self._data = np.asarray(data)
                self._role = "cls" if not rec.trees else "pts"
                rec.trees.append(self)

            def query(self, X, *a, **k):
                d, i = super().query(X, *a, **k)
                if self._role == "cls":
                    if len(rec.draws) > len(rec.gate):          # the colour gate of the current hypothesis
                        rec.gate.append(int(not (d > THR).any()))
                        rec.gate_cnn.append(i.ravel().astype(np.int32))
                        rec.counts.append(-1)
                        rec.slack.append(0)
                    else:                                        # the final correspondences
                        rec.final_cnn = i.ravel().copy()
                return d, i

        def choice(*a, **k):
            r = orig_choice(*a, **k)
            rec.draws.append(np.asarray(r, dtype=np.int32))
            return r

        self._restore = (orig_choice, Base)
        np.random.choice = choice
        ref_pose.KDTree = KD

    def uninstall(self):
        np.random.choice, ref_pose.KDTree = self._restore


def run_case(model, mcls, scene, scls, type, scale_model, seed):
    rec = Recorder()
    rec.install()
    # the per-hypothesis inlier count is derived from the point tree's recorded query outputs with the reference's own expression
    # (utils/pose.py:180-185)
    try:
        np.random.seed(seed)
        m = model.copy()
        KD = ref_pose.KDTree
        orig_q = KD.query

        def q(self, X, *a, **k):
            d, i = orig_q(self, X, *a, **k)
            if self._role == "pts":
                t = len(rec.draws) - 1
                dd, ii = d.ravel(), i.ravel()
                dc = np.linalg.norm(scls - mcls[ii], axis=1)
                inl = np.where((dd < THR) & (dc < THR))[0]
                rec.counts[t] = int(len(inl))
                if len(inl) > rec.best_count:                  # the rows the final colour query is asked for (utils/pose.py:191-198)
                    rec.best_count, rec.best_rows = len(inl), inl
                rec.slack[t] = int(((np.abs(dd - THR) < SLACK) | (np.abs(dc - THR) < SLACK)).sum())
            return d, i

        KD.query = q
        pose = ref_pose.PoseEstimator.init_pose_3d(m, mcls, scene, scls, type=type, scale_model=scale_model)
    except TypeError:
        pose = "crash"
    finally:
        rec.uninstall()
    T = len(rec.draws)
    return rec, pose, T


def check_lead(counts, slack):
    counts, slack = np.asarray(counts), np.asarray(slack)
    if counts.max() <= 0:
        return True
    b = int(np.argmax(counts))
    for t in range(len(counts)):
        if t == b or counts[t] < 0:
            continue
        s = slack[b] + slack[t]
        if abs(int(counts[t]) - int(counts[b])) <= s and not (counts[t] == counts[b] and s == 0):
            return False
    return True


def recovered(pose, yaw, tra):
    if not isinstance(pose, dict):
        return False
    R = np.asarray(pose["rot"], np.float64)
    dR = R @ yaw_matrix(yaw).T
    ang = np.degrees(np.arccos(np.clip((np.trace(dR) - 1) / 2, -1, 1)))
    return ang < 1.0 and np.linalg.norm(np.asarray(pose["tra"], np.float64) - tra) < 0.05


def main():
    m32, c32 = surface(torch.float32)
    m16, c16 = surface(torch.float16)
    print("model points: f32 %d, f16 %d" % (len(m32), len(m16)))
    cases = [  # name, dtype, type, N, yaw, tra, special
        ("k32_1000", 32, "kabsch", 1000, 0.6, (0.3, -0.2, 6.0), None),
        ("k32_3000", 32, "kabsch", 3000, -1.1, (-0.5, 0.1, 9.0), None),
        ("k32_300", 32, "kabsch", 300, 2.0, (1.0, 0.4, 12.0), None),
        ("k16_1000", 16, "kabsch", 1000, 0.9, (0.2, 0.0, 7.0), None),
        ("k16_300", 16, "kabsch", 300, -0.4, (-0.8, 0.3, 5.0), None),
        ("p32_1000", 32, "procrustes", 1000, 0.3, (0.1, -0.1, 8.0), None),
        ("p32_300", 32, "procrustes", 300, 1.4, (0.6, 0.2, 10.0), None),
        ("k32_5", 32, "kabsch", 5, 0.6, (0.3, -0.2, 6.0), None),
        ("none_n4", 32, "kabsch", 4, 0.6, (0.3, -0.2, 6.0), None),
        ("none_gate", 32, "kabsch", 200, 0.6, (0.3, -0.2, 6.0), "gate"),
        ("none_inliers", 32, "kabsch", 60, 0.6, (0.3, -0.2, 6.0), "inliers"),
    ]
    out = {"slack": np.float64(SLACK), "threshold": np.float64(THR), "names": np.array([c[0] for c in cases]),
           "model32": m32, "model32_cls": c32, "model16": m16, "model16_cls": c16}
    n_rec = 0
    for ci, (name, dt, type, n, yaw, tra, special) in enumerate(cases):
        model, mcls = (m32, c32) if dt == 32 else (m16, c16)
        scale_model = 2.0
        decisive = False
        for attempt in range(6):
            rng = np.random.default_rng(1000 * ci + attempt)
            scene, scls = make_scene(model, mcls, n, rng, yaw, tra, scale_model)
            if special == "gate":
                scls = (scls + 1.0).astype(np.float32)
            elif special == "inliers":
                scene = rng.uniform(-20, 20, (n, 3)).astype(np.float32)
            seed = 1 + attempt
            rec, pose, T = run_case(model, mcls, scene, scls, type, scale_model, seed)
            decisive = not rec.counts or check_lead(rec.counts, rec.slack)
            if decisive:
                break
            print(name, "seed", seed, "refused: best count within the slack of another")
        # no decisive seed: the fixture is kept with decisive = 0 and its best index / final pose are not compared (counts still are)
        counts = np.asarray(rec.counts, np.int32) if rec.counts else np.zeros(0, np.int32)
        best = int(np.argmax(counts)) if len(counts) and counts.max() > 0 else -1
        ok = isinstance(pose, dict)
        rc = recovered(pose, yaw, tra)
        n_rec += int(rc) if special is None and n >= 300 else 0
        print("%-13s N=%4d %-10s f%d seed %d: T=%d gate %d scored %d best %d count %d found %s recovered %s" % (
            name, n, type, dt, seed, T, int(np.sum(rec.gate)), int((counts >= 0).sum()), best, counts.max() if len(counts) else -1, ok, rc))
        p = "c%d_" % ci
        out.update({p + "type": np.array(type), p + "dtype": np.int32(dt), p + "seed": np.int64(seed), p + "scene": scene, p + "scene_cls": scls,
                    p + "yaw": np.float64(yaw), p + "tra_gt": np.asarray(tra, np.float64), p + "scale_model": np.float64(scale_model),
                    p + "draws": np.asarray(rec.draws, np.int32).reshape(-1, 4), p + "gate": np.asarray(rec.gate, np.int32),
                    p + "counts": counts, p + "near": np.asarray(rec.slack, np.int32), p + "best": np.int32(best),
                    p + "found": np.int32(ok), p + "recovered": np.int32(rc), p + "decisive": np.int32(decisive),
                    p + "gate_cnn": np.asarray(rec.gate_cnn, np.int32).reshape(-1, 4),
                    p + "final_rows": np.asarray(rec.best_rows if ok else np.zeros(0), np.int32),
                    p + "final_cnn": rec.final_cnn if rec.final_cnn is not None else np.zeros(0, np.int64)})
        if ok:
            out.update({p + "rot": np.asarray(pose["rot"], np.float32), p + "tra": np.asarray(pose["tra"], np.float32),
                        p + "scale": np.float64(pose["scale"])})
    out["n_cases"] = np.int32(len(cases))
    out["ref_recovered"] = np.int32(n_rec)
    out["ref_recovery_cases"] = np.int32(sum(1 for c in cases if c[6] is None and c[3] >= 300))
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, "%.1f KB" % (os.path.getsize(OUT) / 1024))


if __name__ == "__main__":
    main()
