"""RANSAC pose initialisation on the GPU against G15 (the reference's own init_pose_3d, recorded by tools/make_golden_pose.py)."""
import os

import numpy as np
import pytest
import torch

from sdflabel_amd import pose as P
from sdflabel_amd.pipelines.pose import PoseEstimator

pytestmark = pytest.mark.gpu
G15 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g15_pose_init.npz")
DEV = "cuda:0"


@pytest.fixture(scope="module")
def g15():
    return np.load(G15)


def _case(g, ci):
    c = "c%d_" % ci
    dt = int(g[c + "dtype"])
    return dict(name=str(g["names"][ci]), type=str(g[c + "type"]), model=g["model%d" % dt], mcls=g["model%d_cls" % dt],
                scene=g[c + "scene"], scls=g[c + "scene_cls"], draws=g[c + "draws"], gate=g[c + "gate"], counts=g[c + "counts"],
                near=g[c + "near"], best=int(g[c + "best"]), found=int(g[c + "found"]), final_rows=g[c + "final_rows"],
                final_cnn=g[c + "final_cnn"], scale_model=float(g[c + "scale_model"]), c=c)


def _run(k, **kw):
    idx = [k["draws"]] if len(k["draws"]) else None
    out = P.ransac_pose([torch.from_numpy(k["model"]).to(DEV)], [torch.from_numpy(k["mcls"]).to(DEV)], [k["scene"]], [k["scls"]],
                        type=k["type"], scale_model=k["scale_model"], idx=idx, sampler="numpy" if idx else "device", **kw)
    return {key: (v.cpu().numpy() if torch.is_tensor(v) else v) for key, v in out.items()}


@pytest.mark.parametrize("name", ["k32_1000", "k32_3000", "k32_300", "k16_1000", "k16_300", "p32_1000", "p32_300"])
def test_g15_parity(g15, name):
    ci = list(g15["names"]).index(name)
    k = _case(g15, ci)
    o = _run(k)
    n = k["scene"].shape[0]
    gate = (o["gate"][0] & 1).astype(np.int32)
    assert np.array_equal(gate, k["gate"]), "colour gate flags differ"
    scored = (o["gate"][0] & 2) != 0
    assert np.array_equal(scored, k["counts"] >= 0)
    rank_def = (o["gate"][0] & 4) != 0
    chk = scored & ~rank_def
    diff = np.abs(o["counts"][0][chk] - k["counts"][chk])
    assert (diff == 0).mean() >= 0.99, (name, (diff != 0).sum(), chk.sum())
    assert np.all(diff <= k["near"][chk]), "a count differs by more than the near-threshold slack"
    # every found case: the reference's best hypothesis, its inlier count and the final pose (decisive or not: the device's counts must
    # then agree at the top, which the per-hypothesis check above does not require by itself)
    assert int(o["found"][0]) == k["found"] == 1
    assert int(o["best"][0]) == k["best"]
    assert int(o["n_inliers"][0]) == len(k["final_rows"]) == k["counts"][k["best"]]
    rot, tra = g15[k["c"] + "rot"], g15[k["c"] + "tra"]
    assert np.abs(o["rot"][0] - rot).max() < 1e-5
    assert np.abs(o["tra"][0] - tra).max() < 1e-4
    sc = float(g15[k["c"] + "scale"])
    if k["type"] == "kabsch":
        assert float(o["scale"][0]) == np.float32(sc)
    else:
        assert abs(float(o["scale"][0]) - sc) <= 1e-5 * abs(sc)
    assert o["cnn_idx"].shape[1] == n and (o["cnn_idx"][0] >= 0).all() and (o["cnn_idx"][0] < k["model"].shape[0]).all()


def test_g15_colour_nn_table_equals_kdtree_answers(g15):
    """row by row: the table's entry for every scene point the reference queried (the 4 sampled points of every hypothesis and the best
    hypothesis' inliers) equals the reference KDTree's answer"""
    checked = 0
    for ci in range(int(g15["n_cases"])):
        k = _case(g15, ci)
        c = k["c"]
        if not len(k["draws"]):
            continue
        cnn = _run(k)["cnn_idx"][0]
        gate_cnn = g15[c + "gate_cnn"]
        assert gate_cnn.shape == k["draws"].shape
        assert np.array_equal(cnn[k["draws"]], gate_cnn), k["name"]
        rows = g15[c + "final_rows"]
        assert np.array_equal(cnn[rows], k["final_cnn"][:len(rows)]), k["name"]
        checked += gate_cnn.size + len(rows)
    assert checked > 20000


@pytest.mark.parametrize("name", ["k32_5", "none_n4", "none_gate", "none_inliers"])
def test_g15_none_cases(g15, name):
    k = _case(g15, list(g15["names"]).index(name))
    assert k["found"] == 0
    o = _run(k)
    assert int(o["found"][0]) == 0
    np.random.seed(int(g15[k["c"] + "seed"]))
    assert PoseEstimator.init_pose_3d(torch.from_numpy(k["model"]).to(DEV), k["mcls"], k["scene"], k["scls"], type=k["type"],
                                      scale_model=k["scale_model"]) is None


def test_dropin_estimate_matches_reference_dict(g15):
    k = _case(g15, 0)
    np.random.seed(int(g15[k["c"] + "seed"]))
    pe = PoseEstimator(type="kabsch", scale=k["scale_model"])
    r = pe.estimate(torch.from_numpy(k["model"]).to(DEV), torch.from_numpy(k["mcls"]).to(DEV), torch.from_numpy(k["scene"]).to(DEV),
                    torch.from_numpy(k["scls"]).to(DEV), None, None)
    assert set(r) == {"scale", "rot", "tra"}
    assert r["rot"].dtype == np.float32 and r["rot"].shape == (3, 3) and r["tra"].dtype == np.float32 and r["tra"].shape == (3,)
    assert r["scale"] == k["scale_model"]
    assert np.abs(r["rot"] - g15[k["c"] + "rot"]).max() < 1e-5 and np.abs(r["tra"] - g15[k["c"] + "tra"]).max() < 1e-4


def _frame(g15, n_crops=16):
    m, mc = g15["model32"], g15["model32_cls"]
    rng = np.random.default_rng(4)
    items = []
    for i in range(n_crops):
        n = int(rng.integers(5, 1200)) if i % 5 else int(rng.integers(1500, 3000))
        yaw = rng.uniform(-np.pi, np.pi)
        c, s = np.cos(yaw), np.sin(yaw)
        R = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
        n_in = n - n // 2
        sel = rng.choice(m.shape[0], n_in)
        p = (R @ (2.0 * m[sel].astype(np.float64)).T).T + np.array([0.2, 0.1, 8.0]) + rng.normal(0, 0.005, (n_in, 3))
        col = mc[sel] + rng.normal(0, 0.01, (n_in, 3))
        po = rng.uniform(p.min(0) - 0.5, p.max(0) + 0.5, (n // 2, 3))
        co = rng.uniform(0, 1, (n // 2, 3))
        items.append((m, mc, np.concatenate([p, po]).astype(np.float32), np.concatenate([col, co]).astype(np.float32), yaw))
    return items


@pytest.mark.parametrize("sampler", ["device", "numpy"])
def test_ragged_frame_equals_each_crop_alone(g15, sampler):
    items = _frame(g15)
    pe = PoseEstimator(type="kabsch", scale=2.0)
    keys = list(range(100, 116))
    np.random.seed(11)
    _, raw = pe.estimate_many([it[:4] for it in items], sampler=sampler, seed=9, keys=keys, return_raw=True)
    np.random.seed(11)
    for i, it in enumerate(items):
        _, one = pe.estimate_many([it[:4]], sampler=sampler, seed=9, keys=[keys[i]], return_raw=True)
        n = it[2].shape[0]
        for key in ("found", "best", "n_inliers", "scale", "rot", "tra", "gate", "counts", "idx"):
            assert torch.equal(raw[key][i], one[key][0]), (i, key)
        assert torch.equal(raw["cnn_idx"][i, :n], one["cnn_idx"][0, :n])


def test_device_sampler_equals_numpy_restatement():
    ncnt = torch.tensor([4, 5, 37, 1000, 3000], dtype=torch.int32, device=DEV)
    keys = [3, 1 << 40, 7, 0, 123456789]
    idx = P.device_sample(ncnt, 567, seed=2024, keys=keys).cpu().numpy()
    for b, n in enumerate(ncnt.tolist()):
        assert np.array_equal(idx[b], P.sample_indices_numpy(2024, keys[b], n, 567)), b


def test_device_sampler_recovers_known_poses(g15):
    items = _frame(g15, 64)
    items = [it for it in items if it[2].shape[0] >= 300]
    res = PoseEstimator(type="kabsch", scale=2.0).estimate_many([it[:4] for it in items], sampler="device", seed=1)
    ok = 0
    for it, r in zip(items, res):
        if r is None:
            continue
        c, s = np.cos(it[4]), np.sin(it[4])
        R = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
        ang = np.degrees(np.arccos(np.clip((np.trace(r["rot"].astype(np.float64) @ R.T) - 1) / 2, -1, 1)))
        ok += ang < 1.0 and np.linalg.norm(r["tra"] - np.array([0.2, 0.1, 8.0])) < 0.05
    ref_rate = int(g15["ref_recovered"]) / int(g15["ref_recovery_cases"])
    assert ok / len(items) >= ref_rate, (ok, len(items), ref_rate)
