"""The seven kernels of csrc/pose.hip against the two references of tests/_pose_ref.py, stage by stage: every link is judged on its own
from the device's own upstream outputs (the pattern of tests/test_gpu_trace_ref.py).  (b), the operation-order restatement, must be met in
every integer and every defined float bit; (a), the independent mpmath / brute-force reference, within the rounding bounds of the number
formats plus K u64 / gap (K measured on the CPU: tests/test_pose_refs_cpu.py, profiles/pose_tests_notes.md).
Every launch runs between guard words on all its outputs and on the workspace's tail; the workspace starts as a byte pattern, so what the
kernels must leave unwritten is checked too.  tests/test_pose_refs_cpu.py pins the references themselves (host build, sanitizers, G15).
"""
import ctypes

import numpy as np
import pytest
import torch

from sdflabel_amd import _lib
from sdflabel_amd import pose as P
from tests import _pose_cases as PC
from tests import _pose_ref as PR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
f32, f64 = np.float32, np.float64
PAD = 64                      # guard words in front of and behind every output
SENT_I, SENT_B = -1234567, 0xA5
CASES = sorted(PC.CASE_NAMES)
_RUNS = {}


class Out:
    """a device array between two guards of PAD sentinel words; starts all sentinel"""

    def __init__(self, shape, dtype):
        self.shape, self.dtype = tuple(shape), dtype
        self.n = int(np.prod(self.shape))
        self.full = torch.as_tensor(np.full(self.n + 2 * PAD, SENT_I, np.int32), device=DEV)

    @property
    def p(self):
        return self.full.data_ptr() + PAD * 4

    def get(self):
        w = self.full.cpu().numpy()
        assert (w[:PAD] == SENT_I).all() and (w[PAD + self.n:] == SENT_I).all(), "a guard was written"
        return w[PAD:PAD + self.n].view(self.dtype).reshape(self.shape).copy()


def launch(case):
    """sdfr_ransac_pose on the packed arrays of a case, every output and the workspace guarded; returns numpy arrays, the workspace's five
    segments among them (undefined entries: the 0xA5 pattern)"""
    B, T, ncap, mcap = case["B"], case["T"], case["scene"].shape[1], case["model"].shape[1]
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=DEV)
    model, mcls, scene, scls, mcnt, ncnt = (t(case[k]) for k in ("model", "mcls", "scene", "scls", "mcnt", "ncnt"))
    keys = t(case["keys"])
    idx_in = None if case["idx"] is None else t(case["idx"])
    outs = dict(found=Out((B,), np.int32), best=Out((B,), np.int32), n_inliers=Out((B,), np.int32), scale=Out((B,), f32), rot=Out((B, 9), f32),
                tra=Out((B, 3), f32), cnn_idx=Out((B, ncap), np.int32), gate=Out((B, T), np.int32), counts=Out((B, T), np.int32), idx=Out((B, T, 4), np.int32))
    h = _lib.lib()
    segs, total = P.workspace_layout(B, ncap, T)
    assert total == h.sdfr_ransac_ws_bytes(B, ncap, T)
    ws = torch.full((total + 256,), SENT_B, dtype=torch.uint8, device=DEV)
    assert ws.data_ptr() % 256 == 0
    thr = (ctypes.c_double * 2)(case["metric_thr"], case["nocs_thr"])
    rc = h.sdfr_ransac_pose(model.data_ptr(), mcls.data_ptr(), mcnt.data_ptr(), mcap, int(case["f16"]), scene.data_ptr(), scls.data_ptr(),
                            ncnt.data_ptr(), ncap, B, None if idx_in is None else idx_in.data_ptr(), case["seed"], keys.data_ptr(), T, case["type"],
                            case["scale_model"], ctypes.cast(thr, ctypes.c_void_p), ws.data_ptr(), outs["found"].p, outs["best"].p,
                            outs["n_inliers"].p, outs["scale"].p, outs["rot"].p, outs["tra"].p, outs["cnn_idx"].p, outs["gate"].p,
                            outs["counts"].p, outs["idx"].p, _lib.stream_ptr())
    torch.cuda.synchronize()
    _lib.check(rc, "sdfr_ransac_pose")
    o = {k: v.get() for k, v in outs.items()}
    if idx_in is not None:
        assert (o["idx"].view(np.int32) == SENT_I).all(), "idx_out was written although the draws were handed in"
        o["idx"] = case["idx"].copy()
    raw = ws.cpu().numpy()
    assert (raw[total:] == SENT_B).all(), "the workspace's tail was written"
    at = 0
    for name, nbytes, dtype, shape in segs:
        npdt = {torch.float64: f64, torch.float32: f32, torch.int32: np.int32}[dtype]
        n = int(np.prod(shape)) * np.dtype(npdt).itemsize
        o[name] = raw[at:at + n].view(npdt).reshape(shape).copy()
        assert (raw[at + n:at + nbytes] == SENT_B).all(), "the padding after %s was written" % name
        at += nbytes
    return o


def run(name):
    if name not in _RUNS:
        _RUNS[name] = launch(PC.all_cases()[name])
    return _RUNS[name]


def unwritten(a):
    return (np.ascontiguousarray(a).view(np.uint8) == SENT_B).all()


# ---- layout and sampler -------------------------------------------------------------------------------------------------------------------------

def test_workspace_views_mirror_the_library_and_a_run():
    h = _lib.lib()
    for B, ncap, T in ((1, 1, 1), (1, 5, 7), (3, 513, 64), (4, 6, 16), (2, 257, 255), (1, 256, 256), (16, 3000, 567), (7, 31, 33), (1, 32, 8), (5, 1000, 9),
                       (64, 64, 64), (2, 1, 567)):
        assert P.workspace_layout(B, ncap, T)[1] == h.sdfr_ransac_ws_bytes(B, ncap, T), (B, ncap, T)
    # the Python entry point on a crafted case: its views hold what the guarded launch of the same packed arrays left
    case, dev = PC.all_cases()["crafted_p16"], run("crafted_p16")
    lists = lambda k, cnt, dt: [torch.from_numpy(case[k][b, :int(case[cnt][b])].astype(dt)) for b in range(case["B"])]
    out = P.ransac_pose(lists("model", "mcnt", np.float16), lists("mcls", "mcnt", np.float16), lists("scene", "ncnt", f32), lists("scls", "ncnt", f32),
                        type="procrustes", idx=list(case["idx"]), sampler="numpy", iterations=case["T"], device=DEV)
    v = {k: x.cpu().numpy() for k, x in P.workspace_views(out).items()}
    got = {k: out[k].cpu().numpy() for k in ("found", "best", "n_inliers", "scale", "rot", "tra", "cnn_idx", "gate", "counts", "idx")}
    got["rot"] = got["rot"].reshape(-1, 9)
    got.update(v)
    PR.defined_equal(dev, got, case, "ransac_pose")


def test_device_sampler_at_n4_and_the_edges_of_a_workgroup():
    for T in (1, 7, 8, 9, 255, 256, 257, 567):
        ncnt = torch.tensor([4, 3, 5, 257], dtype=torch.int32, device=DEV)
        keys = [0, 9, 1 << 40, -3]
        idx = P.device_sample(ncnt, T, seed=-5, keys=keys).cpu().numpy()
        for b, n in enumerate(ncnt.tolist()):
            ref = P.sample_indices_numpy(-5, keys[b], n, T)
            assert np.array_equal(idx[b], ref), (T, b)
            assert (np.sort(ref, 1)[:, 1:] != np.sort(ref, 1)[:, :-1]).all() or n < 4
        assert sorted(idx[0, 0]) == [0, 1, 2, 3] and not idx[1].any()


# ---- (b): every integer, every defined float bit ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", CASES)
def test_whole_chain_equals_the_restatement(name):
    """from the inputs alone: gate, counts, plist, pcount, best, mask, found, n_inliers and every defined float bit (cnn_d, hyp rows of scored
    hypotheses, scale, rot, tra); what the kernels must not write is still the pattern"""
    case, dev, ref = PC.all_cases()[name], run(name), PC.restated(name)
    PR.defined_equal(ref, dev, case, name)
    for b in range(case["B"]):
        N, pc = int(case["ncnt"][b]), int(dev["pcount"][b])
        assert (dev["cnn_idx"][b, N:] == SENT_I).all() and unwritten(dev["cnn_d"][b, N:]) and unwritten(dev["mask"][b, N:]), name
        assert unwritten(dev["plist"][b, pc:]) and unwritten(dev["hyp"][b][dev["counts"][b] < 0]), name


@pytest.mark.parametrize("name", CASES)
def test_every_stage_from_the_devices_own_upstream(name):
    """each link on its own: the colour-NN table from the inputs; gate / plist / hyp rows from the device's table; counts from the device's
    rows; best from the device's counts (first maximum); the mask from the device's winner and rows; the final fit from the device's mask"""
    case, dev = PC.all_cases()[name], run(name)
    ref = PR.restate(case, device=dev)
    PR.defined_equal(ref, dev, case, name)
    for b in range(case["B"]):
        N, cnt = int(case["ncnt"][b]), dev["counts"][b]
        top = int(cnt.max())
        first = int(np.argmax(cnt)) if top > 0 else -1
        assert dev["best"][b] == first and dev["n_inliers"][b] == max(top, 0), (name, b)
        assert int(dev["mask"][b, :N].sum()) == dev["n_inliers"][b], (name, b)
        assert ((dev["gate"][b] & 2) != 0).tolist() == (cnt >= 0).tolist() and list(dev["plist"][b, :dev["pcount"][b]]) == list(np.flatnonzero(cnt >= 0))


def test_what_the_builders_know_holds_on_the_device():
    """the crafted flags and counts, the forced ties, the thresholds and the select rules, read from the device"""
    for name, case in PC.all_cases().items():
        dev = run(name)
        for b, ex in enumerate(case["expect"]):
            what = (name, b, ex.get("kind"))
            for p, j in ex.get("cnn", {}).items():
                assert dev["cnn_idx"][b, p] == j, what
            for p, m in ex.get("mask", {}).items():
                assert dev["mask"][b, p] == m, what
            for key in ("n_inliers", "found", "best", "pcount"):
                if key in ex:
                    assert dev[key][b] == ex[key], what + (key,)
            if "plist" in ex:
                assert list(dev["plist"][b, :ex["pcount"]]) == ex["plist"], what
            k, g, cnt = ex.get("kind"), dev["gate"][b], dev["counts"][b]
            typ = case["type"]
            if k == "final_deficient":
                assert dev["scale"][b] == 0 and not dev["rot"][b].any() and not dev["tra"][b].any(), what
            if k in ("collinear_axis", "collinear_skew", "h0"):
                assert g[0] == (7 if typ == 0 else 5) and (cnt[0] >= 0) == (typ == 0), what
            if k in ("collinear_axis", "collinear_skew") and typ == 0:
                R = dev["hyp"][b, 0].reshape(3, 4)[:, :3].astype(f64)
                assert np.abs(R @ R.T - np.eye(3)).max() < 4 * PR.U32 and abs(np.linalg.det(R) - 1) < 8 * PR.U32, what
                assert np.abs(R @ np.array(ex["dir_from"]) - np.array(ex["dir_to"])).max() < 4 * PR.U32, what
            if k == "h0" and typ == 0:
                row = dev["hyp"][b, 0].reshape(3, 4)
                mf, mt, _, _ = PR.sample_moments(case["scene"][b, :4], case["model"][b, [0, 0, 0, 0]], case["f16"])
                assert np.array_equal(row[:, :3], np.eye(3, dtype=f32)) and np.array_equal(row[:, 3], ((mt - mf) - mt + mt).astype(f32)), what
            if k in ("rank_below", "rank_above", "c_below", "c_above"):
                assert (g[0], cnt[0] >= 0) == {"rank_below": (5, False), "rank_above": (7, True), "c_below": (3, True), "c_above": (1, False)}[k], what
            if k == "oob":
                w = [e["kind"] for e in case["expect"]].index("well")
                assert list(g) == [3, 0, 0, 3] and cnt[1] == -1 and cnt[2] == -1, what
                assert dev["hyp"][b, 0].tobytes() == dev["hyp"][w, 0].tobytes() and dev["hyp"][b, 3].tobytes() == dev["hyp"][w, 1].tobytes(), what


@pytest.mark.parametrize("tag", ["nonfinite", "nonfinite_p"])
def test_nonfinite_scene_points_score_nothing_and_change_nothing_else(tag):
    """a NaN or infinite scene point: a hypothesis that samples it is scored with 0 inliers (gate 7) or, 'procrustes' only, rejected by
    the rank rule (gate 5); the point is nobody's inlier, every other hypothesis, the winner and the pose are those of the same crop with the point far away"""
    clean, bad = run(tag + "_clean"), run(tag)
    assert np.array_equal(clean["gate"][0] & 1, bad["gate"][0] & 1) and np.array_equal(clean["cnn_idx"], bad["cnn_idx"])
    for t in (0, 1):          # 'procrustes' may also reject such a sample by its rank rule, depending on where the NaNs land
        assert (bad["gate"][0, t], bad["counts"][0, t]) in ([(7, 0)] if tag == "nonfinite" else [(7, 0), (5, -1)]), t
    assert np.array_equal(clean["gate"][0, 2:], bad["gate"][0, 2:]) and np.array_equal(clean["counts"][0, 2:], bad["counts"][0, 2:])
    assert clean["hyp"][0, 2:][clean["counts"][0, 2:] >= 0].tobytes() == bad["hyp"][0, 2:][bad["counts"][0, 2:] >= 0].tobytes()
    assert clean["counts"][0, 2:].max() >= 5 and bad["mask"][0, 7] == 0 and bad["mask"][0, 8] == 0 and bad["found"][0] == 1
    for k in ("best", "n_inliers", "found", "rot", "tra", "scale"):
        assert clean[k].tobytes() == bad[k].tobytes(), k
    assert clean["mask"][0, :60].tobytes() == bad["mask"][0, :60].tobytes()


@pytest.mark.parametrize("name", ["ragged", "pass_counts", "crafted_p32", "thresholds", "select_ties"])
def test_each_crop_alone_gives_the_bits_of_the_batch(name):
    case, dev = PC.all_cases()[name], run(name)
    for b in range(case["B"]):
        one = PC.crop_alone(case, b)
        alone = launch(one)
        N = int(case["ncnt"][b])
        part = {k: (v[b:b + 1, :max(N, 1)] if k in ("cnn_idx", "cnn_d", "mask") else v[b:b + 1]) for k, v in dev.items()}
        PR.defined_equal(part, alone, one, (name, b))


@pytest.mark.parametrize("name", ["ragged", "edge_T567", "random_1", "crafted_k16"])
def test_a_second_run_gives_the_same_bits(name):
    case = PC.all_cases()[name]
    PR.defined_equal(run(name), launch(case), case, name)


# ---- (a): the independent reference -----------------------------------------------------------------------------------------------------------------

def test_colour_nn_equals_the_brute_force_and_ties_go_to_the_lowest_index():
    ties = 0
    for name, case in PC.all_cases().items():
        dev = run(name)
        for b in range(case["B"]):
            N, M = int(case["ncnt"][b]), int(case["mcnt"][b])
            with np.errstate(all="ignore"):
                idx, dist, tie = PR.colour_nn_brute(case["mcls"][b, :M], case["scls"][b, :N])
            assert np.array_equal(dev["cnn_idx"][b, :N][~tie], idx[~tie]) and np.allclose(dev["cnn_d"][b, :N], dist, rtol=4 * PR.U64, atol=0), (name, b)
            for p in np.flatnonzero(tie):
                d = ((case["scls"][b, p].astype(f64) - case["mcls"][b, :M].astype(f64)) ** 2).sum(1)
                assert dev["cnn_idx"][b, p] == np.flatnonzero(d == d.min())[0], (name, b, p)
            ties += int(tie.sum())
    assert ties >= 16


def device_row_figures(typ):
    """(rows, rows beyond the bound, worst |row - (a)| / bound) of the device's scored hypotheses of every case of one fit type"""
    rows = over = 0
    worst = 0.0
    for name, case in PC.all_cases().items():
        if case["type"] != typ or name.startswith("nonfinite"):
            continue
        dev = run(name)
        for b in range(case["B"]):
            for t in np.flatnonzero(dev["counts"][b] >= 0):
                ii = dev["idx"][b, t]
                frm, to = case["scene"][b, ii], case["model"][b, dev["cnn_idx"][b, ii]]
                fit = PR.fit_mp(frm, to, typ, False, case["f16"])
                if fit["gap"] < 1e-3:
                    continue
                mf, mt, _, _ = PR.sample_moments(frm, to, case["f16"])
                fit["tscale"] = PR.tscale(fit["c"], mf, mt)
                d, bound = np.abs(dev["hyp"][b, t].astype(f64) - PR.row_exact(fit)), PR.row_bound(fit, PR.K_FIT)
                rows, over, worst = rows + 1, over + int((d > bound).any()), max(worst, float((d / bound).max()))
    return rows, over, worst


@pytest.mark.parametrize("fit", ["kabsch", "procrustes"])
def test_hypothesis_rows_within_the_fit_bound_of_the_reference(fit):
    """every scored, admitted (gap >= 1e-3) row of the device within 2 u32 |R c| + u32 |t| + K u64 / gap of reference (a), u32 = 2^-24.

    (With float32(R) * float32(c) formed in float32, three roundings, 4 of the 79 'procrustes' rows were beyond it: rs_hyp_row now stores
    the float64 product once, as the original implementation does.)"""
    rows, over, worst = device_row_figures(PR_TYPES[fit])
    print("pose rows (%s): %d rows, %d beyond the bound, worst at %.3f of it" % (fit, rows, over, worst))
    assert rows >= 60
    assert over == 0, "%d of %d %s rows beyond the bound, the worst at %.3f of it" % (over, rows, fit, worst)


PR_TYPES = {"kabsch": 0, "procrustes": 1}


def test_final_pose_within_the_fit_bound_of_the_reference():
    """found, and scale / rot / tra within u32 |value| + K u64 / gap of the mpmath fit of the device's own inliers and colour-NN table"""
    checked = 0
    for name, case in PC.all_cases().items():
        if name.startswith("nonfinite"):
            continue
        dev = run(name)
        for b in range(case["B"]):
            if not dev["found"][b]:
                continue
            N = int(case["ncnt"][b])
            rows = np.flatnonzero(dev["mask"][b, :N])
            frm, to = case["model"][b, dev["cnn_idx"][b, rows]], case["scene"][b, rows]
            fit = PR.fit_mp(frm, to, case["type"], case["f16"], False, numpy_means=False)
            assert fit["ok"], (name, b)
            if fit["gap"] < 1e-3:
                continue
            fit["tscale"] = PR.tscale(fit["c"], np.abs(frm).max(0), np.abs(to).max(0))
            bR, bt, bc = PR.final_bound(fit, PR.K_FIT)
            assert (np.abs(dev["rot"][b].astype(f64) - fit["R"].reshape(9)) <= bR).all(), (name, b)
            assert (np.abs(dev["tra"][b].astype(f64) - fit["t"]) <= bt).all(), (name, b, np.abs(dev["tra"][b].astype(f64) - fit["t"]) / bt)
            if case["type"] == 1:
                assert abs(float(dev["scale"][b]) - fit["c"]) <= bc, (name, b)
            else:
                assert dev["scale"][b] == f32(case["scale_model"]), (name, b)
            checked += 1
    assert checked >= 12
