"""The RANSAC pose initialisation without a GPU: csrc/pose_cells.h and csrc/jacobi3.h compiled into a host program
(tests/pose_host/pose_host.cpp) against the numpy restatement (tests/_pose_ref.py, (b)) bit for bit -- also under the address and
undefined-behaviour sanitizers --, the restatement against the independent high-precision reference ((a): mpmath SVD, brute-force
neighbours), reference (a) against golden G15, the Jacobi solver against mpmath on the matrices where it could go wrong, and a mutation check
of the host program.  tests/test_gpu_pose_ref.py compares the kernels with the same two references stage by stage.
"""
import functools
import os
import subprocess

import numpy as np
import pytest

from tests import _pose_cases as PC
from tests import _pose_ref as PR
from tests._util import GOLD, build_host_program

f32, f64 = np.float32, np.float64
SAN = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def run_host(exe, tmp, case):
    src, dst = os.path.join(str(tmp), "in.bin"), os.path.join(str(tmp), "out.bin")
    with open(src, "wb") as f:
        f.write(PR.case_bytes(case))
    r = subprocess.run([exe, src, dst], capture_output=True, text=True)
    assert r.returncode == 0, (case["name"], r.returncode, r.stderr[-2000:])
    return PR.parse_out(open(dst, "rb").read(), case)


def host_checks(exe, tmp, names=None):
    for name, case in PC.all_cases().items():
        if names is not None and name not in names:
            continue
        got, ref = run_host(exe, tmp, case), PC.restated(name)
        PR.defined_equal(ref, got, case, name)
        for b in range(case["B"]):          # what must stay unwritten
            N, pc = int(case["ncnt"][b]), int(ref["pcount"][b])
            assert (got["cnn_idx"][b, N:] == -7).all() and (got["mask"][b, N:] == -7).all() and (got["plist"][b, pc:] == -7).all(), name
            assert (got["hyp"][b][ref["counts"][b] < 0] == -7).all(), name


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("pose_host")
    return build_host_program(d, "pose_host/pose_host.cpp", "pose_host"), d


def test_pose_cells_on_the_host_equal_the_restatement_bit_for_bit(host):
    host_checks(*host)


def test_pose_cells_host_program_under_sanitizers(tmp_path):
    host_checks(build_host_program(tmp_path, "pose_host/pose_host.cpp", "pose_host_san", SAN), tmp_path)


# ---- the cases do what they were built for ---------------------------------------------------------------------------------------------------

def test_cases_cover_the_edges_they_name():
    cases = PC.all_cases()
    assert {c["T"] for c in cases.values()} >= {1, 7, 8, 9, 255, 256, 257, 567}
    assert {int(n) for c in cases.values() for n in c["ncnt"]} >= {5, 255, 256, 257, 513}
    assert {int(m) for c in cases.values() for m in c["mcnt"]} >= {1, 2, 255, 256, 257, 600}
    assert list(PC.restated("pass_counts")["pcount"]) == [0, 1, 8, 9]
    rag = cases["ragged"]
    assert rag["B"] == 3 and {5, 513} <= set(rag["ncnt"].tolist()) and {1, 600} <= set(rag["mcnt"].tolist())
    for name in ("random_0", "random_1", "random_2"):
        assert cases[name]["T"] == 64 and cases[name]["ncnt"].max() <= 400 and cases[name]["mcnt"].max() <= 400
        assert PC.restated(name)["found"][0] == 1          # a random case that found nothing would test little


def test_crafted_cases_behave_as_built():
    """the restatement on the crafted samples: flags, counts, the known transforms; the properties that stand in for a unique R"""
    for typ in (0, 1):
        for f16 in (False, True):
            case = PC.crafted_case(typ, f16)
            o = PC.restated(case["name"])
            for b, ex in enumerate(case["expect"]):
                k, g, cnt, row = ex["kind"], o["gate"][b], o["counts"][b], o["hyp"][b, 0]
                what = (case["name"], k)
                if k != "oob":
                    assert g[2] == 0 and g[3] == 0 and cnt[2] == -1 and cnt[3] == -1, what          # the draws with a failing colour
                if k in ("well", "well_negV", "reflection", "coplanar", "thin"):
                    # (a reflected sample is scored, but the best ROTATION leaves its points where no model point is)
                    assert g[0] == 3 and g[1] == 3 and (cnt[0] >= 4 if k != "reflection" else cnt[0] == 0), what
                if "R" in ex:
                    known = np.concatenate([ex["R"] * ex["c"], ex["t"][:, None]], 1).reshape(12)          # the motion the sample was made with
                    assert np.abs(row - known).max() <= 2 * PR.U32 * ex["c"] + 64 * PR.U64, what
                if k.startswith("collinear") or k == "h0":
                    assert g[0] == (7 if typ == 0 else 5), what
                    assert (cnt[0] >= 0) == (typ == 0), what
                if k.startswith("collinear") and typ == 0:
                    R = row.reshape(3, 4)[:, :3].astype(f64)
                    assert np.abs(R @ R.T - np.eye(3)).max() < 4 * PR.U32 and abs(np.linalg.det(R) - 1) < 8 * PR.U32, what
                    assert np.abs(R @ np.array(ex["dir_from"]) - np.array(ex["dir_to"])).max() < 4 * PR.U32, what
                if k == "h0" and typ == 0:
                    assert np.array_equal(row.reshape(3, 4)[:, :3], np.eye(3, dtype=f32)), what
                    mf, mt, _, _ = PR.sample_moments(case["scene"][b, :4], case["model"][b, [0, 0, 0, 0]], f16)
                    assert np.array_equal(row.reshape(3, 4)[:, 3], ((mt - mf) - mt + mt).astype(f32)), what
                if k == "rank_below":
                    assert g[0] == 5 and cnt[0] == -1, what
                if k == "rank_above":
                    assert g[0] == 7 and cnt[0] >= 0, what
                if k == "c_below":
                    assert g[0] == 3 and cnt[0] >= 4, what
                if k == "c_above":
                    assert g[0] == 1 and cnt[0] == -1, what
                if k == "oob":
                    assert list(g) == [3, 0, 0, 3] and cnt[1] == -1 and cnt[2] == -1 and cnt[0] >= 4, what
                    w = [e["kind"] for e in case["expect"]].index("well")
                    assert np.array_equal(o["hyp"][b, 0], o["hyp"][w, 0]) and np.array_equal(o["hyp"][b, 3], o["hyp"][w, 1]), what
            kinds = {e["kind"]: e for e in case["expect"]}
            assert kinds["well_negV"]["detV_negative"] and kinds["reflection"]["detV_negative"] and not kinds["well"]["detV_negative"]


def test_tie_threshold_and_select_cases_behave_as_built():
    cases = PC.all_cases()
    for name, case in cases.items():
        o = PC.restated(name)
        for b, ex in enumerate(case["expect"]):
            what = (name, ex.get("kind"))
            for p, j in ex.get("cnn", {}).items():
                assert o["cnn_idx"][b, p] == j, what
            for p, m in ex.get("mask", {}).items():
                assert o["mask"][b, p] == m, what + (p,)
            for key in ("n_inliers", "found", "best", "pcount"):
                if key in ex:
                    assert o[key][b] == ex[key], what + (key,)
            if "plist" in ex:
                assert list(o["plist"][b, :ex["pcount"]]) == ex["plist"], what
            if ex.get("kind") == "select":
                assert all(o["counts"][b, t] == 7 for t in ex["a_at"]) and all(o["counts"][b, t] == 4 for t in ex["b_at"]), what
                assert (o["counts"][b] >= 0).sum() == len(ex["a_at"]) + len(ex["b_at"]), what
            if ex.get("kind") == "final_deficient":
                assert o["scale"][b] == 0 and not o["rot"][b].any() and not o["tra"][b].any() and o["mask"][b, :4].sum() == 0, what
            if ex.get("kind") in ("metric", "colour_thr", "tie_score", "tie_colour", "count4", "count5", "select", "final_deficient"):
                r = o["hyp"][b, ex.get("a_at", [0])[0]].reshape(3, 4)            # the identity sample: R = I, c = 1, t = +0 exactly
                assert np.array_equal(r[:, :3], np.eye(3, dtype=f32)) and r[:, 3].tobytes() == np.zeros(3, f32).tobytes(), what
    # the ties are ties: equal float32 distances at the two candidates, equal float64 colour distances
    t = cases["ties_k32"]
    tp, mp = t["scene"][1, :9], t["model"][1]
    for p, (i, j) in {4: (10, 11), 5: (12, 13), 6: (14, 290), 7: (16, 17), 8: (18, 19)}.items():
        d = [PR.fma32(*(np.array([tp[p, k] - mp[q, k]], f32) for k in (0, 0)), PR.fma32(*(np.array([tp[p, k] - mp[q, k]], f32) for k in (1, 1)),
                      np.array([(tp[p, 2] - mp[q, 2]) ** 2], f32)))[0] for q in (i, j)]
        assert d[0] == d[1] and d[0] <= 0.015625, p
    _, _, tie = PR.colour_nn_brute(t["mcls"][0], t["scls"][0, :8])
    assert tie[4:8].all()


@pytest.mark.parametrize("tag", ["nonfinite", "nonfinite_p"])
def test_nonfinite_scene_points_score_nothing_and_change_nothing_else(tag):
    """a NaN or infinite scene point: a hypothesis that samples it is scored with 0 inliers (gate 7) or, 'procrustes' only, rejected by
    the rank rule (gate 5); the point is nobody's inlier, every other hypothesis, the winner and the pose are those of the same crop with the point far away"""
    clean, bad = PC.restated(tag + "_clean"), PC.restated(tag)
    assert np.array_equal(clean["gate"][0] & 1, bad["gate"][0] & 1) and np.array_equal(clean["cnn_idx"], bad["cnn_idx"])
    for t in (0, 1):          # 'procrustes' may also reject such a sample by its rank rule, depending on where the NaNs land
        assert (bad["gate"][0, t], bad["counts"][0, t]) in ([(7, 0)] if tag == "nonfinite" else [(7, 0), (5, -1)]), t
    assert np.array_equal(clean["gate"][0, 2:], bad["gate"][0, 2:]) and np.array_equal(clean["counts"][0, 2:], bad["counts"][0, 2:])
    assert clean["hyp"][0, 2:][clean["counts"][0, 2:] >= 0].tobytes() == bad["hyp"][0, 2:][bad["counts"][0, 2:] >= 0].tobytes()
    assert clean["counts"][0, 2:].max() >= 5 and bad["mask"][0, 7] == 0 and bad["mask"][0, 8] == 0 and bad["found"][0] == 1
    for k in ("best", "n_inliers", "found", "rot", "tra", "scale"):
        assert clean[k].tobytes() == bad[k].tobytes(), k
    assert clean["mask"][0, :60].tobytes() == bad["mask"][0, :60].tobytes()


# ---- restatement (b) against reference (a) ------------------------------------------------------------------------------------------------------

def sampled_fits(case, o):
    """(b, t, from, to) of every hypothesis of a restated case that passed the colour gate"""
    for b in range(case["B"]):
        for t in np.flatnonzero(o["gate"][b] & 1):
            ii = o["idx"][b, t]
            yield b, int(t), case["scene"][b, ii], case["model"][b, o["cnn_idx"][b, ii]]


def fit_pair(frm, to, typ, f16):
    """restatement (b) in float64 and reference (a) of one sample: ((ok, R, c, t, ratio), fit)"""
    mf, mt, H, sig = PR.sample_moments(frm, to, f16)
    with np.errstate(all="ignore"):
        rb = PR.rs_fit(H, mf, mt, sig, typ)
    fit = PR.fit_mp(frm, to, typ, False, f16)
    fit["tscale"] = PR.tscale(fit["c"], mf, mt)
    return rb, fit


def measure_case(case, o, stats):
    typ, f16 = case["type"], case["f16"]
    for b, t, frm, to in sampled_fits(case, o):
        (ok, R, c, tr, ratio), fit = fit_pair(frm, to, typ, f16)
        key = case["name"]
        st = stats.setdefault(key, dict(admitted=0, excluded=0, worst=0.0, min_gap=np.inf, type=typ))
        # decisions first: the rank rule and c > 3 as the reference decides them (crafted cases keep a margin; a random sample within
        # 1e-3 of either threshold is not the reference's to decide)
        if typ == 1 and abs(fit["rank_margin"]) > 1e-3 * 3 * PR.EPS32:
            assert ok == fit["ok"], (key, b, t)
        if ok and fit["ok"] and abs(fit["c"] - 3.0) > 1e-6:
            assert bool(f32(c) > f32(3.0)) == bool(f32(fit["c"]) > f32(3.0)) == (o["counts"][b, t] < 0), (key, b, t)
        if fit["gap"] < 1e-3 or not ok:
            st["excluded"] += 1
            continue
        assert (o["gate"][b, t] & 4) == 0 or ratio < 1e-3
        st["admitted"] += 1
        e = PR.fit_err(R, c, tr, fit)
        st["worst"] = max(st["worst"], e * fit["gap"] / PR.U64)
        st["min_gap"] = min(st["min_gap"], fit["gap"])
        if o["counts"][b, t] >= 0:          # the float32 row within the bound of the GPU test
            row_figures(st, o["hyp"][b, t], fit)


def row_figures(st, row, fit):
    d, bound = np.abs(row.astype(f64) - PR.row_exact(fit)), PR.row_bound(fit, PR.K_FIT)
    st["rows"] = st.get("rows", 0) + 1
    st["row_worst"] = max(st.get("row_worst", 0.0), float((d / bound).max()))
    st["row_over"] = st.get("row_over", 0) + int((d > bound).any())


def g15_samples(g, ci):
    c = "c%d_" % ci
    dt = int(g[c + "dtype"])
    typ = PR_TYPES[str(g[c + "type"])]
    model = g["model%d" % dt]
    if typ == 0:
        model = model * model.dtype.type(float(g[c + "scale_model"]))          # the reference's in-dtype `model_pts *= scale_model`
    return c, typ, dt == 16, model.astype(f32), g["model%d_cls" % dt].astype(f32)


PR_TYPES = {"kabsch": 0, "procrustes": 1}


@functools.lru_cache(maxsize=None)
def measured():
    """name -> figures of restatement (b) against reference (a): every gate-passing hypothesis of the suite's cases and of golden G15"""
    stats = {}
    for name, case in PC.all_cases().items():
        if name.startswith("nonfinite"):
            continue
        measure_case(case, PC.restated(name), stats)
    g = np.load(os.path.join(GOLD, "g15_pose_init.npz"))
    for ci in range(int(g["n_cases"])):
        c, typ, f16, model, _ = g15_samples(g, ci)
        st = stats.setdefault("g15_" + str(g["names"][ci]), dict(admitted=0, excluded=0, worst=0.0, min_gap=np.inf, type=typ))
        for t in np.flatnonzero(g[c + "gate"] if len(g[c + "draws"]) else []):
            frm, to = g[c + "scene"][g[c + "draws"][t]], model[g[c + "gate_cnn"][t]]
            (ok, R, cc, tr, ratio), fit = fit_pair(frm, to, typ, f16)
            if fit["gap"] < 1e-3 or not ok:
                st["excluded"] += 1
                continue
            st["admitted"] += 1
            st["worst"] = max(st["worst"], PR.fit_err(R, cc, tr, fit) * fit["gap"] / PR.U64)
            st["min_gap"] = min(st["min_gap"], fit["gap"])
            if not f32(cc) > f32(3.0):
                row_figures(st, PR.hyp_row(R, cc, tr), fit)
    return stats


def test_K_of_the_fit_bound_is_the_measured_one(capsys):
    """K of the fit bound is MEASURED here: the worst err * gap / u64 of restatement (b) against the mpmath reference over every admitted
    hypothesis of the suite's cases and of golden G15; PR.K_WORST records it (rounded up) and PR.K_FIT = 4 * K_WORST is the bound's K."""
    stats = measured()
    worst = max(s["worst"] for s in stats.values())
    with capsys.disabled():
        for k, s in stats.items():
            print("\npose K: %-18s admitted %4d excluded %4d worst err*gap/u64 %7.3f min gap %8.3g rows %4d over %3d worst row/bound %.3f" %
                  (k, s["admitted"], s["excluded"], s["worst"], s["min_gap"], s.get("rows", 0), s.get("row_over", 0), s.get("row_worst", 0.0)), end="")
        print("\npose K: worst %.3f (recorded K_WORST %.3f, K_FIT %.3f); exact-fma path %d of %d candidates" %
              (worst, PR.K_WORST, PR.K_FIT, PR.FMA_EXACT["exact_path"], PR.FMA_EXACT["candidates"]))
    assert worst <= PR.K_WORST and PR.K_FIT == 4 * PR.K_WORST
    assert sum(s["admitted"] for s in stats.values()) > 2000
    for typ in (0, 1):          # no crafted sample of the admitted kinds was excluded
        for f16 in (False, True):
            for ex in PC.crafted_case(typ, f16)["expect"]:
                if ex["kind"] in ("well", "well_negV", "reflection", "coplanar", "thin"):
                    assert ex["fit"]["gap"] >= 1e-3


@pytest.mark.parametrize("fit", ["kabsch", "procrustes"])
def test_restatement_rows_within_the_fit_bound(fit):
    """every float32 row [rot*scale | tra] of the restatement within 2 u32 |R c| + u32 |t| + K u64 / gap of reference (a), u32 = 2^-24.

    This test found a bug: rs_hyp_row formed float32(R) * float32(c) in float32, three roundings, and 9 of 394 'procrustes' rows were
    beyond the bound (the worst at 1.18 of it).  The original implementation's procrustes returns float64 R and c and stores their float64
    product to float32 once; rs_hyp_row now does that ('kabsch', c = 1, keeps its bits)."""
    rows = over = 0
    worst = 0.0
    for k, s in measured().items():
        if s["type"] == PR_TYPES[fit]:
            rows, over, worst = rows + s.get("rows", 0), over + s.get("row_over", 0), max(worst, s.get("row_worst", 0.0))
    assert rows > 300
    assert over == 0, "%d of %d %s rows beyond the bound, the worst at %.3f of it" % (over, rows, fit, worst)


def test_neighbours_and_inlier_decisions_against_brute_force():
    """colour NN equals the float64 brute force except at exact ties, where the lowest index is required; every inlier decision of every
    scored hypothesis equals the float64 brute force where the reference's margin to a threshold or to the runner-up is not tiny"""
    decided = undecided = 0
    for name, case in PC.all_cases().items():
        if name.startswith("nonfinite") or name in ("edge_T257", "ragged"):          # (the big ones are left to the restatement: time)
            continue
        o = PC.restated(name)
        for b in range(case["B"]):
            N, M = int(case["ncnt"][b]), int(case["mcnt"][b])
            mp, mc, sp, sc = case["model"][b, :M], case["mcls"][b, :M], case["scene"][b, :N], case["scls"][b, :N]
            idx, dist, tie = PR.colour_nn_brute(mc, sc)
            assert np.array_equal(o["cnn_idx"][b, :N][~tie], idx[~tie]) and np.allclose(o["cnn_d"][b, :N], dist, rtol=4 * PR.U64, atol=0), name
            for p in np.flatnonzero(tie):
                d = ((sc[p].astype(f64) - mc.astype(f64)) ** 2).sum(1)
                assert o["cnn_idx"][b, p] == np.flatnonzero(d == d.min())[0], (name, p)
            for t in np.flatnonzero(o["counts"][b] >= 0)[:24]:
                inl, margin = PR.score_brute(o["hyp"][b, t], mp, mc, sp, sc, case["metric_thr"], case["nocs_thr"])
                mine = PR.score_stage(case, b, {t: o["hyp"][b, t]})[t]
                sure = margin > 1e-5
                assert np.array_equal(mine[sure], inl[sure]), (name, b, t)
                decided += int(sure.sum())
                undecided += int((~sure).sum())
    assert decided > 10000 and undecided < decided // 20


def test_reference_a_against_g15():
    """reference (a) tied to the recorded run of the original implementation: the colour NN of every drawn point, the gate, every scored
    hypothesis' inlier count (within the golden's own near-threshold slack: its transforms came out of a float32 SVD) and the final poses of
    all eleven cases"""
    from scipy.spatial import cKDTree
    g = np.load(os.path.join(GOLD, "g15_pose_init.npz"))
    thr = float(g["threshold"])
    scored = 0
    for ci in range(int(g["n_cases"])):
        c, typ, f16, model, mcls = g15_samples(g, ci)
        name = str(g["names"][ci])
        scene, scls, draws = g[c + "scene"], g[c + "scene_cls"], g[c + "draws"]
        if len(draws):
            idx, dist, tie = PR.colour_nn_brute(mcls, scls)
            assert not tie[np.unique(draws)].any() and np.array_equal(idx[draws], g[c + "gate_cnn"]), name
            assert np.array_equal((dist[draws] <= thr).all(1).astype(np.int32), g[c + "gate"]), name
            tree = cKDTree(model.astype(f64))
            for t in np.flatnonzero(g[c + "counts"] >= 0):
                fit = PR.fit_mp(scene[draws[t]], model[idx[draws[t]]], typ, False, f16)
                if fit["gap"] < 1e-3:
                    continue
                assert fit["ok"] and not f32(fit["c"]) > f32(3.0), (name, t)
                d, nn = tree.query(PR.transform(PR.row_mp(fit), scene).astype(f64))
                dc = np.linalg.norm(scls - mcls[nn], axis=1)          # float32, as recorded
                cnt = int(((d < thr) & (dc < thr)).sum())
                assert abs(cnt - int(g[c + "counts"][t])) <= int(g[c + "near"][t]), (name, t, cnt, int(g[c + "counts"][t]))
                scored += 1
        assert int(g[c + "found"]) == (1 if name in ("k32_1000", "k32_3000", "k32_300", "k16_1000", "k16_300", "p32_1000", "p32_300") else 0)
        if int(g[c + "found"]):
            rows = g[c + "final_rows"]
            fit = PR.fit_mp(model[g[c + "final_cnn"][:len(rows)]], scene[rows], typ, f16, False, numpy_means=False)
            assert np.abs(fit["R"] - g[c + "rot"]).max() < 1e-5 and np.abs(fit["t"] - g[c + "tra"]).max() < 1e-4, name
            if typ == 1:
                assert abs(fit["c"] - float(g[c + "scale"])) <= 1e-5 * fit["c"], name
    assert scored > 1000


# ---- the Jacobi solver ------------------------------------------------------------------------------------------------------------------------

def jacobi_inputs():
    rng = np.random.default_rng(7)
    out = []
    for _ in range(24):
        a = rng.normal(size=(3, 3))
        out.append(a + a.T)
    out += [np.diag(v) for v in ([3.0, 1.0, 2.0], [1.0, 2.0, 3.0], [-1.0, 5.0, 0.0], [2.0, 3.0, 1.0])]
    q = np.linalg.qr(rng.normal(size=(3, 3)))[0]
    out += [q @ np.diag(v) @ q.T for v in ([2.0, 2.0, 1.0], [3.0, 1.0, 1.0], [1.0, 1.0, 1.0], [4.0, 0.0, 0.0], [4.0, 1.0, 0.0])]
    out += [np.zeros((3, 3)), np.eye(3), np.outer([1.0, 2.0, 2.0], [1.0, 2.0, 2.0]), np.outer(q[0], q[0]) + 2 * np.outer(q[1], q[1])]
    out = [(m + m.T) / 2 for m in out]
    n = len(out)
    out += [m * 1e-150 for m in out[:n]] + [m * 1e150 for m in out[:n]]
    return np.array(out, f64)


def judge_jacobi(S, lam, V):
    import mpmath
    mpmath.mp.dps = 50
    c = 16.0          # a cyclic Jacobi on a 3 x 3: a few sweeps of three rotations, each a handful of roundings per entry
    norm = float(np.abs(S).max())
    assert np.isfinite(lam).all() and np.isfinite(V).all()
    assert lam[0] >= lam[1] >= lam[2]
    assert np.abs(V.T @ V - np.eye(3)).max() <= 1e-14
    Sm, Vm = mpmath.matrix(S.tolist()), mpmath.matrix(V.tolist())
    res = Sm * Vm - Vm * mpmath.diag([mpmath.mpf(float(v)) for v in lam])
    assert max(abs(res[i, j]) for i in range(3) for j in range(3)) <= c * PR.U64 * norm
    E, _ = mpmath.eigsy(Sm)
    ref = sorted((E[i] for i in range(3)), reverse=True)
    assert max(abs(mpmath.mpf(float(lam[i])) - ref[i]) for i in range(3)) <= c * PR.U64 * norm
    assert abs(abs(np.linalg.det(V)) - 1) <= 1e-14


def test_jacobi3_against_mpmath(host):
    exe, tmp = host
    S = jacobi_inputs()
    src, dst = os.path.join(str(tmp), "j_in.bin"), os.path.join(str(tmp), "j_out.bin")
    with open(src, "wb") as f:
        f.write(S.tobytes())
    assert subprocess.run([exe, "jacobi", src, dst]).returncode == 0
    raw = np.fromfile(dst, f64)
    lam, V = raw[:3 * len(S)].reshape(-1, 3), raw[3 * len(S):].reshape(-1, 3, 3)
    for k in range(len(S)):
        with np.errstate(all="ignore"):
            l2, V2 = PR.jacobi3(S[k])
        assert l2.tobytes() == lam[k].tobytes() and V2.tobytes() == V[k].tobytes(), k          # host program == restatement
        judge_jacobi(S[k], lam[k], V[k])
    # the sign of det V is consistent with the R it produces: a proper R whichever sign V came out with
    seen = set()
    for k in range(24):
        H = np.random.default_rng(k).normal(size=(3, 3))
        info = {}
        ok, R, c, t, ratio = PR.rs_fit(H, np.zeros(3), np.zeros(3), 1.0, 0, info)
        seen.add(info["detV"] < 0)
        assert abs(np.linalg.det(R) - 1) < 1e-13 and np.abs(R @ R.T - np.eye(3)).max() < 1e-13
        fit = PR.fit_mp_H(H.tolist(), np.zeros(3), np.zeros(3), 1.0, 0)
        assert np.abs(R - fit["R"]).max() * fit["gap"] <= PR.K_FIT * PR.U64, k
    assert seen == {True, False}


# ---- the mutation check --------------------------------------------------------------------------------------------------------------------------

MUTANTS = {"MUT_CNN_TIE_LAST": "ties_k32", "MUT_SELECT_GE": "select_ties", "MUT_DROP_SV": "crafted_k32", "MUT_METRIC_LE": "metric_up1",
           "MUT_NO_F16_MEAN_ROUND": "random_2"}


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_every_mutant_of_the_host_program_is_caught(tmp_path, mutant):
    """each mutant changes one call site of the HOST PROGRAM (a -D switch in tests/pose_host/pose_host.cpp; pose_cells.h has none): the case
    named for it must then differ from the restatement"""
    exe = build_host_program(tmp_path, "pose_host/pose_host.cpp", "pose_host_" + mutant.lower(), ["-D" + mutant])
    with pytest.raises(AssertionError):
        host_checks(exe, tmp_path, names=[MUTANTS[mutant]])
    cells = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "sdflabel_amd", "csrc", "pose_cells.h")).read()
    assert "MUT_" not in cells


def test_workspace_views_mirror_the_library_layout():
    from sdflabel_amd import _lib
    from sdflabel_amd import pose as P
    h = _lib.lib()
    for B, ncap, T in ((1, 1, 1), (1, 5, 7), (3, 513, 64), (4, 6, 16), (2, 257, 255), (1, 256, 256), (16, 3000, 567), (7, 31, 33), (1, 32, 8), (5, 1000, 9),
                       (64, 64, 64), (2, 1, 567)):
        segs, total = P.workspace_layout(B, ncap, T)
        assert total == h.sdfr_ransac_ws_bytes(B, ncap, T), (B, ncap, T)
        assert [s[0] for s in segs] == ["cnn_d", "hyp", "plist", "pcount", "mask"] and all(s[1] % 256 == 0 for s in segs)
