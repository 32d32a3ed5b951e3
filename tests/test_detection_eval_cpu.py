"""The evaluator's statistics without a GPU: the golden G17 against the in-repo restatement (tests/_eval_ref.py), the vectorised filters,
the packing, the host half (`finish`, AP, text), the import plumbing of the compat package, and no host fallback."""
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from tests import _eval_golden as GD
from tests import _eval_ref as E
from tests._util import ROOT

from sdflabel_amd import detection_eval as DE

COMPAT = os.path.join(ROOT, "sdflabel_amd", "compat")


@pytest.fixture(scope="module")
def g17():
    return GD.load()


def _cases(d, scenes=None):
    return [(c, m) for c in GD.configs(d) for m in GD.metrics_of(d, c) if scenes is None or str(d[c + "_scene"]) in scenes]


def _same_bits(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def test_g17_meets_its_conditions(g17):
    """no BEV pair the reference is undefined on, scores in (0, 1], every metric with tp, fp and fn, a false positive removed by the
    DontCare rule, pass A and pass B disagreeing on a detection, and scores of 1 changing an AP"""
    info = GD.golden_conditions(g17)
    assert info["removed"] > 0 and info["differ"] > 0
    assert os.path.getsize(GD.PATH) < 1000000


@pytest.mark.parametrize("scene", ["kitti", "ones", "big", "empty"])
def test_restatement_reproduces_g17(g17, scene):
    """pass-A scores, thresholds and the PR rows of every (configuration, metric, combination) from the recorded overlaps and flags:
    integer columns, thresholds and counts exactly, float columns bit for bit"""
    seen = 0
    for cfg, metric in _cases(g17, (scene,)):
        mk = "%s_%s_" % (cfg, GD.METRIC_NAMES[metric])
        fr = GD.frames(g17, scene)
        for c in range(len(g17[mk + "nthr"])):
            scores, thr, pr, _ = E.combination(fr, **GD.combination_inputs(g17, cfg, metric, c))
            n = int(g17[mk + "nthr"][c])
            a, b = g17[mk + "scores_off"][c], g17[mk + "scores_off"][c + 1]
            assert _same_bits(scores, g17[mk + "scores"][a:b]), (cfg, metric, c)
            assert len(thr) == n and _same_bits(thr, g17[mk + "thr"][c][:n]), (cfg, metric, c)
            assert np.array_equal(pr[:, :3], g17[mk + "pr"][c][:n, :3]), (cfg, metric, c)
            assert _same_bits(pr, g17[mk + "pr"][c][:n]), (cfg, metric, c)
            assert not g17[mk + "pr"][c][n:].any()
            seen += 1
    assert seen > 0


def _flags_for(d, cfg, P):
    classes = [str(c) for c in d[cfg + "_classes"]]
    diffs = [int(x) for x in d[cfg + "_difficulties"]]
    if str(d[cfg + "_filter"]) == "clean_kitti_data":
        return DE.clean_kitti_flags(P, classes, diffs)
    return DE.distance_flags(P, classes, diffs, int(d[cfg + "_frame"]))


def test_vectorised_filters_equal_g17(g17):
    for cfg in GD.configs(g17):
        scene = str(g17[cfg + "_scene"])
        P = DE.pack(GD.annos(g17, scene, "gt"), GD.annos(g17, scene, "dt"))
        F = _flags_for(g17, cfg, P)
        assert np.array_equal(F.ign_gt, g17[cfg + "_ign_gt"]) and np.array_equal(F.ign_dt, g17[cfg + "_ign_dt"]), cfg
        assert np.array_equal(F.num_valid, g17[cfg + "_num_valid"]), cfg
        assert np.array_equal(np.diff(F.dc_off, axis=1), g17[cfg + "_dc_num"]), cfg
        want = g17[cfg + "_dc_boxes"]
        got = np.concatenate([np.concatenate(F.dc_lists(ml) or [np.zeros((0, 4))]) for ml in range(F.ign_gt.shape[0])]) \
            if F.ign_gt.shape[0] else np.zeros((0, 4))
        assert np.array_equal(got.reshape(-1, 4), want.reshape(-1, 4)), cfg


@pytest.mark.parametrize("cfg", ["kitti_cam_kitti", "kitti_lidar_nu"])
def test_directly_callable_filters_return_the_recorded_lists(g17, cfg):
    from sdflabel_amd.pipelines import detection_3d as D3
    fn = getattr(D3, str(g17[cfg + "_filter"]))
    gt, dt = GD.annos(g17, "kitti", "gt"), GD.annos(g17, "kitti", "dt", names_as="array")
    ids = GD.id_to_name(g17)
    name_to_id = {v: k for k, v in ids.items()}
    goff, doff = np.concatenate([[0], np.cumsum(g17["kitti_gt_num"])]), np.concatenate([[0], np.cumsum(g17["kitti_dt_num"])])
    dcoff = GD.dc_offsets(g17, cfg)
    L = len(g17[cfg + "_difficulties"])
    for m, cls in enumerate(g17[cfg + "_classes"]):
        for l, diff in enumerate(g17[cfg + "_difficulties"]):
            ml, total = m * L + l, 0
            for f in range(len(gt)):
                n, ig, idt, boxes = fn(gt[f], dt[f], name_to_id[str(cls)], int(diff), ids, D3.CoordinateFrame(int(g17[cfg + "_frame"])))
                assert isinstance(ig, list) and isinstance(idt, list) and isinstance(boxes, list)
                assert ig == g17[cfg + "_ign_gt"][ml][goff[f]:goff[f + 1]].tolist() and idt == g17[cfg + "_ign_dt"][ml][doff[f]:doff[f + 1]].tolist()
                assert len(boxes) == g17[cfg + "_dc_num"][ml][f]
                if boxes:
                    assert np.array_equal(np.stack(boxes), g17[cfg + "_dc_boxes"][dcoff[ml][f]:dcoff[ml][f + 1]])
                total += n
            assert total == g17[cfg + "_num_valid"][ml]


def _finish_all(d, cfg, tables=None):
    """result_dict and text of a configuration from pr tables (G17's own unless given)"""
    M, L = len(d[cfg + "_classes"]), len(d[cfg + "_difficulties"])
    S, ang, nu = int(d[cfg + "_sample_points"]), bool(int(d[cfg + "_angular"])), bool(int(d[cfg + "_nuscenes"]))
    res = {}
    names = {0: ("Box2DAP", "bbox_2d_pre_curves"), 1: ("BevAP", "bev_pre_curves"), 2: ("Box3DAP", "bbox_3d_kitti_pre_curves"),
             3: ("Box3DAP_Nu", "bbox_3d_nu_pre_curves")}
    for metric in GD.metrics_of(d, cfg):
        mk = "%s_%s_" % (cfg, GD.METRIC_NAMES[metric])
        pr, nthr = (d[mk + "pr"], d[mk + "nthr"]) if tables is None else tables[metric]
        curves = DE.finish(pr, nthr, (M, L, 2), metric == 3, ang and metric in (2, 3))
        res[names[metric][1]] = curves
        res[names[metric][0]] = DE.mean_ap(curves["precision"], curves["recall"], S)
        if ang and metric in (2, 3):
            suffix = "dist" if metric == 3 else "iou"
            res["AoeAP_" + suffix] = DE.mean_ap(curves["orientation_aoe"], curves["recall"], S)
            res["AosAP_" + suffix] = DE.mean_ap(curves["orientation_aos"], curves["recall"], S)
    name_to_id = {v: k for k, v in GD.id_to_name(d).items()}
    ids = [name_to_id[str(c)] for c in d[cfg + "_classes"]]
    table = (d["dist_thresholds"] if nu else d["overlap_thresholds"])[:, :, :, ids]
    text = DE.format_result(None, [str(c) for c in d[cfg + "_classes"]], [int(x) for x in d[cfg + "_difficulties"]], nu, ang, table, res)
    return res, text


def test_finish_reproduces_every_result_array_and_the_text(g17):
    for cfg in GD.configs(g17):
        res, text = _finish_all(g17, cfg)
        keys = [k[len(cfg) + 5:] for k in g17 if k.startswith(cfg + "_res_")]
        assert keys
        flat = {}
        for k, v in res.items():
            if isinstance(v, dict):
                flat.update({"%s_%s" % (k, c): a for c, a in v.items()})
            else:
                flat[k] = v
        assert sorted(flat) == sorted(keys), cfg
        for k in keys:
            want = g17["%s_res_%s" % (cfg, k)]
            assert flat[k].shape == want.shape and np.array_equal(flat[k], want, equal_nan=True), (cfg, k)
        assert text == str(g17[cfg + "_text"]), cfg


def test_packing_names_offsets_and_empty_frames(g17):
    gt, dt = GD.annos(g17, "kitti", "gt"), GD.annos(g17, "kitti", "dt")
    P = DE.pack(gt, dt)
    assert P.G == 57 and np.array_equal(P.gt.num, g17["kitti_gt_num"]) and np.array_equal(P.dt.num, g17["kitti_dt_num"])
    assert np.array_equal(P.gt.off, np.concatenate([[0], np.cumsum(g17["kitti_gt_num"])]))
    assert np.array_equal(P.ooff[1:], np.cumsum(g17["kitti_gt_num"].astype(np.int64) * g17["kitti_dt_num"]))
    assert [P.vocab[i] for i in P.gt.name_id] == [str(n).lower() for n in g17["kitti_gt_name"]]
    assert np.array_equal(P.dt.bbox, g17["kitti_dt_bbox"]) and np.array_equal(P.gt.location, g17["kitti_gt_location"])
    # names as arrays and in mixed case give the same ids and flags
    gt2 = [dict(a, name=np.array([n.upper() if i % 2 else n for i, n in enumerate(a["name"])], dtype=str)) for a in gt]
    dt2 = [dict(a, name=np.array([n.swapcase() for n in a["name"]], dtype=str)) for a in dt]
    P2 = DE.pack(gt2, dt2)
    assert P2.vocab == P.vocab and np.array_equal(P2.gt.name_id, P.gt.name_id) and np.array_equal(P2.dt.name_id, P.dt.name_id)
    a, b = DE.clean_kitti_flags(P, ["Car", "Pedestrian"], [0, 2]), DE.clean_kitti_flags(P2, ["cAR", "PEDESTRIAN"], [0, 2])
    assert np.array_equal(a.ign_gt, b.ign_gt) and np.array_equal(a.ign_dt, b.ign_dt)
    assert P.name_id("Tram") == -1 and not (DE.clean_kitti_flags(P, ["Tram"], [0]).ign_gt == 0).any()
    # only empty frames; detections without the ground-truth-only columns
    E0 = DE.pack(GD.annos(g17, "empty", "gt"), GD.annos(g17, "empty", "dt"))
    assert E0.G == 3 and E0.gt.n == 0 and E0.dt.n == 0 and E0.gt.bbox.shape == (0, 4) and E0.vocab == []
    dt3 = [{k: v for k, v in a.items() if k not in ("truncated", "occluded")} for a in dt]
    P3 = DE.pack(gt, dt3)
    assert P3.dt.truncated is None and np.array_equal(DE.clean_kitti_flags(P3, ["Car"], [1]).ign_dt, DE.clean_kitti_flags(P, ["Car"], [1]).ign_dt)
    with pytest.raises(AssertionError):
        DE.pack(gt, dt[:-1])


def test_callable_flags_pack_what_a_user_filter_returns(g17):
    gt, dt = GD.annos(g17, "kitti", "gt"), GD.annos(g17, "kitti", "dt")
    ids = GD.id_to_name(g17)
    name_to_id = {v: k for k, v in ids.items()}

    def mine(*a):
        return DE.clean_kitti_data(*a)

    F = DE.callable_flags(mine, gt, dt, [name_to_id["Car"], name_to_id["Cyclist"]], [0, 1, 2], ids, DE.CAMERA)
    V = DE.clean_kitti_flags(DE.pack(gt, dt), ["Car", "Cyclist"], [0, 1, 2])
    assert np.array_equal(F.ign_gt, V.ign_gt) and np.array_equal(F.ign_dt, V.ign_dt) and np.array_equal(F.num_valid, V.num_valid)
    for ml in range(6):
        assert all(np.array_equal(a, b) for a, b in zip(F.dc_lists(ml), V.dc_lists(ml)))


def test_evaluator_plumbing_without_reference_constants(g17):
    """get_shards, get_mAP and the lazily resolved defaults: without the reference's pipelines.constants the tables must be passed"""
    from sdflabel_amd.pipelines import detection_3d as D3
    with pytest.raises(ValueError, match="pipelines.constants"):
        D3.Detection3DEvaluator(D3.clean_kitti_data)
    ev = D3.Detection3DEvaluator(D3.clean_kitti_data, GD.id_to_name(g17), g17["overlap_thresholds"], g17["dist_thresholds"])
    assert ev.get_shards(57, 50) == [1] * 50 + [7] and ev.get_shards(3, 50) == [3] and ev.get_shards(100, 50) == [2] * 50
    assert int(D3.Metrics.BBOX_3D_NU_AP) == 3 and int(D3.CoordinateFrame.CAMERA) == 2
    assert D3.angle_diff(3.0, -3.0, 2 * np.pi) == pytest.approx(6.0 - 2 * np.pi)
    c = g17["kitti_cam_kitti_res_bbox_2d_pre_curves_precision"], g17["kitti_cam_kitti_res_bbox_2d_pre_curves_recall"]
    assert np.array_equal(ev.get_mAP(*c), g17["kitti_cam_kitti_res_Box2DAP"], equal_nan=True)


def _tree_with_poisoned_evaluator(root):
    """a stand-in of the reference's layout whose own pipelines/detection_3d.py and rotate_iou.py must never be imported"""
    pkg = root / "pipelines"
    pkg.mkdir(parents=True)
    (pkg / "detection_3d.py").write_text("raise ImportError('the reference-like numba detection_3d.py was imported')\n")
    (pkg / "rotate_iou.py").write_text("raise ImportError('the reference-like numba.cuda rotate_iou.py was imported')\n")
    (pkg / "constants.py").write_text("KITTI_CLASS_NAMES = {0: 'Car'}\nKITTI_OVERLAP_THRESHOLDS = 'iou'\nNU_OVERLAP_THRESHOLDS = 'dist'\n")
    (pkg / "evaluate_standin.py").write_text("from pipelines.detection_3d import Detection3DEvaluator, clean_kitti_data, CoordinateFrame  # noqa: F401\n")
    (root / "main.py").write_text(textwrap.dedent("""
        import os, sys
        import pipelines.evaluate_standin as s
        import pipelines.detection_3d as d
        print(os.path.dirname(os.path.abspath(s.__file__)))
        print(os.path.abspath(d.__file__))
        print([int(m in sys.modules) for m in ('numba', 'scipy', 'mpi4py')])
        ev = s.Detection3DEvaluator(s.clean_kitti_data, coordinate_frame=s.CoordinateFrame.CAMERA)
        print(ev.overlap_thresholds, ev.dist_thresholds, ev.id_to_name)
    """))
    return pkg


@pytest.mark.parametrize("launch", ["script", "compat_first"])
def test_compat_detection_3d_wins_over_the_reference_portion(tmp_path, launch):
    ref = tmp_path / "reference"
    pkg = _tree_with_poisoned_evaluator(ref)
    work = tmp_path / "elsewhere"
    work.mkdir()
    if launch == "script":
        env = dict(os.environ, PYTHONPATH=os.pathsep.join([COMPAT, ROOT]))
        cmd = [sys.executable, str(ref / "main.py")]
    else:
        env = dict(os.environ, PYTHONPATH=os.pathsep.join([COMPAT, str(ref), ROOT]))
        cmd = [sys.executable, "-c", "import runpy; runpy.run_path(%r)" % str(ref / "main.py")]
    res = subprocess.run(cmd, env=env, cwd=str(work), capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    lines = res.stdout.strip().splitlines()
    assert os.path.realpath(lines[0]) == os.path.realpath(str(pkg))
    assert os.path.realpath(lines[1]) == os.path.realpath(os.path.join(COMPAT, "pipelines", "detection_3d.py"))
    assert lines[2] == "[0, 0, 0]"
    assert lines[3] == "iou dist {0: 'Car'}"          # the defaults come from the tree's own pipelines/constants.py


def test_no_host_fallback_without_gpu(g17):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: tests/test_gpu_detection_eval.py covers the device path")
    from sdflabel_amd import SdfrError
    from sdflabel_amd.pipelines import detection_3d as D3
    gt, dt = GD.annos(g17, "kitti", "gt"), GD.annos(g17, "kitti", "dt")
    ev = D3.Detection3DEvaluator(D3.clean_kitti_data, GD.id_to_name(g17), g17["overlap_thresholds"], g17["dist_thresholds"],
                                 coordinate_frame=D3.CoordinateFrame.CAMERA)
    P = DE.pack(gt, dt)
    calls = [lambda: ev.evaluate_detection_3d(gt, dt, ["Car"], difficulties=(0, 1)),
             lambda: ev.eval_metric(gt, dt, [2], (0,), D3.Metrics.BBOX_2D_AP, g17["overlap_thresholds"][:, :, :, [2]], None),
             lambda: ev.calculate_match_degree_sharded(gt, dt, D3.Metrics.BEV_3D_AP, 50),
             lambda: D3.get_thresholds(np.array([0.5, 0.7]), 3),
             lambda: DE.Session(P, DE.CAMERA),
             lambda: DE.Frames(P.gt.num, P.dt.num, P.dt.score)]
    for call in calls:
        with pytest.raises(SdfrError):
            call()
