"""Access to the golden G17 (tests/golden/g17_detection_eval.npz, written by tools/make_golden_eval.py) for the evaluator's tests, and the
conditions the file has to meet so that a test on it cannot hide a failure.

Keys.  Per scene s in (kitti, ones, big, empty): s_gt_num / s_dt_num [G] and the concatenated annotation columns s_gt_<key> / s_dt_<key>
(name, truncated, occluded, alpha, bbox, dimensions, location, rotation_y, score).  ov_<scene>_<frame>_<metric>: the frames' [nd][ng]
overlap blocks one after the other (BEV / 3-D as the float32 values they are).  Per configuration c in `configs`: c_scene, c_filter,
c_frame, c_nuscenes, c_angular, c_sample_points, c_classes, c_difficulties, c_text, c_res_<result_dict key>[_<curve>], the flags c_ign_gt
[ML][NG], c_ign_dt [ML][ND], c_num_valid [ML], c_dc_num [ML][G], c_dc_boxes (all DontCare boxes, (class, difficulty) major, then frame), and
per metric m in (bbox2d, bev, box3d | nu): c_m_pr [C][S][7], c_m_thr [C][S], c_m_nthr [C], c_m_scores with c_m_scores_off [C + 1] (pass A,
frame order).  Combination c = (class * L + difficulty) * 2 + level.
"""
import os

import numpy as np

from tests import _eval_ref as E

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g17_detection_eval.npz")
METRIC_NAMES = ("bbox2d", "bev", "box3d", "nu")
ANNO_KEYS = ("truncated", "occluded", "alpha", "bbox", "dimensions", "location", "rotation_y", "score")
_CACHE = {}


def load():
    if "d" not in _CACHE:
        with np.load(PATH) as z:
            _CACHE["d"] = {k: z[k] for k in z.files}
    return _CACHE["d"]


def configs(d):
    return [str(c) for c in d["configs"]]


def metrics_of(d, cfg):
    return (0, 1, 3 if int(d[cfg + "_nuscenes"]) else 2)


def annos(d, scene, side, names_as="list"):
    """the scene's annotation dicts of one side ("gt" / "dt"), one per frame"""
    num = d["%s_%s_num" % (scene, side)]
    off = np.concatenate([[0], np.cumsum(num)])
    out = []
    for f in range(len(num)):
        a, b = off[f], off[f + 1]
        names = d["%s_%s_name" % (scene, side)][a:b]
        an = dict(name=[str(n) for n in names] if names_as == "list" else np.array(names))
        for k in ANNO_KEYS:
            an[k] = d["%s_%s_%s" % (scene, side, k)][a:b].copy()
        out.append(an)
    return out


def frames(d, scene):
    p = scene + "_"
    return E.Frames(d[p + "gt_num"], d[p + "dt_num"], d[p + "dt_score"], d[p + "gt_rotation_y"], d[p + "dt_rotation_y"], d[p + "gt_alpha"],
                    d[p + "dt_alpha"], d[p + "dt_bbox"])


def id_to_name(d):
    return {int(i): str(n) for i, n in zip(d["id_to_name_ids"], d["id_to_name_names"])}


def overlaps(d, cfg, metric):
    return d["ov_%s_%d_%s" % (str(d[cfg + "_scene"]), int(d[cfg + "_frame"]), METRIC_NAMES[metric])].astype(np.float64)


def level_thresholds(d, cfg, metric):
    """min_overlap [C] of a configuration's metric, as eval_metric derives it: minus the distance threshold for the distance metric"""
    name_to_id = {v: k for k, v in id_to_name(d).items()}
    ids = [name_to_id[str(c)] for c in d[cfg + "_classes"]]
    tab = -1.0 * d["dist_thresholds"][metric][:, :, ids] if metric == 3 else d["overlap_thresholds"][metric][:, :, ids]
    L = len(d[cfg + "_difficulties"])
    return np.array([tab[k, l, m] for m in range(len(ids)) for l in range(L) for k in range(tab.shape[0])], np.float64)


def dc_offsets(d, cfg):
    """dc_off [ML][G + 1] into c_dc_boxes"""
    num = d[cfg + "_dc_num"].astype(np.int64)
    flat = np.concatenate([[0], np.cumsum(num.reshape(-1))])
    ML, G = num.shape
    return np.stack([flat[ml * G:ml * G + G + 1] for ml in range(ML)]) if ML else np.zeros((0, G + 1), np.int64)


def combination_inputs(d, cfg, metric, c):
    """keyword arguments of _eval_ref.combination for combination c of a metric"""
    ml = c // 2
    ang = bool(int(d[cfg + "_angular"])) and metric in (2, 3)
    kw = dict(ov_flat=overlaps(d, cfg, metric), ign_gt=d[cfg + "_ign_gt"][ml], ign_dt=d[cfg + "_ign_dt"][ml],
              num_valid_gt=int(d[cfg + "_num_valid"][ml]), min_overlap=level_thresholds(d, cfg, metric)[c],
              sample_points=int(d[cfg + "_sample_points"]), angular=ang)
    if metric == 0:
        kw.update(dc_boxes=d[cfg + "_dc_boxes"], dc_off=dc_offsets(d, cfg)[ml])
    return kw


def golden_conditions(d):
    """raises AssertionError unless the golden can tell a wrong implementation from a right one"""
    assert int(d["bev_overruns"]) == 0 and int(d["bev_pairs"]) > 10000
    for s in ("kitti", "ones", "big"):
        sc = d[s + "_dt_score"]
        assert len(sc) and np.isfinite(sc).all() and (sc > 0).all() and (sc <= 1).all()
    assert len(set(d["kitti_dt_score"].tolist())) < len(d["kitti_dt_score"])          # ties
    assert (d["ones_dt_score"] == 1).all()
    assert d["big_gt_num"].max() > 64 and d["big_dt_num"].max() > 64
    assert d["kitti_gt_num"].min() == 0 and d["kitti_dt_num"].min() == 0 and ((d["kitti_gt_num"] == 0) & (d["kitti_dt_num"] == 0)).any()
    assert len(d["kitti_gt_num"]) == 57 and d["empty_gt_num"].sum() == 0 and d["empty_dt_num"].sum() == 0
    for cfg, metric in (("kitti_cam_kitti", 0), ("kitti_cam_kitti", 1), ("kitti_cam_kitti", 2), ("kitti_cam_nu", 3), ("kitti_lidar_nu", 3)):
        pr = d["%s_%s_pr" % (cfg, METRIC_NAMES[metric])]
        assert ((pr[:, :, 0] > 0) & (pr[:, :, 1] > 0) & (pr[:, :, 2] > 0)).any(axis=1).any(), (cfg, metric)
    # the DontCare rule removes a false positive, and pass A / pass B choose different detections for some ground truth
    cfg = "kitti_cam_kitti"
    fr = frames(d, "kitti")
    removed = differ = 0
    for metric in (0, 2):
        for c in range(len(d["%s_%s_nthr" % (cfg, METRIC_NAMES[metric])])):
            kw = combination_inputs(d, cfg, metric, c)
            n = int(d["%s_%s_nthr" % (cfg, METRIC_NAMES[metric])][c])
            if n == 0:
                continue
            th = d["%s_%s_thr" % (cfg, METRIC_NAMES[metric])][c][n - 1]
            for f in range(len(fr)):
                g0, g1, d0, d1 = fr.goff[f], fr.goff[f + 1], fr.doff[f], fr.doff[f + 1]
                ov = kw["ov_flat"][fr.ooff[f]:fr.ooff[f + 1]].reshape(d1 - d0, g1 - g0)
                extra = {}
                if metric == 0:
                    off = kw["dc_off"]
                    extra = dict(dt_bbox=fr.dt_bbox[d0:d1], dc=kw["dc_boxes"][off[f]:off[f + 1]])
                a = E.match_frame(ov, fr.dt_score[d0:d1], kw["ign_gt"][g0:g1], kw["ign_dt"][d0:d1], kw["min_overlap"])
                b = E.match_frame(ov, fr.dt_score[d0:d1], kw["ign_gt"][g0:g1], kw["ign_dt"][d0:d1], kw["min_overlap"], th, True, **extra)
                removed += b["removed"]
                da, db = dict(a["assign"]), dict(b["assign"])
                differ += sum(1 for g in da if g in db and da[g] != db[g])
    assert removed > 0, "no frame where the DontCare rule removes a false positive"
    assert differ > 0, "pass A (highest score) and pass B (highest overlap) never disagree"
    changed = any(not np.array_equal(d["kitti_cam_kitti_res_" + k], d["ones_cam_kitti_res_" + k], equal_nan=True)
                  for k in ("Box2DAP", "BevAP", "Box3DAP"))
    assert changed, "scores of 1 change no AP value"
    return dict(removed=removed, differ=differ)
