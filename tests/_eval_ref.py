"""Plain numpy / Python restatement of the evaluator's statistics (csrc/detection_eval.hip): pass A (true-positive scores), the recall walk
that picks the score thresholds, and pass B (the seven sums of a PR row).  The in-repo reference where the golden G17 has no entry, and
the check that G17's tables follow from G17's recorded overlaps and flags.

It sums in the order the definition sums: per frame the match degree and -log(score) one true positive after the other, the yaw error
and the orientation similarity with numpy's sum over an array of `fp` leading zeros followed by the terms, then frame after frame into
the row.  Hence the float columns are reproduced bit for bit, not only the integer ones.
"""
import math

import numpy as np

NO_DETECTION = -10000000
TWO_PI = 2 * np.pi


def py_angle_diff(x, y, period):
    """signed smallest difference x - y of two angles; Python's float % (result takes the divisor's sign)"""
    d = (x - y + period / 2) % period - period / 2
    if d > np.pi:
        d = d - (2 * np.pi)
    return d


def dc_overlap(box, dc):
    """intersection of an image box with a DontCare box divided by the BOX's area (0 where they do not overlap)"""
    iw = min(box[2], dc[2]) - max(box[0], dc[0])
    if iw > 0:
        ih = min(box[3], dc[3]) - max(box[1], dc[1])
        if ih > 0:
            return iw * ih / ((box[2] - box[0]) * (box[3] - box[1]))
    return 0.0


def match_frame(ov, dt_score, ign_gt, ign_dt, min_overlap, thresh=0.0, compute_fp=False, angular=False, gt_yaw=None, dt_yaw=None,
                gt_alpha=None, dt_alpha=None, dt_bbox=None, dc=None):
    """one greedy matching of a frame.  ov[j][i]: detection j against ground truth i (float64).  dc: DontCare boxes [n][4], or None when
    the metric has no DontCare rule.  Returns a dict: tp, fp, fn, yaw, sim, md, conf, scores (of the true positives, in ground-truth order),
    assign [(gt, det)] of every consumed detection, removed (false positives taken away by the DontCare rule)."""
    nd, ng = len(dt_score), len(ign_gt)
    assigned = [False] * nd
    gone = [bool(compute_fp and dt_score[j] < thresh) for j in range(nd)]
    tp = fp = fn = 0
    md = 0
    conf = 0
    scores, assign, dyaw, dalpha = [], [], [], []
    for i in range(ng):
        if ign_gt[i] == -1:
            continue
        det, valid, best, by_ignored = -1, NO_DETECTION, -100000, False
        for j in range(nd):
            if ign_dt[j] == -1 or assigned[j] or gone[j]:
                continue
            o = ov[j, i]
            if not o > min_overlap:
                continue
            if not compute_fp:
                if dt_score[j] > valid:
                    det, valid = j, dt_score[j]
            elif ign_dt[j] == 0:
                if o > best or by_ignored:
                    best, det, valid, by_ignored = o, j, 1, False
            elif valid == NO_DETECTION:         # ign_dt[j] == 1: only while nothing has been chosen
                det, valid, by_ignored = j, 1, True
        if valid == NO_DETECTION:
            if ign_gt[i] == 0:
                fn += 1
            continue
        assigned[det] = True
        assign.append((i, det))
        if ign_gt[i] == 1 or ign_dt[det] == 1:
            continue
        tp += 1
        md += abs(best)
        conf += -math.log(dt_score[det])
        scores.append(dt_score[det])
        if angular:
            dyaw.append(abs(py_angle_diff(float(gt_yaw[i]), float(dt_yaw[det]), TWO_PI)))
            dalpha.append(gt_alpha[i] - dt_alpha[det])
    yaw = sim = 0
    removed = 0
    if compute_fp:
        free = [j for j in range(nd) if not (assigned[j] or ign_dt[j] != 0 or gone[j])]
        fp = len(free)
        if dc is not None:
            for b in dc:
                for j in free:
                    if not assigned[j] and dc_overlap(dt_bbox[j], b) > min_overlap:
                        assigned[j] = True
                        removed += 1
        fp -= removed
        if angular and (tp > 0 or fp > 0):
            a = np.zeros((fp + len(dyaw),))
            b = np.zeros((fp + len(dyaw),))
            for n in range(len(dyaw)):
                a[fp + n] = dyaw[n]
                b[fp + n] = (1.0 + np.cos(np.float64(dalpha[n]))) / 2.0
            yaw, sim = np.sum(a), np.sum(b)
    return dict(tp=tp, fp=fp, fn=fn, yaw=yaw, sim=sim, md=md, conf=conf, scores=scores, assign=assign, removed=removed)


def recall_thresholds(scores, num_gt, num_sample_pts=41):
    """the score thresholds of a PR curve: scores sorted descending, one kept whenever the running recall target is nearer to this
    detection's recall than to the next one's; the target advances by repeated += 1 / (num_sample_pts - 1.0)"""
    s = np.sort(np.asarray(scores, np.float64))[::-1]
    cur = 0
    out = []
    n = len(s)
    for i in range(n):
        left = (i + 1) / num_gt
        right = (i + 2) / num_gt if i < n - 1 else left
        if i < n - 1 and (right - cur) < (cur - left):
            continue
        out.append(s[i])
        cur += 1 / (num_sample_pts - 1.0)
    return out


class Frames:
    """what the statistics need of a packed dataset: per-frame counts and the concatenated columns (numpy, host)"""

    def __init__(self, gt_num, dt_num, dt_score, gt_yaw=None, dt_yaw=None, gt_alpha=None, dt_alpha=None, dt_bbox=None):
        self.gt_num, self.dt_num = np.asarray(gt_num, np.int64), np.asarray(dt_num, np.int64)
        self.goff = np.concatenate([[0], np.cumsum(self.gt_num)])
        self.doff = np.concatenate([[0], np.cumsum(self.dt_num)])
        self.ooff = np.concatenate([[0], np.cumsum(self.gt_num * self.dt_num)])
        self.dt_score, self.gt_yaw, self.dt_yaw, self.gt_alpha, self.dt_alpha, self.dt_bbox = dt_score, gt_yaw, dt_yaw, gt_alpha, dt_alpha, dt_bbox

    def __len__(self):
        return len(self.gt_num)


def combination(fr, ov_flat, ign_gt, ign_dt, num_valid_gt, min_overlap, sample_points=41, angular=False, dc_boxes=None, dc_off=None):
    """pass A, thresholds and pass B of one (class, difficulty, level).  ov_flat: the frames' [nd][ng] blocks one after the other
    (float64); ign_gt / ign_dt: flags over all ground truths / detections; dc_boxes [n][4] with dc_off [G + 1], or None.
    Returns scores (pass A, frame order), thresholds, pr [len(thresholds)][7], and per frame the pass-A result."""
    G = len(fr)
    ov_flat = np.asarray(ov_flat, np.float64)
    views = []
    for f in range(G):
        g0, g1, d0, d1 = fr.goff[f], fr.goff[f + 1], fr.doff[f], fr.doff[f + 1]
        kw = dict(gt_yaw=fr.gt_yaw[g0:g1], dt_yaw=fr.dt_yaw[d0:d1], gt_alpha=fr.gt_alpha[g0:g1], dt_alpha=fr.dt_alpha[d0:d1]) if angular else {}
        if dc_boxes is not None:
            kw.update(dt_bbox=fr.dt_bbox[d0:d1], dc=dc_boxes[dc_off[f]:dc_off[f + 1]])
        views.append((ov_flat[fr.ooff[f]:fr.ooff[f + 1]].reshape(d1 - d0, g1 - g0), fr.dt_score[d0:d1], ign_gt[g0:g1], ign_dt[d0:d1], kw))
    scores, first = [], []
    for ov, sc, ig, idt, kw in views:
        r = match_frame(ov, sc, ig, idt, min_overlap)
        first.append(r)
        scores += r["scores"]
    thr = recall_thresholds(scores, num_valid_gt, sample_points)
    pr = np.zeros([len(thr), 7])
    for ov, sc, ig, idt, kw in views:
        for t, th in enumerate(thr):
            r = match_frame(ov, sc, ig, idt, min_overlap, th, True, angular, **kw)
            pr[t, 0] += r["tp"]
            pr[t, 1] += r["fp"]
            pr[t, 2] += r["fn"]
            pr[t, 5] += r["md"]
            pr[t, 6] += r["conf"]
            pr[t, 3] += r["yaw"]
            pr[t, 4] += r["sim"]
    return np.array(scores, np.float64), np.array(thr, np.float64), pr, first
