"""pipelines/detection_3d.py of the reference (numba CPU JIT + scipy there) on sdflabel_amd.detection_eval: the same public names,
constructor arguments and results; the match degrees, the matching, the thresholds and the PR accumulation run on the device.

Imports neither numba, scipy nor mpi4py.  No GPU: SdfrError, there is no CPU fallback.

Differences that change no result: `eval_metric` keeps `num_shards` and ignores it (sharding only bounds the reference's matrix sizes);
the two shipped filters are recognised by identity and computed vectorised over the packed annotations, any other `filter_data_fn` is
called per frame exactly as the reference calls it.  The default threshold tables and the KITTI ontology are data of the reference's
pipelines/constants.py: they are looked up there when that module is importable, otherwise the caller passes `id_to_name`,
`per_class_iou_overlap_thresholds` and `per_class_dist_thresholds`.
"""
from enum import IntEnum

import numpy as np
import torch

from sdflabel_amd import detection_eval as _e
from sdflabel_amd.detection_eval import clean_kitti_data, difficulty_by_distance  # noqa: F401  (public names of the reference's module)


class Metrics(IntEnum):
    """BBOX_2D_AP: image boxes; BEV_3D_AP: bird's eye view boxes; BBOX_3D_KITTI_AP: 3-D IoU; BBOX_3D_NU_AP: centre distance"""
    BBOX_2D_AP = 0
    BEV_3D_AP = 1
    BBOX_3D_KITTI_AP = 2
    BBOX_3D_NU_AP = 3


class CoordinateFrame(IntEnum):
    """CAMERA: x left, y down, z front; LIDAR / VEHICLE: z up"""
    LIDAR = 0
    VEHICLE = 1
    CAMERA = 2


_DEFAULT = object()


def _constant(name, what):
    try:
        from pipelines import constants
    except ImportError:
        raise ValueError("%s: no default here (the reference's pipelines.constants is not importable); pass it to Detection3DEvaluator" % what)
    return getattr(constants, name)


def angle_diff(x, y, period):
    """signed smallest difference between two angles, from y to x"""
    diff = (x - y + period / 2) % period - period / 2
    if diff > np.pi:
        diff = diff - (2 * np.pi)
    return diff


def get_thresholds(scores, num_gt, num_sample_pts=41):
    """score thresholds of a PR curve of a score array (sdfr_eval_thresholds: sort and recall walk on the device): a list"""
    import torch
    dev = _e._device(None)
    lib, p = _e._lib, _e._lib.ptr
    s = torch.as_tensor(np.asarray(scores, np.float64).reshape(-1)).to(dev).contiguous()
    n, S = int(s.numel()), int(num_sample_pts)
    ws_bytes = int(lib.lib().sdfr_eval_ws_bytes(0, n, 1, S, 0, 0))
    ws = torch.empty((ws_bytes + 7) // 8, dtype=torch.int64, device=dev)
    thr = torch.empty((1, S), dtype=torch.float64, device=dev)
    nthr = torch.empty((1,), dtype=torch.int32, device=dev)
    num = torch.full((1,), int(num_gt), dtype=torch.int64, device=dev)
    with lib.guard(thr):
        lib.check(lib.lib().sdfr_eval_thresholds(p(s), n, p(num), 1, 1, S, p(ws), ws_bytes, p(thr), p(nthr), None, lib.stream_ptr()),
                  "sdfr_eval_thresholds")
    return thr[0, :int(nthr.item())].cpu().tolist()


class Detection3DEvaluator:
    """3-D detection evaluation in the KITTI annotation format: 2-D box AP, BEV AP, 3-D AP (IoU or centre distance), orientation error and
    similarity.  Arguments as in the reference: filter_data_fn (a callable with the signature of clean_kitti_data), id_to_name,
    per_class_iou_overlap_thresholds / per_class_dist_thresholds [metric][level][difficulty][class], coordinate_frame,
    compute_angular_metrics, compute_nuscenes, sample_points, sampling_frequency."""

    def __init__(self, filter_data_fn, id_to_name=_DEFAULT, per_class_iou_overlap_thresholds=_DEFAULT, per_class_dist_thresholds=_DEFAULT,
                 coordinate_frame=CoordinateFrame.LIDAR, compute_angular_metrics=True, compute_nuscenes=True, sample_points=41,
                 sampling_frequency=1):
        self.filter_data_fn = filter_data_fn
        self.sample_points = sample_points
        self.compute_angular_metrics = compute_angular_metrics
        self.coordinate_frame = coordinate_frame
        self.compute_nuscenes = compute_nuscenes
        self.sampling_frequency = sampling_frequency
        self.id_to_name = _constant("KITTI_CLASS_NAMES", "id_to_name") if id_to_name is _DEFAULT else id_to_name
        self.name_to_id = {v: n for n, v in self.id_to_name.items()}
        self.overlap_thresholds = _constant("KITTI_OVERLAP_THRESHOLDS", "per_class_iou_overlap_thresholds") \
            if per_class_iou_overlap_thresholds is _DEFAULT else per_class_iou_overlap_thresholds
        if per_class_dist_thresholds is _DEFAULT:
            try:
                per_class_dist_thresholds = _constant("NU_OVERLAP_THRESHOLDS", "per_class_dist_thresholds")
            except ValueError:
                if compute_nuscenes:
                    raise
                per_class_dist_thresholds = None
        self.dist_thresholds = per_class_dist_thresholds
        self._session = None
        self._keep = False          # True inside evaluate_detection_3d: its metrics share one packed, uploaded dataset

    # -- the packed dataset of the current call ----------------------------------------------------------------------------------------------
    def _open(self, gt_annos, dt_annos):
        """pack and upload; once for all metrics of an evaluate_detection_3d call, afresh for every direct call of eval_metric or
        calculate_match_degree_sharded (the caller may have changed the lists in between)"""
        s = self._session if self._keep else None
        if s is None or s[0] is not gt_annos or s[1] is not dt_annos:
            packed = _e.pack(gt_annos, dt_annos)
            s = (gt_annos, dt_annos, _e.Session(packed, int(self.coordinate_frame)), {})
            self._session = s if self._keep else None
        return s[2], s[3]

    def _flags(self, gt_annos, dt_annos, classes_for_eval, difficulties):
        session, cache = self._open(gt_annos, dt_annos)
        key = (tuple(classes_for_eval), tuple(difficulties), id(self.filter_data_fn))
        if key not in cache:
            names = [self.id_to_name[c] for c in classes_for_eval]
            if self.filter_data_fn is clean_kitti_data:
                f = _e.clean_kitti_flags(session.P, names, list(difficulties))
            elif self.filter_data_fn is difficulty_by_distance:
                f = _e.distance_flags(session.P, names, list(difficulties), int(self.coordinate_frame))
            else:
                f = _e.callable_flags(self.filter_data_fn, gt_annos, dt_annos, list(classes_for_eval), list(difficulties), self.id_to_name,
                                      self.coordinate_frame)
            cache[key] = (f, session.flags(f))
        return session, cache[key]

    # -- public interface ---------------------------------------------------------------------------------------------------------------------
    def evaluate_detection_3d(self, gt_annos, dt_annos, classes_for_eval=None, difficulties=(0, )):
        """-> (formatted_result, result_dict) as the reference"""
        assert max(difficulties) <= self.overlap_thresholds.shape[2], \
            "difficuty index shall be smaller than {} but get {}.".format(self.overlap_thresholds.shape[2], max(difficulties))
        if self.compute_nuscenes:
            assert max(difficulties) <= self.dist_thresholds.shape[2], \
                "difficuty index shall be smaller than {} but get {}.".format(self.dist_thresholds.shape[2], max(difficulties))
        self.validate_anno_format(gt_annos, dt_annos)
        assert isinstance(classes_for_eval, (list, tuple)), "Please list of class names for evaluation"
        ids = []
        for name in classes_for_eval:
            if name not in self.name_to_id:
                raise KeyError("{} is not a valid class to evaluate in the given ontology".format(name))
            ids.append(self.name_to_id[name])
        if self.compute_angular_metrics:
            for anno in dt_annos:
                assert 'rotation_y' in anno
                assert 'alpha' in anno
        dist_thresholds = self.dist_thresholds[:, :, :, ids] if self.compute_nuscenes else None
        overlap_thresholds = self.overlap_thresholds[:, :, :, ids]
        self._keep = True
        try:
            r = self.do_eval(gt_annos, dt_annos, ids, difficulties, overlap_thresholds, dist_thresholds)
        finally:
            self._keep, self._session = False, None
        names = ["Box2DAP", "BevAP", "Box3DAP", "AoeAP_iou", "AoeAP_dist", "AosAP_iou", "AosAP_dist", "Box3DAP_Nu", "bbox_2d_pre_curves",
                 "bev_pre_curves", "bbox_3d_kitti_pre_curves", "bbox_3d_nu_pre_curves"]
        result_dict = {n: v for n, v in zip(names, r) if v is not None}
        text = _e.format_result(None, [self.id_to_name[c] for c in ids], difficulties, self.compute_nuscenes, self.compute_angular_metrics,
                                dist_thresholds if self.compute_nuscenes else overlap_thresholds, result_dict)
        return text, result_dict

    def validate_anno_format(self, gt_annos, dt_annos):
        necessary_keys = ['name', 'alpha', 'bbox', 'dimensions', 'location', 'rotation_y', 'score']
        for i, (gt_anno, dt_anno) in enumerate(zip(gt_annos, dt_annos)):
            for key in necessary_keys:
                assert key in gt_anno, "{} not present in GT {}".format(key, i)
                assert key in dt_anno, "{} not present in prediction {}".format(key, i)
                if key in ['bbox', 'dimensions', 'location']:
                    assert len(gt_anno[key].shape) == 2
                    assert len(dt_anno[key].shape) == 2

    def do_eval(self, gt_annos, dt_annos, classes_for_eval, difficulties, overlap_thresholds, dist_thresholds):
        """every metric on the given class ids -> (mAP_bbox, mAP_bev, mAP_3d, mAP_aoe_iou, mAP_aoe_dist, mAP_aos_iou, mAP_aos_dist, mAPnu_3d,
        bbox_2d_pr_curves, bev_pr_curves, bbox_3d_kitti_pr_curves, bbox_3d_nu_pr_curves); what is not computed is None.  All metrics are
        enqueued before the first table is read back."""
        ang = self.compute_angular_metrics
        metrics = [(Metrics.BBOX_2D_AP, False), (Metrics.BEV_3D_AP, False),
                   (Metrics.BBOX_3D_NU_AP if self.compute_nuscenes else Metrics.BBOX_3D_KITTI_AP, ang)]
        pending = [self._enqueue(gt_annos, dt_annos, classes_for_eval, difficulties, m, overlap_thresholds, dist_thresholds, a) for m, a in metrics]
        curves = [self._curves(p) for p in pending]
        aps = [self.get_mAP(c["precision"], c["recall"]) for c in curves]
        aoe = self.get_mAP(curves[2]["orientation_aoe"], curves[2]["recall"]) if ang else None
        aos = self.get_mAP(curves[2]["orientation_aos"], curves[2]["recall"]) if ang else None
        if self.compute_nuscenes:
            return aps[0], aps[1], None, None, aoe, None, aos, aps[2], curves[0], curves[1], None, curves[2]
        return aps[0], aps[1], aps[2], aoe, None, aos, None, None, curves[0], curves[1], curves[2], None

    def _enqueue(self, gt_annos, dt_annos, classes_for_eval, difficulties, metric, overlap_thresholds, dist_thresholds, compute_angular_metrics):
        assert len(gt_annos) == len(dt_annos), "Must provide a prediction for every ground truth sample"
        session, (flags, dflags) = self._flags(gt_annos, dt_annos, classes_for_eval, difficulties)
        table = dist_thresholds if metric == Metrics.BBOX_3D_NU_AP else overlap_thresholds
        M, L, K = len(classes_for_eval), len(difficulties), table.shape[1]
        stats = session.statistics(int(metric), dflags, M * L, K, _e.level_thresholds(table, int(metric), L), self.sample_points,
                                   bool(compute_angular_metrics))
        return stats, (M, L, K), metric == Metrics.BBOX_3D_NU_AP, bool(compute_angular_metrics)

    @staticmethod
    def _curves(pending):
        stats, shape, distance, ang = pending
        pr = stats["pr"]
        both = torch.cat([pr.reshape(-1), stats["nthr"].to(pr.dtype)]).cpu().numpy()          # one read-back: the call's only synchronisation
        return _e.finish(both[:pr.numel()].reshape(pr.shape), both[pr.numel():].astype(np.int32), shape, distance, ang)

    def eval_metric(self, gt_annos, dt_annos, classes_for_eval, difficulties, metric, overlap_thresholds, dist_thresholds,
                    compute_angular_metrics=False, num_shards=50):
        """one metric -> dict of curves recall, precision, orientation_aoe, orientation_aos, tp_mean_error, tp_mean_confidence_error, each
        [classes][difficulties][levels][sample_points].  num_shards is accepted and ignored: no result depends on it."""
        return self._curves(self._enqueue(gt_annos, dt_annos, classes_for_eval, difficulties, metric, overlap_thresholds, dist_thresholds,
                                          compute_angular_metrics))

    def calculate_match_degree_sharded(self, gt_annos, dt_annos, metric, num_shards):
        """-> (overlaps: list of [n_dt][n_gt] float64 arrays per frame, overlaps_by_shard: list of block matrices per shard (the pairs of
        different frames are zero here; the reference fills them with values nothing reads), total_gt_num, total_dt_num), numpy arrays"""
        session, _ = self._open(gt_annos, dt_annos)
        P = session.P
        flat = session.overlaps(int(metric)).to("cpu").numpy().astype(np.float64)
        overlaps = [flat[P.ooff[f]:P.ooff[f + 1]].reshape(int(P.dt.num[f]), int(P.gt.num[f])) for f in range(P.G)]
        by_shard, at = [], 0
        for n in self.get_shards(P.G, num_shards):
            m = np.zeros((int(P.dt.num[at:at + n].sum()), int(P.gt.num[at:at + n].sum())))
            r = c = 0
            for f in range(at, at + n):
                m[r:r + overlaps[f].shape[0], c:c + overlaps[f].shape[1]] = overlaps[f]
                r, c = r + overlaps[f].shape[0], c + overlaps[f].shape[1]
            by_shard.append(m)
            at += n
        return overlaps, by_shard, P.gt.num.copy(), P.dt.num.copy()

    def get_shards(self, num, num_shards):
        """num split into num_shards equal parts, the remainder in a last one"""
        assert num_shards > 0, "Invalid number of shards"
        each, rest = divmod(num, num_shards)
        full = [each] * (num_shards if each > 0 else 0)
        return full if rest == 0 else full + [rest]

    def bev_box_overlap(self, boxes, qboxes, criterion=-1):
        from sdflabel_amd import box_iou
        return box_iou.rotate_iou(boxes, qboxes, criterion).cpu().numpy()

    def box_3d_overlap(self, boxes, qboxes, criterion=-1):
        from sdflabel_amd import box_iou
        return box_iou.box3d_iou(boxes, qboxes, criterion, camera_frame=self.coordinate_frame == CoordinateFrame.CAMERA).cpu().numpy()

    def prepare_data(self, gt_annos, dt_annos, current_class, difficulty):
        """the reference's per-frame lists: (gt_data_list, dt_data_list, ignored_gts, ignored_dets, dontcares, ignores_per_sample,
        total_num_valid_gt)"""
        gt_list, dt_list, ignored_gts, ignored_dets, dontcares, per_sample = [], [], [], [], [], []
        total = 0
        for g, d in zip(gt_annos, dt_annos):
            n, ig, idt, boxes = self.filter_data_fn(g, d, current_class, difficulty, self.id_to_name, self.coordinate_frame)
            ignored_gts.append(np.array(ig, dtype=np.int64))
            ignored_dets.append(np.array(idt, dtype=np.int64))
            boxes = np.stack(boxes, 0).astype(np.float64) if len(boxes) else np.zeros((0, 4))
            per_sample.append(boxes.shape[0])
            dontcares.append(boxes)
            total += n
            gt_list.append(np.concatenate([g["bbox"], g["rotation_y"][..., np.newaxis], g["alpha"][..., np.newaxis]], 1))
            dt_list.append(np.concatenate([d["bbox"], d["rotation_y"][..., np.newaxis], d["alpha"][..., np.newaxis], d["score"][..., np.newaxis]], 1))
        return gt_list, dt_list, ignored_gts, ignored_dets, dontcares, np.array(per_sample, dtype=np.int64), total

    def get_mAP(self, precision, recall):
        return _e.mean_ap(precision, recall, self.sample_points)
