"""PoseEstimator -- drop-in for the reference's utils/pose.py PoseEstimator (types 'kabsch' and 'procrustes'), computed on the device by
sdflabel_amd.pose.ransac_pose.  A caller changes one import line:

    from sdflabel_amd.pipelines.pose import PoseEstimator      # was: from utils.pose import PoseEstimator

`estimate` / `init_pose_3d` draw their hypotheses with np.random.choice exactly as the reference does (the caller's global legacy RNG is
consumed identically, so a script seeded like refine_css.py gets the reference's hypotheses) and return the same dict: 'scale', 'rot'
(float32 [3][3]), 'tra' (float32 [3]), or None.  `estimate_many` runs a frame's annotations in one launch sequence; the host waits for
the device once, when it reads the results (the inputs go up through pinned buffers with asynchronous copies).

Differences from the reference, all deliberate:
  - the caller's model array is not scaled in place ('kabsch' scales a copy, in the model's dtype, as the reference's `*=` does);
  - where the reference's final `procrustes` returns None (a rank-deficient inlier set) and it crashes with a TypeError (utils/pose.py:212),
    the result is None;
  - 'pnp' (cv2.solvePnPRansac, init_pose_2d) is not ported and raises NotImplementedError.
"""
import numpy as np
import torch

from ..pose import MIN_NUM_INLIERS, ransac_iterations, ransac_pose, sample_indices_numpy  # noqa: F401

_PNP = ("PoseEstimator type 'pnp' (init_pose_2d: cv2.solvePnPRansac on the NOCS image, utils/pose.py:43-83) is not ported; "
        "use 'kabsch' or 'procrustes'")


def _n_points(a):
    return int(a.shape[0])


def _draw_numpy(n, T):
    """the reference's draws for one annotation (utils/pose.py:146): T calls of np.random.choice on the global legacy RNG"""
    return np.stack([np.random.choice(range(n), 4, replace=False) for _ in range(T)]).astype(np.int32)


def _device_of(*arrays):
    for a in arrays:
        if torch.is_tensor(a) and a.is_cuda:
            return a.device
    return torch.device("cuda", torch.cuda.current_device())


def _results(out, type, scale_model, B):
    """one device -> host copy of the frame's results (packed as int32: the flag is never read through a float), then the reference's dicts"""
    packed = torch.cat([out["found"], out["scale"].view(torch.int32), out["rot"].reshape(B * 9).view(torch.int32),
                        out["tra"].reshape(B * 3).view(torch.int32)]).cpu().numpy()
    found = packed[:B]
    scale = packed[B:2 * B].view(np.float32)
    rot = packed[2 * B:11 * B].view(np.float32).reshape(B, 3, 3)
    tra = packed[11 * B:14 * B].view(np.float32).reshape(B, 3)
    res = []
    for b in range(B):
        if not found[b]:
            res.append(None)
            continue
        s = scale_model if type == "kabsch" else np.float32(scale[b])
        res.append({"scale": s, "rot": np.array(rot[b], dtype=np.float32), "tra": np.array(tra[b], dtype=np.float32)})
    return res


class PoseEstimator:
    """utils/pose.py PoseEstimator(type='kabsch', scale=2.2) on the device"""

    def __init__(self, type='kabsch', scale=2.2):
        self.scale = scale
        self.type = type

    def estimate(self, pcd_dsdf, nocs_dsdf, pcd_scene, nocs_scene, off_intrinsics=None, nocs_pred_resized=None):
        """the reference's estimate (utils/pose.py:13-38): init_pose_3d with type=self.type, scale_model=self.scale"""
        if self.type in ('kabsch', 'procrustes'):
            return self.init_pose_3d(pcd_dsdf, nocs_dsdf, pcd_scene, nocs_scene, type=self.type, scale_model=self.scale)
        if self.type == 'pnp':
            raise NotImplementedError(_PNP)
        return None                    # the reference leaves init_pose unbound for an unknown type

    @staticmethod
    def init_pose_2d(cam, nocs_region, scale_model=1):
        raise NotImplementedError(_PNP)

    @staticmethod
    def init_pose_3d(model_pts, model_cls, scene_pts, scene_cls, metric_distance_threshold=0.15, nocs_distance_threshold=0.15,
                     type='procrustes', scale_model=1):
        """utils/pose.py:85-233 on the device.  Returns {'scale', 'rot', 'tra'} or None (fewer than 5 scene points, fewer than 5 best
        inliers, or -- where the reference raises a TypeError -- a rank-deficient final procrustes)."""
        if type not in ('kabsch', 'procrustes'):
            raise NotImplementedError(_PNP if type == 'pnp' else "init_pose_3d: unknown type %r" % (type,))
        n = _n_points(scene_pts)
        if n < 5:
            return None
        T = ransac_iterations()
        idx = _draw_numpy(n, T)
        out = ransac_pose([model_pts], [model_cls], [scene_pts], [scene_cls], type=type, scale_model=scale_model, idx=[idx],
                          metric_distance_threshold=metric_distance_threshold, nocs_distance_threshold=nocs_distance_threshold,
                          device=_device_of(model_pts, scene_pts))
        return _results(out, type, scale_model, 1)[0]

    def estimate_many(self, items, sampler='device', seed=0, keys=None, return_raw=False):
        """A frame's annotations in one launch sequence; the host waits for the device once, to read the results.

        items: list of (pcd_dsdf, nocs_dsdf, pcd_scene, nocs_scene[, ...]) per annotation (extra entries, e.g. the PnP inputs, are ignored).
        sampler: 'device' -- counter-based hash of (seed, keys[i], hypothesis), keys default to the annotation's position; 'numpy' -- the
        reference's np.random.choice draws annotation after annotation (the same global RNG stream as calling `estimate` in a loop).
        Returns a list of dicts or None (and the raw device results with return_raw=True)."""
        if self.type == 'pnp':
            raise NotImplementedError(_PNP)
        if not items:
            return ([], None) if return_raw else []
        T = ransac_iterations()
        idx = None
        if sampler == 'numpy':
            idx = [_draw_numpy(_n_points(it[2]), T) if _n_points(it[2]) >= 5 else None for it in items]
        elif sampler != 'device':
            raise ValueError("estimate_many: sampler must be 'device' or 'numpy'")
        out = ransac_pose([it[0] for it in items], [it[1] for it in items], [it[2] for it in items], [it[3] for it in items], type=self.type,
                          scale_model=self.scale, sampler=sampler, seed=seed, keys=keys, idx=idx,
                          device=_device_of(*[x for it in items for x in it[:4]]))
        res = _results(out, self.type, self.scale, len(items))
        return (res, out) if return_raw else res
