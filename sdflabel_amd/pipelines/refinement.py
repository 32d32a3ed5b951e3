"""The frame-loop helpers of the reference's utils/refinement.py, computed on the device where they touch points.  A caller changes one
import line:

    from sdflabel_amd.pipelines import refinement as rtools      # was: import utils.refinement as rtools

Ported: reproject, get_kitti_label, roty_in_bev, alpha_in_bev, compute_iou, get_iou, adjust_intrinsics_crop, rot_from_yaw, compute_depth_map,
build_view_frustum, build_cam_frustum, unproject, transform_bgr_crop, get_annos, is_anno_easy / _moderate / _hard -- same signatures, same
return values -- and get_kitti_frame, whose differences are listed below.  The remaining dataset, visualisation and cv2 helpers of that
module (project, the open3d line sets, ...) are not ported, which is why there is no module of that name under compat/: it would shadow them.

Differences from the reference, all deliberate:
  - reproject of numpy inputs runs on the device in float32 like the torch branch and returns float32 numpy arrays (the reference's numpy
    branch computes in float64; the optimiser casts that cloud to float32, optimizer.py:64); `filter` works for both kinds of input;
  - get_kitti_label returns `scaled_points` as a numpy array, fetched from the device on return (labels_many keeps it there);
  - compute_depth_map drops a point that float32 rounding puts at x == w or y == h, where the reference raises IndexError;
  - transform_bgr_crop needs neither cv2, PIL nor torchvision: PIL's 8-bit bilinear resize is reproduced byte for byte on the device; it
    returns CPU tensors, as the reference does, and does not modify crop_bgr;
  - get_kitti_frame needs no open3d: the normals of its road-plane removal follow frame.lidar_normals' own statement of Open3D's hybrid
    search and covariance normals (Open3D is not installed where this was developed: parity with it is untested); it returns the depth map
    as a device tensor and a ScenePoints object in the o3d.geometry.PointCloud's place;
  - cv2.undistortPoints / cv2.projectPoints are taken to be the plain pinhole (cv2 is not installed where this was developed: untested).
A frame's annotations are better served by sdflabel_amd.frame (reproject_many, init_params_many, labels_many, css_inputs_many): one launch
sequence and one synchronisation per stage instead of one per annotation; pipelines.frame.refine_sample is the whole loop for a sample.
"""
import numpy as np
import torch

from ..frame import (adjust_intrinsics_crop, alpha_in_bev, build_cam_frustum, build_view_frustum, compute_iou, css_inputs_many,  # noqa: F401
                     depth_map, get_iou, kitti_frame, labels_many, reproject_many, rot_from_yaw, roty_in_bev, unproject)


def is_anno_easy(anno):
    """utils/refinement.py:15-27: KITTI difficulty "easy" -- not occluded, truncated at most 0.15, box at least 40 pixels high"""
    height = anno['bbox'][3] - anno['bbox'][1]
    return not ((anno['occluded'] > 0) or (anno['truncated'] > 0.15) or height < 40)


def is_anno_moderate(anno):
    """utils/refinement.py:30-42: "moderate" -- occluded at most 1, truncated at most 0.30, box at least 25 pixels high"""
    height = anno['bbox'][3] - anno['bbox'][1]
    return not ((anno['occluded'] > 1) or (anno['truncated'] > 0.30) or height < 25)


def is_anno_hard(anno):
    """utils/refinement.py:45-57: "hard" -- occluded at most 2, truncated at most 0.5, box at least 25 pixels high"""
    height = anno['bbox'][3] - anno['bbox'][1]
    return not ((anno['occluded'] > 2) or (anno['truncated'] > 0.5) or height < 25)


def get_annos(diff_annos, sample):
    """utils/refinement.py:565-583: the sample's annotations up to a difficulty ('hard': all three lists, 'medium': easy + medium, anything
    else: easy), sorted by ascending depth (a stable sort, as sorted is)"""
    if diff_annos == 'hard':
        annos = sample['annos']['easy'] + sample['annos']['medium'] + sample['annos']['hard']
    elif diff_annos == 'medium':
        annos = sample['annos']['easy'] + sample['annos']['medium']
    else:
        annos = sample['annos']['easy']
    return sorted(annos, key=lambda i: i['location'][2])


def compute_depth_map(lidar, cam, w, h):
    """utils/refinement.py:87-105: the sparse depth image (h, w) float32 of the lidar points inside the camera's frustum, as a numpy array
    (frame.depth_map keeps it on the device)"""
    return depth_map(lidar, cam, w, h).cpu().numpy()


def transform_bgr_crop(crop_bgr, orig=False):
    """utils/refinement.py:60-84: a BGR crop (H, W, 3) in 0 ... 1 as the CSS network's input, a (3, 128, 128) float32 CPU tensor (with orig:
    and the same image before Normalize).  The one-crop call of frame.css_inputs_many."""
    H, W = int(crop_bgr.shape[0]), int(crop_bgr.shape[1])
    out = css_inputs_many(crop_bgr, [[0, 0, W, H]], orig=orig)
    return (out[0][0].cpu(), out[1][0].cpu()) if orig else out[0].cpu()


def reproject(color, depth, K, flip_color_channels=False, filter=False):
    """utils/refinement.py:360-410: the non-zero pixels of a depth map as 3-D points (N, 3) with their colours (N, 3), in row-major pixel
    order; filter=True keeps only the points with some colour channel > 0 (the foreground of a NOCS image)."""
    as_numpy = not torch.is_tensor(depth)
    (points, colors), = reproject_many([color], [depth], [K], filter=filter)
    if flip_color_channels:
        colors = torch.stack((colors[:, 2], colors[:, 1], colors[:, 0]), 1)
    if as_numpy:
        return points.cpu().numpy(), colors.cpu().numpy()
    return points, colors


def get_kitti_label(dsdf, grid, latent, scale, trans, yaw, p_WC, bbox):
    """utils/refinement.py:501-562: the KITTI label of one annotation's refined parameters.  Returns (label, scaled_points, cam_T).  The
    latent is passed to the decoder as it is, un-normalised, as the reference does (:536).  An empty band raises ValueError, as the
    reference's min() of an empty array does."""
    res, = labels_many(dsdf, grid, [{'latent': latent, 'scale': scale, 'trans': trans, 'yaw': yaw}], p_WC, [bbox])
    if res is None:
        raise ValueError("get_kitti_label: no grid point within the band of the zero level set (zero-size array to reduction operation)")
    label, scaled_points, cam_T = res
    return label, np.asarray(scaled_points), cam_T


class ScenePoints:
    """What get_kitti_frame returns in the o3d.geometry.PointCloud's place: `.points` and `.colors`, each converting with np.asarray to the
    float64 [n][3] array open3d's Vector3dVector would hold (float32 values, widened).  The data stays on the device until one of them is
    converted -- the read of the point count is the one host synchronisation, made then and not before; `.device()` gives the (points,
    colors) float32 device tensors.  No open3d methods (normals, visualisation) are offered."""

    class _Lazy:
        def __init__(self, owner, k):
            self._owner, self._k = owner, k

        def __array__(self, dtype=None, copy=None):
            a = self._owner._fetch()[self._k]
            return a if dtype is None else a.astype(dtype)

        def __len__(self):
            return len(self._owner._fetch()[self._k])

    def __init__(self, points, colors, count):
        self._p, self._c, self._n, self._host = points, colors, count, None
        self.points, self.colors = ScenePoints._Lazy(self, 0), ScenePoints._Lazy(self, 1)

    def device(self):
        n = int(self._n)
        return self._p[:n], self._c[:n]

    def _fetch(self):
        if self._host is None:
            p, c = self.device()
            self._host = (p.cpu().numpy().astype(np.float64), c.cpu().numpy().astype(np.float64))
        return self._host


def get_kitti_frame(sample):
    """utils/refinement.py:612-656: (scene_depth, pcd) of a loaded KITTI sample {'image' (H, W, 3), 'lidar' [N][3] in the camera frame,
    'orig_cam' 3x3}: the lidar cut to the image frustum, the road plane removed by the normal test |n_y| > 0.9, the rest rasterised into the
    sparse depth map, and the coloured scene points reprojected from it -- frame.kitti_frame, no host synchronisation.
    Differences from the reference: scene_depth is a float32 device tensor (H, W) where the reference returns a numpy array (.cpu().numpy()
    gives it); pcd is a ScenePoints, not an o3d.geometry.PointCloud: `.points` and `.colors` convert with np.asarray, nothing else of open3d's
    class is offered.  The normals are frame.lidar_normals' -- written from Open3D's algorithm, parity with Open3D untested.  The reference's
    plane_normal / plane_offset are computed there but never used, so they are not provided.  Parsing the KITTI3D files into the sample
    (datasets/kitti.py) stays with the caller."""
    depth, pts, clrs, info = kitti_frame(sample['image'], sample['lidar'], sample['orig_cam'], return_info=True)
    return depth, ScenePoints(pts, clrs, info["count"])
