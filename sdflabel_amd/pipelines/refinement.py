"""The frame-loop helpers of the reference's utils/refinement.py, computed on the device where they touch points.  A caller changes one
import line:

    from sdflabel_amd.pipelines import refinement as rtools      # was: import utils.refinement as rtools

Ported: reproject, get_kitti_label, roty_in_bev, alpha_in_bev, compute_iou, get_iou, adjust_intrinsics_crop, rot_from_yaw -- same
signatures, same return values.  The dataset, visualisation and cv2 helpers of that module (transform_bgr_crop, compute_depth_map, project,
the open3d line sets, ...) are not ported, which is why there is no module of that name under compat/: it would shadow them.

Differences from the reference, all deliberate:
  - reproject of numpy inputs runs on the device in float32 like the torch branch and returns float32 numpy arrays (the reference's numpy
    branch computes in float64; the optimiser casts that cloud to float32, optimizer.py:64); `filter` works for both kinds of input;
  - get_kitti_label returns `scaled_points` as a numpy array, fetched from the device on return (labels_many keeps it there).
A frame's annotations are better served by sdflabel_amd.frame (reproject_many, init_params_many, labels_many): one launch sequence and one
synchronisation per stage instead of one per annotation.
"""
import numpy as np
import torch

from ..frame import (adjust_intrinsics_crop, alpha_in_bev, compute_iou, get_iou, labels_many, reproject_many, rot_from_yaw,  # noqa: F401
                     roty_in_bev)


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
