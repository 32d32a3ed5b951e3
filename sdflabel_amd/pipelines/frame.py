"""refine_frame -- the annotation loop of the reference's pipelines/refine_css.py:94-245 for one frame, every stage batched over the frame's
annotations.  It contains nothing but calls of the public stages, in the reference's order; composing them by hand gives the same bits.

    from sdflabel_amd.pipelines.frame import refine_frame

What stays with the caller (it needs the dataset, the CSS network or Mask R-CNN): loading the frame, matching boxes, cutting the crops and
running the CSS network on them.
"""
import torch
import torch.nn.functional as F

from ..frame import frame_dict, init_params_many, labels_many, reproject_many, surfaces_many
from .optimizer import optimize_many
from .pose import PoseEstimator
from .refinement import adjust_intrinsics_crop


def refine_frame(annotations, dsdf, grid, css_latents, K_orig, world_to_cam, iters, weights, pose_type='kabsch', scale=2.0, rendering_area=32,
                 sampler='device', seed=0, keys=None, optimize_kwargs=None, return_stages=False):
    """One frame from crops to the evaluator's dict.

    annotations: per annotation a dict with 'bbox' [l, t, r, b] (the crop's box in the image), 'color' (the crop of the image, (H, W, 3)),
    'depth' (the crop of the sparse depth map, (H, W)) and 'nocs_pred' (the CSS network's NOCS image of the crop, (3, h, w), values 0 ... 1).
    css_latents: per annotation the CSS network's latent.  K_orig: the camera's 3x3 intrinsics; world_to_cam: the 4x4 p_WC of the labels.
    iters, weights: the optimiser's iteration count and loss weights {'2d', '3d'}; pose_type, scale: PoseEstimator(type, scale);
    rendering_area: the config's rendering_area (crops are rendered at about rendering_area^2 pixels); sampler, seed, keys: the RANSAC
    draws of PoseEstimator.estimate_many; optimize_kwargs: further arguments of Optimizer.optimize_many.

    Stages: adjust_intrinsics_crop -> reproject_many (the lidar crop, filter=False; the NOCS image resized to the crop with
    nearest-neighbour interpolation, filter=True) -> the surface of the CSS latents -> estimate_many -> init_params_many -> optimize_many
    -> labels_many -> frame_dict.  Annotations without a RANSAC pose are dropped, as the reference `continue`s.
    Returns (frame_estimations, kept): the {key: ndarray} dict of the frame's labels and the indices of the annotations behind its rows
    (and, with return_stages, a dict of every stage's results)."""
    device = grid.points.device
    precision = grid.points.dtype
    n = len(annotations)
    sizes, intr, off = [], [], []
    for a in annotations:
        crop_size = torch.Tensor(tuple(a['depth'].shape[-2:]))
        s, k, o = adjust_intrinsics_crop(K_orig, crop_size, a['bbox'], rendering_area ** 2)
        sizes.append(s), intr.append(k), off.append(o)
    depths = [torch.as_tensor(a['depth']).float() for a in annotations]
    lidar = reproject_many([a['color'] for a in annotations], depths, off, filter=False)
    nocs = [torch.as_tensor(a['nocs_pred']).float() for a in annotations]
    resized = [F.interpolate(nocs[i].unsqueeze(0), size=tuple(depths[i].shape[-2:]), mode='nearest').squeeze(0) for i in range(n)]
    nocs3d = reproject_many(resized, depths, off, filter=True)
    surf = surfaces_many(dsdf, grid, css_latents)
    poses = PoseEstimator(pose_type, scale).estimate_many([(surf[i][0], surf[i][1], nocs3d[i][0], nocs3d[i][1]) for i in range(n)],
                                                           sampler=sampler, seed=seed, keys=keys)
    params = init_params_many(poses, [s[0] for s in surf], [p[0] for p in nocs3d], [a['bbox'] for a in annotations], K_orig, css_latents)
    kept = [i for i in range(n) if params[i] is not None]
    refined = optimize_many([(params[i], nocs[i], lidar[i][0].cpu().numpy(), intr[i].detach().to(device, precision), sizes[i]) for i in kept],
                            iters, dsdf, grid, device, weights, **(optimize_kwargs or {}))
    labels = labels_many(dsdf, grid, refined, world_to_cam, [annotations[i]['bbox'] for i in kept])
    est = frame_dict(labels)
    kept = [i for i, lab in zip(kept, labels) if lab is not None]
    if return_stages:
        return est, kept, {'crop_sizes': sizes, 'intrinsics': intr, 'off_intrinsics': off, 'lidar': lidar, 'nocs_3d': nocs3d, 'surfaces': surf,
                           'poses': poses, 'params': refined, 'labels': labels}
    return est, kept
