"""refine_frame -- the annotation loop of the reference's pipelines/refine_css.py:94-245 for one frame, every stage batched over the frame's
annotations.  It contains nothing but calls of the public stages, in the reference's order; composing them by hand gives the same bits.

    from sdflabel_amd.pipelines.frame import refine_frame

refine_frame starts from finished crops.  refine_sample starts from a loaded KITTI sample: it selects the annotations, builds the depth map
from the lidar if asked -- with remove_road=True from the raw scan, the road plane removed first as get_kitti_frame does --, matches the
detector's boxes, cuts the crops on the device, prepares the CSS network's input, runs the network once over all crops and hands the result
to refine_frame.  What stays with the caller: loading the frame (datasets/kitti.py) and the CSS network itself, which is any
torch.nn.Module passed in.
"""
from collections import defaultdict

import numpy as np
import torch
import torch.nn.functional as F

from .. import _lib
from ..frame import (NECESSARY_KEYS, _as_tensor, css_inputs_many, depth_map, frame_dict, init_params_many, labels_many, match_boxes,
                     reproject_many, road_free_depth_map, surfaces_many)
from ..export import crops_many
from ..mesh import meshes_many
from .. import verify as _verify
from ..complete import _latent_cosine, complete_many
from ..align import align_many
from ..verify import label_windows, verify_many
from .optimizer import optimize_many
from .pose import PoseEstimator
from .refinement import adjust_intrinsics_crop, get_annos


def _grown_size(boxes, margin):
    """an image (W, H) just large enough for the boxes grown by `margin`: nothing is clipped on the right / at the bottom"""
    far = label_windows(boxes, (1 << 30, 1 << 30), margin)[1]
    return max(1, int(far[:, 2].max())), max(1, int(far[:, 3].max()))


def _stage_options(who, return_stages, mesh_resolution, verify, crops):
    """(mesh_resolution, verify, crops) with False and None as None (off) and True as {}; a stage that is on needs return_stages"""
    out = []
    for name, what, v in (("mesh_resolution", "meshes", mesh_resolution), ("verify", "verdicts", verify), ("crops", "crops", crops)):
        v = None if v is None or v is False else ({} if v is True else v)
        if v is not None and not return_stages:
            raise ValueError("%s: %s needs return_stages=True (the %s are returned among the stages)" % (who, name, what))
        out.append(v)
    return out


def _stage_size(kw, boxes):
    """a stage's image (W, H), taken out of its keyword arguments: the explicit 'image_size', or just large enough for its grown boxes"""
    size = kw.pop('image_size', None)
    if size is None and boxes:
        size = _grown_size(boxes, kw.get('margin', 0.25))
    return size or (1, 1)


def refine_frame(annotations, dsdf, grid, css_latents, K_orig, world_to_cam, iters, weights, pose_type='kabsch', scale=2.0, rendering_area=32,
                 sampler='device', seed=0, keys=None, optimize_kwargs=None, return_stages=False, mesh_resolution=None, verify=None, crops=None,
                 complete=None, align=None):
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
    (and, with return_stages, a dict of every stage's results).
    mesh_resolution (needs return_stages=True): the stages gain 'meshes', one sdflabel_amd.mesh.Mesh per kept annotation in the camera frame
    (mesh.meshes_many at that lattice resolution, polished, then Mesh.to_camera with the label's own cam_T).  None: nothing changes.
    verify (needs return_stages=True): True, or a dict of verify.verify_many's keyword arguments.  The stages gain 'verify', one verdict
    dict per kept annotation: the refined shape -- meshed at mesh_resolution, or at 64 when that is None -- is rendered into the
    annotation's box and compared with it, and the annotation's lidar cloud (stages['lidar'][i][0]) is counted in the band round the
    surface.  The dict may also hold 'image_size' (W, H), to which the windows are clipped -- without it the image is taken just large
    enough for the grown boxes -- and 'label_masks', one per ANNOTATION (of its box's shape, or None).  Nothing is filtered: est and kept
    are the bits of the call without verify, and the caller decides what to drop.  One more host read.  None: nothing changes.
    crops (needs return_stages=True): True, or a dict of export.crops_many's keyword arguments (and 'image_size', as for verify).  The stages
    gain 'crops', one export.Crop per kept annotation: the NOCS bytes of the refined shape -- the same meshes as verify's, at
    mesh_resolution, or at 64 when that is None -- in the annotation's box, the annotations occluding each other, and the RGB bytes of the
    annotation's 'color' crop.  Each crop also carries what a CropWriter entry needs: `.latent` (the raw refined latent), `.intrinsics` (the
    frame's K) and `.extrinsics` (the label's cam_T); pipelines.export_crops.export_frame writes them.  No host read; est, kept and every
    other stage are the bits of the call without crops.  None: nothing changes.
    With verify and crops both on and agreeing on image size, margin and z_min, the frame is rasterised once: one verify.RasterBatch goes to
    both stages.  Their results are the bits of the separate calls.
    complete (needs return_stages=True): True, or a dict of complete.complete_many's keyword arguments.  The stages gain 'complete' =
    {'encoded', 'cosine'}: a latent per entry of stages['params'] fitted to its lidar cloud alone (stages['lidar'][i][0]) at the refined pose, starting
    from the refined latent -- an independent check of the refinement beside verify --, and float64 [n] on the device, the cosine between the
    completed and the refined unit latents.  `origin`, the sensor's position, is the camera centre by default: that approximates the KITTI
    lidar's own position, which sits some decimetres from the camera.  No host read; est, kept and every other stage are the bits of the call
    without complete.  None: nothing changes.
    align (needs return_stages=True): True, or a dict of align.align_many's keyword arguments.  The stages gain 'align' = {'aligned', 'delta'}:
    pose and shape of every entry of stages['params'] fitted to its lidar cloud alone (stages['lidar'][i][0]), starting from the refined
    parameters -- a second, independent estimate of the pose, not only of the latent --, and float32 [n][5] on the device, the fitted yaw,
    trans and scale minus the refined ones.  `origin` as for complete.  No host read; est, kept and every other stage are the bits of the call
    without align.  None: nothing changes."""
    mesh_resolution, verify, crops = _stage_options("refine_frame", return_stages, mesh_resolution, verify, crops)
    align = None if align is None or align is False else ({} if align is True else dict(align))
    if align is not None and not return_stages:
        raise ValueError("refine_frame: align needs return_stages=True (the fitted poses are returned among the stages)")
    complete = None if complete is None or complete is False else ({} if complete is True else dict(complete))
    if complete is not None and not return_stages:
        raise ValueError("refine_frame: complete needs return_stages=True (the completed latents are returned among the stages)")
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
    meshes = None
    if mesh_resolution is not None or verify is not None or crops is not None:
        live = [j for j, lab in enumerate(labels) if lab is not None]
        meshes = meshes_many(dsdf, [refined[j]['latent'].to(precision) if torch.is_tensor(refined[j]['latent']) else refined[j]['latent']
                                    for j in live], resolution=64 if mesh_resolution is None else mesh_resolution)
        for m, j in zip(meshes, live):
            m.scale, m.cam_T = float(labels[j][1]._s), labels[j][2]              # the scale and matrix the label itself was built with
        meshes = [m.to_camera() for m in meshes]
    verdicts, crop_list = None, None
    if verify is not None or crops is not None:
        boxes = [annotations[kept[j]]['bbox'] for j in live]
        vkw, ckw = dict(verify or {}), dict(crops or {})
        vsize, csize = _stage_size(vkw, boxes), _stage_size(ckw, boxes)
        made = [(tuple(size), kw.get('margin', 0.25), kw.get('z_min', 0.1)) for size, kw in ((vsize, vkw), (csize, ckw))]
        shared = None
        if verify is not None and crops is not None and live and made[0] == made[1]:         # one raster for both stages
            shared = _verify.raster_batch(meshes, K_orig, label_windows(boxes, vsize, made[0][1])[1], vsize, made[0][2])
    if verify is not None:
        label_masks = vkw.pop('label_masks', None)
        verdicts = verify_many(dsdf, [refined[j] for j in live], meshes, [lidar[kept[j]][0] for j in live], K_orig, boxes, vsize,
                               label_masks=None if label_masks is None else [label_masks[kept[j]] for j in live], raster=shared, **vkw)
    if crops is not None:
        crop_list = crops_many(meshes, K_orig, boxes, csize, colors=[annotations[kept[j]]['color'] for j in live], raster=shared, **ckw)
        for c, j in zip(crop_list, live):
            c.latent, c.intrinsics, c.extrinsics = refined[j]['latent'], K_orig, labels[j][2]
    completed = None
    if complete is not None:
        enc = complete_many(dsdf, refined, [lidar[i][0] for i in kept], **complete)
        ref_lat = torch.stack([torch.as_tensor(r['latent']).detach().reshape(-1).to(enc.latents.device) for r in refined]) if refined else enc.latents
        completed = {'encoded': enc, 'cosine': _latent_cosine(enc.latents, ref_lat)}
    aligned = None
    if align is not None:
        fitted = align_many(dsdf, refined, [lidar[i][0] for i in kept], **align)
        start = torch.stack([torch.cat([torch.as_tensor(r[key]).detach().reshape(-1)[:n_].to(fitted.theta.device, torch.float32)
                                        for key, n_ in (('yaw', 1), ('trans', 3), ('scale', 1))]) for r in refined]) if refined else fitted.theta
        aligned = {'aligned': fitted, 'delta': fitted.theta - start}
    kept = [i for i, lab in zip(kept, labels) if lab is not None]
    if return_stages:
        stages = {'crop_sizes': sizes, 'intrinsics': intr, 'off_intrinsics': off, 'lidar': lidar, 'nocs_3d': nocs3d, 'surfaces': surf,
                  'poses': poses, 'params': refined, 'labels': labels}
        if meshes is not None and mesh_resolution is not None:
            stages['meshes'] = meshes
        if verdicts is not None:
            stages['verify'] = verdicts
        if crop_list is not None:
            stages['crops'] = crop_list
        if completed is not None:
            stages['complete'] = completed
        if aligned is not None:
            stages['align'] = aligned
        return est, kept, stages
    return est, kept


def refine_sample(sample, css_net, dsdf, grid, iters, weights, annos=None, diff_annos='', label_type='gt', maskrcnn_labels=None, lidar=None,
                  css_batch=None, pose_type='kabsch', scale=2.0, rendering_area=32, sampler='device', seed=0, keys=None, optimize_kwargs=None,
                  return_stages=False, remove_road=False, mesh_resolution=None, verify=None, crops=None,
                  complete=None, align=None):
    """One KITTI sample from the loaded frame to the evaluator's dicts: the body of the reference's frame loop (refine_css.py:94-245).

    sample: {'image' (H, W, 3) float32 BGR in 0 ... 1, 'orig_cam' 3x3, 'world_to_cam' 4x4, 'annos' {'easy', 'medium', 'hard'} and 'depth'
    (H, W), the sparse depth map}.  With `lidar` ([N][3], camera frame, already restricted to what should be rasterised -- the reference
    removes the road plane first) the depth map is built by frame.depth_map instead and sample['depth'] is not read.  With `lidar` and
    remove_road=True the lidar is the raw scan and the depth map is frame.kitti_frame's (road_free_depth_map): the road plane is removed on the device first, as
    get_kitti_frame does (the normals are frame.lidar_normals' own statement of Open3D's; parity with Open3D is untested).  That adds no
    host synchronisation.
    css_net: a module mapping [n][3][128][128] to {'uvw_sm_masked', 'latent'}; the shipped one is sdflabel_amd.networks.resnet_css.setup_css
    (the reference's network with its output head fused on the device, loads a reference css.pt).  annos: the annotations to label; None selects them with
    get_annos(diff_annos, sample).  label_type: 'gt' (the annotations' own boxes), 'rcnn' or 'maskrcnn' with maskrcnn_labels = {'bboxes'
    [M][4], 'masks' per detector box a mask of its truncated box}.  The remaining arguments are refine_frame's.

    Steps: (1) the annotations; (2) for 'rcnn' / 'maskrcnn' frame.match_boxes: an annotation whose best detector box has get_iou < 0.5 is
    dropped, the others take that box truncated to integers (:101-114); (3) colour and depth crops as views of the frame on the device;
    (4) frame.css_inputs_many -- for 'maskrcnn' with the matched mask, which goes into the CSS input only: the lidar crop's colours are
    reprojected unmasked, as the reference masks crop_bgr after its reproject (:130-135); (5) ONE css_net forward over all crops under
    torch.no_grad(), NOCS = uvw_sm_masked / 255 and the latent in the grid's precision (:142-144); (6) refine_frame, unchanged.

    BATCHING THE CSS FORWARD may differ in low bits from the reference's batch-1 calls, because the convolution algorithm the backend
    picks can depend on the batch size.  css_batch=1 restores one call per crop (css_batch=k: chunks of k crops).
    A network in TRAIN mode -- setup_css's default, and how refine_css.py:40 runs it -- normalises every BatchNorm layer with the statistics of
    the batch it is given, so there a crop's prediction depends on the other crops of the call: only css_batch=1 reproduces the reference's
    per-crop statistics.  (The fused output head itself gives a crop the same bits in any batch.)
    The caller's sample and annotations are not modified (the reference overwrites anno['bbox'] with the matched box).

    Host synchronisations beyond refine_frame's: none for 'gt'; one for 'rcnn' / 'maskrcnn', the read of the match.
    Returns (frame_estimations, kept, frame_annos): refine_frame's dict and the indices into the selected annotations behind its rows, and
    the {key: list / ndarray} dict of ALL selected annotations the evaluator takes as the frame's ground truth (:97, :242-245; with their
    original boxes, and including the annotations that were dropped, as the reference appends before it skips; a key of alpha, bbox,
    dimensions, location, rotation_y, score that no annotation carries is left out, where the reference stores an empty array).  With return_stages a
    fourth value: refine_frame's stages (rows: the annotations that passed the matching) plus 'annos', 'boxes', 'match', 'depth', 'css_input',
    'css_input_orig', 'nocs_pred', 'latents'.  keys, if given, holds one RANSAC key per selected annotation.
    mesh_resolution: refine_frame's (needs return_stages=True; the stages gain 'meshes').
    verify: refine_frame's (needs return_stages=True; the stages gain 'verify').  The windows are clipped to the sample's image, and with
    label_type='maskrcnn' the matched detector masks are the label masks, so 'iou_mask' is filled.
    crops: refine_frame's (needs return_stages=True; the stages gain 'crops').  The windows are clipped to the sample's image and the RGB
    bytes come from the sample's image.
    complete: refine_frame's (needs return_stages=True; the stages gain 'complete').  The sensor's position defaults to the camera centre,
    an approximation of the KITTI lidar's own position.
    align: refine_frame's (needs return_stages=True; the stages gain 'align')."""
    mesh_resolution, verify, crops = _stage_options("refine_sample", return_stages, mesh_resolution, verify, crops)
    if label_type not in ('gt', 'rcnn', 'maskrcnn'):
        raise ValueError("refine_sample: label_type must be 'gt', 'rcnn' or 'maskrcnn'")
    device = grid.points.device
    if device.type != 'cuda':
        raise _lib.SdfrError("refine_sample runs on the GPU only; there is no CPU fallback")
    precision = grid.points.dtype
    annos = get_annos(diff_annos, sample) if annos is None else list(annos)
    frame_annos = defaultdict(list)
    for anno in annos:
        for key, value in anno.items():
            frame_annos[key].append(value)
    for key in NECESSARY_KEYS:
        if key in frame_annos:                                                    # (the reference makes an empty array of a key no annotation has)
            frame_annos[key] = np.asarray(frame_annos[key])
    frame_annos = dict(frame_annos)
    image = _as_tensor(sample['image'], device)
    H, W = int(image.shape[0]), int(image.shape[1])
    K_orig = sample['orig_cam']
    if remove_road and lidar is None:
        raise ValueError("refine_sample: remove_road=True needs the lidar scan")
    if lidar is None:
        depth = _as_tensor(sample['depth'], device)
    else:
        depth = road_free_depth_map(lidar, K_orig, W, H) if remove_road else depth_map(lidar, K_orig, W, H)
    # boxes
    live = list(range(len(annos)))
    boxes = [[int(v) for v in np.asarray(a['bbox']).tolist()] if label_type == 'gt' else None for a in annos]
    if label_type == 'gt':
        for a, bx in zip(annos, boxes):
            if not np.array_equal(np.asarray(a['bbox']), np.asarray(bx)):
                raise ValueError("refine_sample: an annotation's bbox must hold integers for label_type='gt' (the reference slices the image with it)")
    masks, match = None, None
    if label_type != 'gt':
        if maskrcnn_labels is None:
            raise ValueError("refine_sample: label_type %r needs maskrcnn_labels" % label_type)
        det = maskrcnn_labels['bboxes']
        det = det.detach().cpu().numpy() if torch.is_tensor(det) else np.asarray(det)
        live, best_h = [], np.zeros(0, np.int32)
        if annos:
            best, iou, keep = match_boxes(np.asarray([np.asarray(a['bbox'], np.float64) for a in annos]), det)
            host = torch.stack([best, keep.int()]).cpu().numpy()                  # the one host synchronisation of the matching
            best_h = host[0]
            live = [i for i in range(len(annos)) if host[1, i]]
            match = {'best': best, 'iou': iou, 'keep': keep}
        for i in live:
            boxes[i] = det[best_h[i]].astype(np.int64).tolist()                    # bbox_maskrcnn.astype(np.int): truncation
        if label_type == 'maskrcnn':
            masks = [maskrcnn_labels['masks'][int(best_h[i])] for i in live]
    lboxes = [boxes[i] for i in live]
    # crops (views of the frame on the device) and the CSS network's input
    colors = [image[t:b, l:r] for l, t, r, b in lboxes]
    depths = [depth[t:b, l:r] for l, t, r, b in lboxes]
    css_in, css_vis = css_inputs_many(image, np.asarray(lboxes, np.int64).reshape(-1, 4), masks=masks, orig=True)
    nocs, latents = [], []
    if live:
        step = len(live) if not css_batch else max(1, int(css_batch))
        with torch.no_grad():
            for c0 in range(0, len(live), step):
                pred = css_net(css_in[c0:c0 + step])
                uvw, lat = pred['uvw_sm_masked'].detach(), pred['latent'].detach()
                for j in range(uvw.shape[0]):
                    nocs.append(uvw[j] / 255.)
                    latents.append(lat[j].to(precision))
    annotations = [{'bbox': lboxes[j], 'color': colors[j], 'depth': depths[j], 'nocs_pred': nocs[j]} for j in range(len(live))]
    if verify is not None:
        verify = dict(verify, image_size=(W, H))
        if masks is not None:
            verify.setdefault('label_masks', masks)
    if crops is not None:
        crops = dict(crops, image_size=(W, H))
    out = refine_frame(annotations, dsdf, grid, latents, K_orig, sample['world_to_cam'], iters, weights, pose_type=pose_type, scale=scale,
                       rendering_area=rendering_area, sampler=sampler, seed=seed, keys=None if keys is None else [keys[i] for i in live],
                       optimize_kwargs=optimize_kwargs, return_stages=return_stages, mesh_resolution=mesh_resolution, verify=verify, crops=crops, complete=complete,
                       align=align)
    kept = [live[j] for j in out[1]]
    if return_stages:
        stages = dict(out[2], annos=annos, boxes=boxes, match=match, css_input=css_in, css_input_orig=css_vis, nocs_pred=nocs, latents=latents,
                      depth=depth)
        return out[0], kept, frame_annos, stages
    return out[0], kept, frame_annos
