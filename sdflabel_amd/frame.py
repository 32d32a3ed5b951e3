"""Frame labelling on the device: the glue of the reference's per-annotation loop (pipelines/refine_css.py:94-232) around the RANSAC pose,
the refinement and the evaluator, for all annotations of a frame at once.

  reproject_many     utils/refinement.py:360-410 (torch branch) for B ragged crops -- sdfr_reproject, one host synchronisation (the counts)
  init_params_many   refine_css.py:173-196: azimuth-only rotation, yaw, and the height fix-up of the RANSAC pose -- the point sums run in
                     sdfr_point_extents, the 3x3 algebra on the host (init_params_host)
  labels_many        utils/refinement.py:501-562 (get_kitti_label) for B parameter sets: one decoder / band / surface pass over B latents,
                     sdfr_point_extents, ONE device -> host copy per chunk, then the label in numpy float64 (assemble_labels)
  frame_dict         refine_css.py:242-245: a frame's labels stacked into the {key: ndarray} dict the evaluator takes

and the ingest of a frame, what the reference does on the host before a crop exists (csrc/ingest.hip):

  depth_map          utils/refinement.py:87-105 (compute_depth_map): the lidar rasterised into the sparse depth image -- sdfr_depth_map
  match_boxes        refine_css.py:101-114: the detector box of the largest get_iou per annotation, kept from 0.5 -- sdfr_match_boxes
  css_inputs_many    utils/refinement.py:60-84 (transform_bgr_crop) for all boxes of a frame, cut from the frame image on the device, Pillow's
                     8-bit bilinear resample reproduced byte for byte -- sdfr_css_input

and the road-plane removal of the reference's get_kitti_frame (utils/refinement.py:612-656; csrc/normals.hip):

  lidar_normals      a normal per lidar point from its max_nn nearest neighbours within a radius -- sdfr_lidar_normals.  The semantics are
                     written from Open3D's estimate_normals(KDTreeSearchParamHybrid); Open3D is not installed where this was developed, so
                     parity with it is NOT tested (tests pin a float64 restatement of the semantics instead)
  remove_road        the points to keep: inside the frustum and |n_y| <= 0.9
  kitti_frame        the road-removed depth map (sdfr_depth_map_masked) and the coloured scene points reprojected from it

There is no CPU fallback for the point arithmetic; the host parts (init_params_host, assemble_labels and the small helpers) are plain numpy
and are tested without a GPU against values recorded from the reference's own functions.
"""
import math

import numpy as np
import torch

from . import _lib
from .pose import _as_tensor, _upload

P, ck = _lib.ptr, _lib.check
NECESSARY_KEYS = ('alpha', 'bbox', 'dimensions', 'location', 'rotation_y', 'score')      # refine_css.py:242
IOU_RESTIMATE = 0.7                                                                     # refine_css.py:186
BAND_THRESHOLD = 0.03                                                                   # grid.py:43 default, as get_kitti_label calls it


# ---- small host helpers (the reference's utils/refinement.py functions of the same names; pipelines/refinement.py re-exports them) ----------

def rot_from_yaw(yaw):
    """utils/refinement.py:108-125: 3x3 rotation about y of a float or a 1-element tensor, in the tensor's dtype (float32 for a float)"""
    if not isinstance(yaw, torch.Tensor):
        yaw = torch.Tensor([yaw])
    c, s = torch.cos(yaw), torch.sin(yaw)
    z, o = yaw.new_tensor([0]), yaw.new_tensor([1])
    return torch.stack((c, z, s, z, o, z, -s, z, c)).view(3, 3)


def get_iou(a, b, epsilon=1e-5):
    """utils/refinement.py:128-165: IoU of two [x1, y1, x2, y2] boxes without the +1 pixel convention; 0.0 when they do not overlap"""
    w = min(a[2], b[2]) - max(a[0], b[0])
    h = min(a[3], b[3]) - max(a[1], b[1])
    if (w < 0) or (h < 0):
        return 0.0
    inter = w * h
    union = (a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1]) - inter
    return inter / (union + epsilon)


def compute_iou(boxA, boxB):
    """utils/refinement.py:168-198: IoU with the +1 pixel convention (inclusive box corners)"""
    xA, yA = max(boxA[0], boxB[0]), max(boxA[1], boxB[1])
    xB, yB = min(boxA[2], boxB[2]), min(boxA[3], boxB[3])
    inter = max(0, xB - xA + 1) * max(0, yB - yA + 1)
    areaA = (boxA[2] - boxA[0] + 1) * (boxA[3] - boxA[1] + 1)
    areaB = (boxB[2] - boxB[0] + 1) * (boxB[3] - boxB[1] + 1)
    return inter / float(areaA + areaB - inter)


def roty_in_bev(pose):
    """utils/refinement.py:201-220: KITTI rotation_y of a pose -- the angle of its rotated z axis from +x, negative when that axis points forward.
    math.acos raises outside [-1, 1], as in the reference."""
    fwd = (pose[:3, :3] @ np.asarray([0, 0, 1]).T).T
    rotation_y = math.acos(np.asarray([1, 0, 0]) @ fwd)
    if fwd[2] > 0:
        rotation_y *= -1
    return rotation_y


def alpha_in_bev(pose, rot_y):
    """utils/refinement.py:223-252: observation angle alpha = rot_y -/+ the angle of the ray to the object's position in the x-z plane"""
    x, z = pose[0, 3], pose[2, 3]
    theta = np.arctan2(abs(x), abs(z))
    return rot_y + theta if x < 0 else rot_y - theta


def adjust_intrinsics_crop(K, crop_size, bbox, max_crop_area):
    """utils/refinement.py:586-609: (crop size scaled to the rendering area [H, W] as ints, intrinsics of the scaled crop, intrinsics of the
    unscaled crop), the last two CPU float32 tensors.  crop_size: a torch tensor (H, W).  The caller's K is never modified (the reference's
    torch.Tensor(K) aliases a float32 numpy K and shifts the caller's matrix in place)."""
    l, t, r, b = bbox
    crop_H, crop_W = crop_size
    ratio = math.sqrt(max_crop_area / (crop_H * crop_W))
    size = (crop_size * ratio).int().numpy().tolist()
    intrinsics = torch.tensor(np.asarray(K.detach().cpu() if torch.is_tensor(K) else K), dtype=torch.float32)
    intrinsics[0, 2] -= l
    intrinsics[1, 2] -= t
    off_intrinsics = intrinsics.clone()
    intrinsics[:2] *= ratio
    return size, intrinsics, off_intrinsics


# ---- device helpers ----------------------------------------------------------------------------------------------------------------------

def _device(*things):
    for t in things:
        if torch.is_tensor(t) and t.is_cuda:
            return t.device
    if not torch.cuda.is_available():
        raise _lib.SdfrError("sdflabel_amd.frame runs on the GPU only; there is no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())


def _pack_flat(items, device):
    """list of arrays / tensors -> one flat float32 device tensor (host inputs: concatenated on the host and uploaded with ONE asynchronous copy)"""
    if all(not (torch.is_tensor(x) and x.is_cuda) for x in items):
        host = [np.ascontiguousarray(x.detach().numpy() if torch.is_tensor(x) else x, dtype=np.float32).reshape(-1) for x in items]
        return _upload(torch.from_numpy(np.concatenate(host) if host else np.zeros(0, np.float32)), device)
    return torch.cat([_as_tensor(x, device).reshape(-1).float() for x in items])


def point_extents(pts, off, cnt, cap, B, A=None, scale=None, t=None, K=None, half=False):
    """sdfr_point_extents: (ext float32 [B][10] = min/max of x, y, z, u, v of A (s p) + t; n int32 [B]).  No synchronisation."""
    dev = pts.device
    ext = torch.empty((B, 10), dtype=torch.float32, device=dev)
    n = torch.empty((B,), dtype=torch.int32, device=dev)
    with _lib.guard(dev):
        ck(_lib.lib().sdfr_point_extents(P(pts), P(off), P(cnt), int(cap), int(B), P(A), P(scale), P(t), P(K), 1 if half else 0, P(ext), P(n),
                                         _lib.stream_ptr()), "sdfr_point_extents")
    return ext, n


def _ragged(clouds, device):
    """list of [n][3] clouds -> (flat float32 [sum n][3], off int64 [B], cnt int32 [B], largest n) for sdfr_point_extents"""
    ts = [_as_tensor(c, device).reshape(-1, 3).float() for c in clouds]
    ns = [int(x.shape[0]) for x in ts]
    flat = torch.cat(ts) if ts else torch.zeros((0, 3), dtype=torch.float32, device=device)
    if flat.shape[0] == 0:
        flat = torch.zeros((1, 3), dtype=torch.float32, device=device)
    offs = np.concatenate([[0], np.cumsum(ns)[:-1]]).astype(np.int64) if ns else np.zeros(0, np.int64)
    meta = _upload(torch.from_numpy(np.concatenate([offs, np.asarray(ns, np.int64)])), device)
    return flat.contiguous(), meta[:len(ns)].contiguous(), meta[len(ns):].to(torch.int32), max(ns + [0])


# ---- reproject ---------------------------------------------------------------------------------------------------------------------------

@_lib.traced("reproject_device")
def reproject_device(colors, depths, Ks, filter=False, cap=None, over=None, device=None):
    """The launches of reproject_many without its synchronisation.  Returns a dict of device tensors: points, colors [B][cap][3], cnt int32 [B]
    (the TRUE counts) and the sticky flags over int32 [B] (bit 0: the crop held more than cap points, the surplus was dropped)."""
    B = len(depths)
    if not (len(colors) == len(Ks) == B):
        raise ValueError("reproject_many: colors, depths and Ks need one entry per crop")
    device = torch.device(device) if device is not None else _device(*depths, *colors)
    if device.type != "cuda":
        raise _lib.SdfrError("reproject_many runs on the GPU only; there is no CPU fallback")
    meta, kinv, dl, at = [], [], [], 0
    for b in range(B):
        d = depths[b].squeeze() if hasattr(depths[b], "squeeze") else np.squeeze(np.asarray(depths[b]))
        if d.ndim != 2:
            raise ValueError("reproject_many: depth %d must be (H, W) or (1, H, W)" % b)
        H, W = int(d.shape[0]), int(d.shape[1])
        c = colors[b]
        chw = int(c.shape[0]) == 3                                  # the reference's rule (:384): channels first when the first extent is 3
        if tuple(c.shape) != ((3, H, W) if chw else (H, W, 3)):
            raise ValueError("reproject_many: colour %d has shape %s for a %dx%d depth" % (b, tuple(c.shape), H, W))
        meta.append((W, H, at, int(chw)))
        at += H * W
        k = Ks[b]
        k = k.detach().cpu().float() if torch.is_tensor(k) else torch.from_numpy(np.asarray(k, dtype=np.float32))
        kinv.append(torch.inverse(k.reshape(3, 3)).reshape(9))     # on the host, as the reference inverts its CPU off_intrinsics (:381)
        dl.append(d)
    max_pix = max([m[0] * m[1] for m in meta] + [0])
    cap = max_pix if cap is None else int(cap)
    i32 = dict(dtype=torch.int32, device=device)
    out = {"points": torch.empty((B, max(cap, 1), 3), dtype=torch.float32, device=device),
           "colors": torch.empty((B, max(cap, 1), 3), dtype=torch.float32, device=device),
           "cnt": torch.empty((B,), **i32), "over": torch.zeros((B,), **i32) if over is None else over, "cap": cap}
    if B == 0:
        return out
    depth = _pack_flat(dl, device)
    color = _pack_flat(colors, device)
    if depth.numel() == 0:
        depth, color = torch.zeros(1, dtype=torch.float32, device=device), torch.zeros(3, dtype=torch.float32, device=device)
    small = _upload(torch.cat([torch.tensor(meta, dtype=torch.int32).reshape(-1).view(torch.float32), torch.stack(kinv).reshape(-1)]), device)
    meta_d, kinv_d = small[:4 * B].view(torch.int32), small[4 * B:]
    scratch = torch.empty((B * ((max_pix + 255) // 256) + 1,), **i32)
    with _lib.guard(device):
        ck(_lib.lib().sdfr_reproject(P(depth), P(color), P(meta_d), P(kinv_d), B, max_pix, int(bool(filter)), cap, P(out["points"]),
                                     P(out["colors"]), P(out["cnt"]), P(scratch), P(out["over"]), 1, _lib.stream_ptr()), "sdfr_reproject")
    return out


def reproject_many(colors, depths, Ks, filter=False, cap=None):
    """utils/refinement.py:360-410 (torch branch) for a frame's crops in one launch sequence.

    colors: per crop (3, H, W) or (H, W, 3); depths: per crop (H, W) or (1, H, W); Ks: per crop the 3x3 intrinsics of the crop (host arrays or
    CPU tensors, inverted on the host in float32 as the reference does).  Tensors or numpy arrays, on the host or the device.
    Returns per crop (points [n][3], colors [n][3]): float32 device views in torch.nonzero order (row-major), n = the pixels with depth != 0
    and -- with filter -- some colour channel > 0.  ONE host synchronisation: the read of the counts.  cap (default: the largest crop's pixel
    count, which cannot overflow) bounds the points kept per crop; a crop beyond it raises."""
    out = reproject_device(colors, depths, Ks, filter, cap)
    B = len(depths)
    if B == 0:
        return []
    host = torch.cat([out["cnt"], out["over"]]).cpu().numpy()
    if host[B:].any():
        raise _lib.SdfrError("reproject_many: crop(s) %s hold more than cap = %d points" % (np.nonzero(host[B:])[0].tolist(), out["cap"]))
    return [(out["points"][b, :int(host[b])], out["colors"][b, :int(host[b])]) for b in range(B)]


# ---- initial parameters ------------------------------------------------------------------------------------------------------------------

def constrain_rotation(rot):
    """refine_css.py:175-178: the rotation with its second row and column overwritten by [0, 1, 0] (a copy; float32) and
    yaw = roty_in_bev(rot @ diag(-1, 1, 1)) + pi / 2 (float64: the product with the integer matrix is one)"""
    rot = np.array(rot, dtype=np.float32)
    rot[:, 1] = [0, 1, 0]
    rot[1, :] = [0, 1, 0]
    return rot, roty_in_bev(rot @ np.diag([-1, 1, 1])) + math.pi / 2


def init_params_host(pose, rot, yaw, ext, scene_ymin, bbox, latent):
    """refine_css.py:183-196 given the extents of world = rot (pcd scale) + tra: ext = [xmin, xmax, ymin, ymax, zmin, zmax, umin, umax, vmin,
    vmax] (float32) and the scene cloud's smallest y.  Returns (params, iou)."""
    ext = np.asarray(ext, dtype=np.float32)
    tra = np.array(pose['tra'], dtype=np.float32)
    L, R, T, B = ext[6], ext[7], ext[8], ext[9]
    iou = compute_iou(list(bbox), [L, T, R, B])
    if iou < IOU_RESTIMATE:
        tra[1] = np.float32(scene_ymin) + (ext[3] - ext[2]) / 2
    latent = latent.detach().cpu().numpy() if torch.is_tensor(latent) else np.asarray(latent)
    return {'yaw': np.array([yaw]), 'trans': tra / pose['scale'], 'scale': np.array([pose['scale']]), 'latent': latent}, iou


@_lib.traced("init_params_many")
def init_params_many(poses, pcd_dsdf, scene_pts, bboxes, K_orig, latents, return_info=False):
    """The optimiser's initial parameters from the RANSAC poses of a frame (refine_css.py:173-196), quirks included: rot[:, 1] and rot[1, :]
    are overwritten with [0, 1, 0]; yaw = roty_in_bev(rot @ diag(-1, 1, 1)) + pi / 2; world = rot (pcd scale) + tra; the 2-D box of
    project(K_orig, world) is compared with the annotation's box by compute_iou (+1 convention) and below 0.7 the height becomes
    tra[1] = min y of the scene points + (ymax - ymin) / 2 of the world points; trans = tra / scale uses that tra.

    `project` is cv2.projectPoints with zero rotation, zero translation and no distortion, i.e. the pinhole fx x / z + cx, fy y / z + cy.
    cv2 is not installed where this was developed, so that equivalence rests on cv2's documentation, not on a test; the recorded values the
    tests compare with were made with a float64 pinhole in cv2's place.

    poses: per annotation {'scale', 'rot', 'tra'} or None (PoseEstimator.estimate_many); the dicts are not modified.  pcd_dsdf / scene_pts:
    per annotation the model surface and the reprojected NOCS points ([n][3], device or host).  A None pose yields None.
    One host synchronisation: the read of the extents.  Returns per annotation {'yaw', 'trans', 'scale', 'latent'} as the reference builds
    them (numpy), or None."""
    live = [i for i, p in enumerate(poses) if p is not None]
    res = [None] * len(poses)
    if not live:
        return (res, res) if return_info else res
    dev = _device(*[pcd_dsdf[i] for i in live], *[scene_pts[i] for i in live])
    half = all(torch.is_tensor(pcd_dsdf[i]) and pcd_dsdf[i].dtype == torch.float16 or
               isinstance(pcd_dsdf[i], np.ndarray) and pcd_dsdf[i].dtype == np.float16 for i in live) and \
        all(isinstance(poses[i]['scale'], float) for i in live)        # a float16 cloud times a Python float stays float16 in numpy
    rots, yaws = zip(*[constrain_rotation(poses[i]['rot']) for i in live])
    n = len(live)
    K = np.asarray(K_orig.detach().cpu() if torch.is_tensor(K_orig) else K_orig, dtype=np.float32).reshape(9)
    host = np.concatenate([np.stack(rots).reshape(n, 9), np.asarray([[poses[i]['scale']] for i in live], np.float32),
                           np.stack([np.asarray(poses[i]['tra'], np.float32) for i in live]), np.tile(K, (n, 1))], 1).astype(np.float32)
    d = _upload(torch.from_numpy(host), dev)
    A, s, t, Kd = d[:, :9].contiguous(), d[:, 9].contiguous(), d[:, 10:13].contiguous(), d[:, 13:22].contiguous()
    mp, moff, mcnt, mcap = _ragged([pcd_dsdf[i] for i in live], dev)
    sp, soff, scnt, scap = _ragged([scene_pts[i] for i in live], dev)
    e_model, _ = point_extents(mp, moff, mcnt, mcap, n, A, s, t, Kd, half=half)
    e_scene, _ = point_extents(sp, soff, scnt, scap, n)
    ext = torch.cat([e_model, e_scene]).cpu().numpy()
    info = [None] * len(poses)
    for j, i in enumerate(live):
        res[i], iou = init_params_host(poses[i], rots[j], yaws[j], ext[j], ext[n + j, 2], bboxes[i], latents[i])
        info[i] = {'iou': float(iou), 'ext': ext[j].copy(), 'scene_ymin': ext[n + j, 2], 'rot': rots[j]}
    return (res, info) if return_info else res


# ---- labels ------------------------------------------------------------------------------------------------------------------------------

def assemble_labels(ext, yaw, trans, scale, world_to_cam, bboxes):
    """The host part of get_kitti_label (utils/refinement.py:521-562) for B annotations, vectorised, following the reference's dtype flow:
    cos / sin of rot_from_yaw in float32 through torch on the CPU; cam_T, inv(p_WC), location, rotation_y and alpha in float64; trans * scale
    and the dimensions [height, width, length] in the precision of the inputs (float32, or float16 for a float16 grid).

    ext [B][>=6]: min x, max x, min y, max y, min z, max z of the scaled surface points; yaw [B], trans [B][3], scale [B]: numpy arrays in the
    computation's precision.  Returns (labels, cam_T [B][4][4])."""
    prec = np.asarray(trans).dtype
    ext = np.asarray(ext).astype(prec)
    yaw, trans, scale = np.asarray(yaw).reshape(-1), np.asarray(trans).reshape(-1, 3), np.asarray(scale, dtype=prec).reshape(-1)
    B = yaw.shape[0]
    y32 = torch.tensor(yaw.astype(np.float64), dtype=torch.float32)          # results['yaw'].item() -> torch.Tensor([yaw]): float32
    c, s = torch.cos(y32).numpy(), torch.sin(y32).numpy()
    rot = np.zeros((B, 3, 3), np.float32)
    rot[:, 0, 0], rot[:, 0, 2], rot[:, 1, 1], rot[:, 2, 0], rot[:, 2, 2] = c, s, 1, -s, c
    cam_T = np.tile(np.eye(4), (B, 1, 1))
    cam_T[:, :3, :3] = rot @ np.diag([1, -1, 1])
    cam_T[:, :3, 3] = trans * scale[:, None]
    glob = np.linalg.inv(world_to_cam) @ cam_T
    dims = np.stack([ext[:, 3] - ext[:, 2], ext[:, 1] - ext[:, 0], ext[:, 5] - ext[:, 4]], 1)        # height, width, length
    bottom = np.zeros((B, 3))
    bottom[:, 1] = ext[:, 2]
    loc = np.einsum('bij,bj->bi', glob[:, :3, :3], bottom) + glob[:, :3, 3]
    labels = []
    for b in range(B):
        rot_y = roty_in_bev(glob[b])
        labels.append({'name': 'Car', 'bbox': bboxes[b], 'location': loc[b], 'dimensions': [dims[b, 0], dims[b, 1], dims[b, 2]],
                       'rotation_y': rot_y, 'alpha': alpha_in_bev(glob[b], rot_y), 'score': 1})
    return labels, cam_T


class ScaledPoints:
    """get_kitti_label's `scaled_points` of one annotation, kept on the device: the surface points in the grid's precision times the scale.
    `.device()` is the device tensor; `.numpy()` / np.asarray(...) fetch it (one copy, on demand)."""

    def __init__(self, points, scale, dtype):
        self._p, self._s, self._dtype, self._host = points, scale, dtype, None

    def device(self):
        return self._p.to(self._dtype) * self._s.to(self._dtype)

    def numpy(self):
        if self._host is None:
            self._host = self.device().cpu().numpy()
        return self._host

    def __array__(self, dtype=None, copy=None):
        a = self.numpy()
        return a if dtype is None else a.astype(dtype)

    def __len__(self):
        return int(self._p.shape[0])


def _param_rows(params_list, device, dtype):
    """[B][5 + L] in `dtype`: yaw, trans, scale, latent of every annotation (device tensors stay there; host values go up in one copy)"""
    keys = ('yaw', 'trans', 'scale', 'latent')
    if all(not (torch.is_tensor(p[k]) and p[k].is_cuda) for p in params_list for k in keys):
        rows = [torch.cat([torch.as_tensor(np.asarray(p[k].detach() if torch.is_tensor(p[k]) else p[k])).reshape(-1).to(dtype) for k in keys])
                for p in params_list]
        return _upload(torch.stack(rows), device)
    return torch.stack([torch.cat([_as_tensor(p[k], device).reshape(-1).to(dtype) for k in keys]) for p in params_list])


@_lib.traced("labels_many")
def labels_many(dsdf, grid, params_list, world_to_cam, bboxes, max_batch=16, cap=None, threshold=BAND_THRESHOLD, return_raw=False):
    """get_kitti_label (utils/refinement.py:501-562) for a frame: KITTI labels from refined parameters.

    params_list: per annotation {'latent', 'scale', 'trans', 'yaw'} (tensors or arrays, as Optimizer.optimize_many leaves them); they are
    converted to the grid's precision as the reference's caller does (refine_css.py:229-231).  world_to_cam: the 4x4 p_WC; bboxes: per
    annotation the 2-D box that goes into the label unchanged.

    THE LATENT GOES IN RAW: the reference hands params['latent'] to the decoder un-normalised (:536), although the optimiser evaluates the
    normalised latent (optimizer.py:96).  So does this function; it never normalises.
    The computation runs in the grid's precision (:518, :547-550): with a float16 grid (and decoder) the surface points are float16 values and
    so is their product with the scale.

    Per chunk of max_batch annotations: the decoder over the grid, the band selection, the band Jacobian and the surface projection for all
    latents in one launch each (the launches of BatchRenderer's plain decoder stage), sdfr_point_extents, then ONE device -> host copy of
    the extents, counts and parameters -- the chunk's only host synchronisation -- and the label arithmetic on the host (assemble_labels).
    A band that exceeds cap (default max(256, G / 8) rows) raises.
    Returns per annotation (label, scaled_points, cam_T) -- scaled_points a ScaledPoints that stays on the device until asked -- or None for
    an annotation whose band is empty (the reference raises on min() of an empty array)."""
    n_all = len(params_list)
    if len(bboxes) != n_all:
        raise ValueError("labels_many: one bbox per annotation")
    pts = grid.points.detach()
    if not pts.is_cuda:
        raise _lib.SdfrError("labels_many runs on the GPU only; there is no CPU fallback")
    dev, prec = pts.device, pts.dtype
    if prec not in (torch.float32, torch.float16):
        raise _lib.SdfrError("labels_many: the grid must be float32 or float16")
    half = prec == torch.float16
    nprec = np.float16 if half else np.float32
    G, Ld = int(pts.shape[0]), int(dsdf.latent_size)
    NI = Ld + 3
    cap = max(256, G // 8) if cap is None else int(cap)
    handle = dsdf.handle(dev)
    mp = getattr(dsdf, "mlp_precision", torch.float32)
    f16 = mp == torch.float16 and not handle.has_ln
    split = mp == "float32_split" and not handle.has_ln and handle.hp == 512
    L = _lib.lib()
    fwd = L.sdfr_mlp_forward_f16 if f16 else (L.sdfr_mlp_forward_split if split else L.sdfr_mlp_forward)
    grid32 = pts.float()
    res, raw = [], []
    for c0 in range(0, n_all, max(1, int(max_batch))):
        chunk = params_list[c0:c0 + max(1, int(max_batch))]
        B = len(chunk)
        rows = _param_rows(chunk, dev, prec)                                  # in the grid's precision
        rows32 = rows.float()
        inputs = torch.empty((B, G, NI), dtype=torch.float32, device=dev)
        inputs[:, :, :Ld] = rows32[:, None, 5:]
        inputs[:, :, Ld:] = grid32
        f = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)       # noqa: E731
        i = lambda *s: torch.zeros(s, dtype=torch.int32, device=dev)         # noqa: E731
        sdf, mask_ws = f(B * G), i(int(L.sdfr_decoder_mask_words(handle.h, B * G)))
        idx, cnt, over, scratch = i(B, cap), i(B), i(B), i(B * ((G + 255) // 256) + 1)
        J, sdf_band, points, normals = f(B, cap, NI), f(B, cap), f(B, cap, 3), f(B, cap, 3)
        scale32 = rows32[:, 4].contiguous()
        with _lib.guard(dev):
            st = _lib.stream_ptr()
            ck(fwd(handle.h, P(inputs), B * G, P(sdf), P(mask_ws), st), fwd.__name__)
            ck(L.sdfr_band_select_ex(P(sdf), G, B, float(threshold), None, None, P(idx), cap, P(cnt), None, P(scratch), P(over), 1, st),
               "sdfr_band_select_ex")
            ck(L.sdfr_mlp_jacobian(handle.h, P(inputs), G, B, P(idx), cap, P(cnt), P(J), P(sdf_band), P(sdf), P(mask_ws), 2 if f16 else 0, st),
               "sdfr_mlp_jacobian")
            ck(L.sdfr_surface_project(P(inputs[0, :, Ld:]), NI, P(sdf), G, B, P(idx), cap, P(cnt), P(J), NI, Ld, P(points), None, P(normals), st),
               "sdfr_surface_project")
        ext, n = point_extents(points, None, cnt, cap, B, scale=scale32, half=half)
        host = torch.cat([ext.reshape(-1).view(torch.int32), n, over, rows32[:, :5].reshape(-1).view(torch.int32)]).cpu().numpy()
        e = host[:10 * B].view(np.float32).reshape(B, 10)
        nb, ov = host[10 * B:11 * B], host[11 * B:12 * B]
        prm = host[12 * B:].view(np.float32).reshape(B, 5).astype(nprec)        # exact: the values were rounded to the precision on the device
        if ov.any():
            raise _lib.SdfrError("labels_many: the band of annotation(s) %s exceeds cap = %d rows" % ((np.nonzero(ov)[0] + c0).tolist(), cap))
        ok = [b for b in range(B) if nb[b] > 0]
        labels, cam_T = assemble_labels(e[ok], prm[ok, 0], prm[ok, 1:4], prm[ok, 4], world_to_cam, [bboxes[c0 + b] for b in ok]) if ok else ([], [])
        out = [None] * B
        for j, b in enumerate(ok):
            out[b] = (labels[j], ScaledPoints(points[b, :int(nb[b])], rows[b, 4], prec), cam_T[j])
        res += out
        raw.append({"ext": e[:, :6].astype(nprec), "n": nb.copy(), "points": points, "cnt": cnt})
    return (res, raw) if return_raw else res


def frame_dict(labels):
    """refine_css.py:232,242-245: a frame's labels (the non-None ones, in order) as {key: list}, with alpha, bbox, dimensions, location,
    rotation_y and score turned into arrays -- what Detection3DEvaluator takes as a frame's estimations.  `labels`: label dicts, or the
    (label, scaled_points, cam_T) tuples of labels_many."""
    out = {k: [] for k in ('name', 'bbox', 'location', 'dimensions', 'rotation_y', 'alpha', 'score')}
    for lab in labels:
        if lab is None:
            continue
        lab = lab[0] if isinstance(lab, tuple) else lab
        for k, v in lab.items():
            out.setdefault(k, []).append(v)
    for k in NECESSARY_KEYS:
        out[k] = np.asarray(out[k])
    return out


def surfaces_many(dsdf, grid, latents):
    """refine_css.py:150-153 per annotation: the decoder on the grid with the CSS latent (raw, in the grid's precision) and the zero-isosurface
    projection.  Returns per annotation (pcd_dsdf, nocs_dsdf, normals_dsdf)."""
    out = []
    pts = grid.points
    for lat in latents:
        lat = _as_tensor(lat, pts.device).reshape(-1).to(pts.dtype)
        sdf, _ = dsdf(torch.cat([lat.expand(pts.size(0), -1), pts], 1))
        out.append(tuple(t.detach() for t in grid.get_surface_points(sdf)))
    return out


# ---- ingest: depth map, box matching, CSS inputs ----------------------------------------------------------------------------------------
CSS_SIZE = 128                                                                          # transforms.Resize((128, 128)), utils/refinement.py:74


def _host_array(a, dtype=None):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return a if dtype is None else a.astype(dtype, copy=False)


def _device_rows(a, width, device):
    """[n][width] on the device (an empty input is made there: there is nothing to copy)"""
    n = a.numel() if torch.is_tensor(a) else np.asarray(a).size
    if n == 0:
        return torch.zeros((0, width), dtype=torch.float64, device=device)
    return _as_tensor(a, device).reshape(-1, width)


def unproject(K, p2d):
    """utils/refinement.py:475-477: the rays ((u - cx) / fx, (v - cy) / fy, 1) through pixels p2d [n][2], float32.  cv2.undistortPoints without
    distortion is taken to be this pinhole (evaluated in float64, as cv2 does internally, and rounded to float32); cv2 is not installed where
    this was developed, so that equivalence is not tested."""
    K = _host_array(K, np.float64)
    p = np.asarray(p2d, np.float64).reshape(-1, 2)
    return np.stack([(p[:, 0] - K[0, 2]) / K[0, 0], (p[:, 1] - K[1, 2]) / K[1, 1], np.ones(len(p))], 1).astype(np.float32)


def build_view_frustum(K, l, t, r, b):
    """utils/refinement.py:480-494: the four inward plane normals (top, right, bottom, left) of the frustum through the box's corner pixels,
    float32 [4][3]"""
    corners = np.asarray([(l, t), (r - 1, t), (r - 1, b - 1), (l, b - 1)], dtype=np.float32)
    rays = unproject(K, corners)
    rays /= np.linalg.norm(rays, axis=1)[:, None]
    return np.stack((np.cross(rays[0], rays[1]), np.cross(rays[1], rays[2]), np.cross(rays[2], rays[3]), np.cross(rays[3], rays[0])))


def build_cam_frustum(K, img_w, img_h):
    """utils/refinement.py:497-498"""
    return build_view_frustum(K, 0, 0, img_w, img_h)


@_lib.traced("depth_map")
def depth_map(lidar, K, w, h, return_info=False):
    """compute_depth_map (utils/refinement.py:87-105) on the device: the lidar points [N][3] (camera frame; float64 or float32, host or
    device) inside the view frustum of the w x h image, projected by the pinhole of K in float64, rounded to float32 and truncated to a
    pixel.  Where several points land on a pixel the LAST one in input order sets it, as the reference's loop overwrites -- by an integer
    atomic maximum of the point index, so two runs give the same image.  The frustum planes are computed on the host (build_view_frustum).
    A kept point that float32 rounding puts at x == w or y == h (the reference raises IndexError there) is dropped and counted.
    `project` = cv2.projectPoints is taken to be the plain pinhole, as in init_params_many.
    No host synchronisation.  Returns depth float32 [h][w] on the device; with return_info also {'winner': int32 [h][w] (the index of the
    point behind each pixel, -1 without one), 'counts': int32 [2] = (points that landed on a pixel, points dropped outside the image)}."""
    w, h = int(w), int(h)
    dev = _device(lidar)
    if dev.type != "cuda":
        raise _lib.SdfrError("depth_map runs on the GPU only; there is no CPU fallback")
    Kh = _host_array(K, np.float64).reshape(3, 3)
    planes = np.ascontiguousarray(build_view_frustum(Kh, 0, 0, w, h), dtype=np.float32)
    cam = np.array([Kh[0, 0], Kh[1, 1], Kh[0, 2], Kh[1, 2]], np.float64)
    pts = _device_rows(lidar, 3, dev)
    if pts.dtype not in (torch.float32, torch.float64):
        pts = pts.double()
    pts = pts.contiguous()
    depth = torch.empty((h, w), dtype=torch.float32, device=dev)
    winner = torch.empty((h, w), dtype=torch.int32, device=dev)
    counts = torch.empty((2,), dtype=torch.int32, device=dev)
    with _lib.guard(dev):
        ck(_lib.lib().sdfr_depth_map(P(pts), int(pts.dtype == torch.float64), int(pts.shape[0]), planes.ctypes.data, cam.ctypes.data, w, h,
                                     P(depth), P(winner), P(counts), _lib.stream_ptr()), "sdfr_depth_map")
    return (depth, {"winner": winner, "counts": counts}) if return_info else depth


@_lib.traced("match_boxes")
def match_boxes(anno_boxes, det_boxes):
    """The matching of refine_css.py:101-114 for A annotation boxes against M detector boxes ([x1, y1, x2, y2] rows, host or device): get_iou
    (utils/refinement.py:128-165) in float64 -- the boxes are widened to float64 first, whatever they come in --, per annotation the FIRST
    detector box of the largest IoU (np.argmax).  No host synchronisation.
    Returns device tensors (best int32 [A], iou float64 [A], keep bool [A] = iou >= 0.5); best is -1 where there is no detector box."""
    dev = _device(anno_boxes, det_boxes)
    if dev.type != "cuda":
        raise _lib.SdfrError("match_boxes runs on the GPU only; there is no CPU fallback")
    a = _device_rows(anno_boxes, 4, dev).double().contiguous()
    d = _device_rows(det_boxes, 4, dev).double().contiguous()
    A, M = int(a.shape[0]), int(d.shape[0])
    best = torch.empty((A,), dtype=torch.int32, device=dev)
    iou = torch.empty((A,), dtype=torch.float64, device=dev)
    keep = torch.empty((A,), dtype=torch.int32, device=dev)
    with _lib.guard(dev):
        ck(_lib.lib().sdfr_match_boxes(P(a), A, P(d) if M else None, M, P(best), P(iou), P(keep), _lib.stream_ptr()), "sdfr_match_boxes")
    return best, iou, keep.bool()


@_lib.traced("css_inputs_many")
def css_inputs_many(image, boxes, masks=None, orig=False, return_u8=False):
    """transform_bgr_crop (utils/refinement.py:60-84) for all A boxes of a frame in one launch sequence, cut from the frame image on the
    device: per crop (crop * 255).astype(uint8) in float32, BGR -> RGB, PIL's 8-bit bilinear resize to 128 x 128 (reproduced byte for byte:
    horizontal pass over all rows, vertical pass over its uint8 result, 22-bit integer coefficients computed in double), ToTensor
    (float32(u8) / 255) and Normalize ((x - mean) / std).

    image: the frame [H][W][3], float32 BGR in 0 ... 1 (sample['image']), host or device.  boxes: A rows [l, t, r, b] of integers inside the
    image (host values; a device tensor is fetched).  masks: None, or per box None / a [b - t][r - l] mask that is multiplied into the crop
    in float32 first (refine_css.py:135, label_type 'maskrcnn').
    No host synchronisation for host boxes.  Returns im float32 [A][3][128][128] on the device; with orig (im, im_orig) where im_orig is the
    image before Normalize; with return_u8 additionally the resampled uint8 image [A][128][128][3]."""
    dev = _device(image)
    if dev.type != "cuda":
        raise _lib.SdfrError("css_inputs_many runs on the GPU only; there is no CPU fallback")
    img = _as_tensor(image, dev)
    if img.dim() != 3 or img.shape[2] != 3:
        raise ValueError("css_inputs_many: the image must be (H, W, 3), got %s" % (tuple(img.shape),))
    img = img.float().contiguous()
    H, W = int(img.shape[0]), int(img.shape[1])
    bx = _host_array(boxes).reshape(-1, 4)
    if not np.array_equal(bx, np.trunc(bx)):
        raise ValueError("css_inputs_many: boxes must hold integers (the reference slices the image with them)")
    bx = bx.astype(np.int64)
    A = int(bx.shape[0])
    f32 = dict(dtype=torch.float32, device=dev)
    im = torch.empty((A, 3, CSS_SIZE, CSS_SIZE), **f32)
    im_orig = torch.empty((A, 3, CSS_SIZE, CSS_SIZE), **f32) if orig else None
    u8 = torch.empty((A, CSS_SIZE, CSS_SIZE, 3), dtype=torch.uint8, device=dev) if return_u8 else None
    if A:
        if masks is not None and len(masks) != A:
            raise ValueError("css_inputs_many: one mask (or None) per box")
        meta = np.zeros((A, 8), np.int32)
        rows = blocks = melems = 0
        mlist = []
        for i, (l, t, r, b) in enumerate(bx.tolist()):
            if not (0 <= l < r <= W and 0 <= t < b <= H):
                raise ValueError("css_inputs_many: box %d = %s is empty or outside the %d x %d image" % (i, [l, t, r, b], W, H))
            m = None if masks is None else masks[i]
            meta[i] = (l, t, r - l, b - t, -1 if m is None else melems, rows, blocks, 0)
            if m is not None:
                if tuple(m.shape) != (b - t, r - l):
                    raise ValueError("css_inputs_many: mask %d has shape %s for a %d x %d crop" % (i, tuple(m.shape), b - t, r - l))
                mlist.append(m.float() if torch.is_tensor(m) else np.asarray(m, np.float32))
                melems += (b - t) * (r - l)
            rows += b - t
            blocks += (b - t + 7) // 8
        ksize = 2 * int(math.ceil(max(float(meta[:, 2:4].max()) / CSS_SIZE, 1.0))) + 1
        meta_d = _upload(torch.from_numpy(meta), dev)
        masks_d = _pack_flat(mlist, dev) if mlist else None
        coef = torch.empty((A, 2, CSS_SIZE, 2 + ksize), dtype=torch.int32, device=dev)
        tmp = torch.empty((rows, CSS_SIZE, 3), dtype=torch.uint8, device=dev)
        with _lib.guard(dev):
            ck(_lib.lib().sdfr_css_input(P(img), H, W, P(meta_d), A, P(masks_d), ksize, blocks, P(coef), P(tmp), P(im), P(im_orig), P(u8),
                                         _lib.stream_ptr()), "sdfr_css_input")
    out = (im,) + ((im_orig,) if orig else ()) + ((u8,) if return_u8 else ())
    return out[0] if len(out) == 1 else out


# ---- road-plane removal: lidar normals, the kept points, the frame's depth map and scene cloud -------------------------------------------

def _cloud(lidar, dev):
    pts = _device_rows(lidar, 3, dev)
    if pts.dtype not in (torch.float32, torch.float64):
        pts = pts.double()
    return pts.contiguous()


def _frustum(K, w, h):
    Kh = _host_array(K, np.float64).reshape(3, 3)
    return Kh, np.ascontiguousarray(build_view_frustum(Kh, 0, 0, int(w), int(h)), dtype=np.float32)


def _normals(pts, planes, radius, max_nn, want_idx):
    dev, N, max_nn = pts.device, int(pts.shape[0]), int(max_nn)
    if not 1 <= max_nn <= 64:
        raise ValueError("lidar_normals: max_nn must be 1 ... 64")
    if not (float(radius) > 0 and math.isfinite(float(radius))):
        raise ValueError("lidar_normals: the radius must be positive and finite")
    L = _lib.lib()
    normals = torch.empty((N, 3), dtype=torch.float64, device=dev)
    cnt = torch.empty((N,), dtype=torch.int32, device=dev)
    idx = torch.empty((N, max_nn), dtype=torch.int32, device=dev) if want_idx else None
    inside = torch.empty((N,), dtype=torch.uint8, device=dev)
    nbytes = int(L.sdfr_lidar_normals_ws_bytes(N))
    if nbytes < 0:
        raise _lib.SdfrError("lidar_normals: %d points are more than the library takes" % N)
    ws = torch.empty((max(nbytes, 16),), dtype=torch.uint8, device=dev)
    with _lib.guard(dev):
        ck(L.sdfr_lidar_normals(P(pts), int(pts.dtype == torch.float64), N, None if planes is None else planes.ctypes.data, float(radius), max_nn,
                                P(normals), P(cnt), P(idx), P(inside), P(ws), nbytes, _lib.stream_ptr()), "sdfr_lidar_normals")
    return normals, cnt, idx, inside


def _road_keep(pts, planes, radius, max_nn, cos_thresh):
    """(keep bool [N], info) of remove_road for a device cloud and host frustum planes"""
    normals, cnt, _, inside = _normals(pts, planes, radius, max_nn, False)
    inside = inside.bool()
    return inside & ~(normals[:, 1].abs() > float(cos_thresh)), {"normals": normals, "nn_count": cnt, "in_frustum": inside}


@_lib.traced("lidar_normals")
def lidar_normals(lidar, K=None, w=None, h=None, radius=1.0, max_nn=30, return_info=False):
    """A normal per lidar point, what get_kitti_frame asks of Open3D's estimate_normals(KDTreeSearchParamHybrid(radius=1.0, max_nn=30))
    (utils/refinement.py:628-631), on the device.  THE SEMANTICS ARE OURS, written from Open3D's EstimateNormals / KDTreeFlann::SearchHybrid;
    Open3D is not installed where this was developed, so parity with it is NOT tested.  The tests pin a float64 restatement of these rules:

    lidar [N][3], camera frame, float64 or float32 (widened first), host or device.  With K, w and h a point is in the frustum iff all four
    build_view_frustum(K, 0, 0, w, h) planes . p > 0 (float32 planes, float64 products, as depth_map); without them every point counts.  Only
    frustum points are queries and only frustum points can be neighbours.  The neighbours of point i are the frustum points j (i included)
    with d2 = (dx*dx + dy*dy) + dz*dz < radius*radius -- strictly, in float64; the radius is rounded to float32 first (1.0 and 0.5 are exact)
    -- ordered by (d2, j), the first max_nn (at most 64) kept, a tie at the cut going to the lower index; no cap on the candidates.  With fewer
    than 3 neighbours the normal is (0, 0, 1); otherwise the unit eigenvector of the smallest eigenvalue of the centred covariance
    (1 / k) sum (q - m)(q - m)^T, float64, summed in neighbour order; a zero covariance gives (0, 0, 1).  Open3D leaves the sign to its
    solver; here n . p <= 0 (towards the camera), a product of exactly 0 keeping the solver's sign.  Outside the frustum: (0, 0, 1).
    The same bits on every run; no host synchronisation.
    Returns normals float64 [N][3] on the device; with return_info also {'nn_count' int32 [N], 'nn_idx' int32 [N][max_nn] in that order,
    padded with -1, 'in_frustum' bool [N]}."""
    dev = _device(lidar)
    if dev.type != "cuda":
        raise _lib.SdfrError("lidar_normals runs on the GPU only; there is no CPU fallback")
    if (K is None) != (w is None) or (K is None) != (h is None):
        raise ValueError("lidar_normals: K, w and h go together")
    planes = None if K is None else _frustum(K, w, h)[1]
    normals, cnt, idx, inside = _normals(_cloud(lidar, dev), planes, radius, max_nn, return_info)
    return (normals, {"nn_count": cnt, "nn_idx": idx, "in_frustum": inside.bool()}) if return_info else normals


@_lib.traced("remove_road")
def remove_road(lidar, K, w, h, radius=1.0, max_nn=30, cos_thresh=0.9, return_info=False):
    """The points get_kitti_frame rasterises (utils/refinement.py:623-644): inside the image frustum and not on the road, the road being the
    points whose normal (lidar_normals, with its untested relation to Open3D) has |n_y| > cos_thresh.  No host synchronisation.
    Returns keep bool [N] on the device; with return_info also {'normals', 'nn_count', 'in_frustum'}.
    The reference's plane_normal / plane_offset (:636-640) are computed there but never used, so they are not provided."""
    dev = _device(lidar)
    if dev.type != "cuda":
        raise _lib.SdfrError("remove_road runs on the GPU only; there is no CPU fallback")
    keep, info = _road_keep(_cloud(lidar, dev), _frustum(K, w, h)[1], radius, max_nn, cos_thresh)
    return (keep, info) if return_info else keep


@_lib.traced("road_free_depth_map")
def road_free_depth_map(lidar, K, w, h, radius=1.0, max_nn=30, cos_thresh=0.9, return_info=False):
    """kitti_frame's depth map alone: remove_road, then compute_depth_map over the kept points in input order -- sdfr_depth_map_masked, the
    last kept point on a pixel wins, so the image has the bits of depth_map(lidar[keep]).  No host synchronisation.
    Returns depth float32 [h][w] on the device; with return_info also {'keep', 'normals', 'nn_count', 'in_frustum', 'winner' (indices into
    the WHOLE cloud), 'counts'}."""
    w, h = int(w), int(h)
    dev = _device(lidar)
    if dev.type != "cuda":
        raise _lib.SdfrError("road_free_depth_map runs on the GPU only; there is no CPU fallback")
    Kh, planes = _frustum(K, w, h)
    cam = np.array([Kh[0, 0], Kh[1, 1], Kh[0, 2], Kh[1, 2]], np.float64)
    pts = _cloud(lidar, dev)
    keep, info = _road_keep(pts, planes, radius, max_nn, cos_thresh)
    depth = torch.empty((h, w), dtype=torch.float32, device=dev)
    winner = torch.empty((h, w), dtype=torch.int32, device=dev)
    counts = torch.empty((2,), dtype=torch.int32, device=dev)
    with _lib.guard(dev):
        ck(_lib.lib().sdfr_depth_map_masked(P(pts), int(pts.dtype == torch.float64), int(pts.shape[0]), P(keep.view(torch.uint8)), planes.ctypes.data,
                                            cam.ctypes.data, w, h, P(depth), P(winner), P(counts), _lib.stream_ptr()), "sdfr_depth_map_masked")
    return (depth, dict(info, keep=keep, winner=winner, counts=counts)) if return_info else depth


@_lib.traced("kitti_frame")
def kitti_frame(image, lidar, K, return_info=False, radius=1.0, max_nn=30, cos_thresh=0.9):
    """get_kitti_frame (utils/refinement.py:612-656) from a raw scan: the frustum cut, remove_road, compute_depth_map over the kept points in
    input order (road_free_depth_map) and the reprojection of the coloured scene points (reproject_device, as :653).  image: the frame
    (H, W, 3); lidar [N][3], camera frame.  No host synchronisation.
    Returns (scene_depth float32 [H][W], pts_scene float32 [H * W][3], clrs_scene float32 [H * W][3]) on the device; the first `count` rows
    of the last two are the scene's points in row-major pixel order, the rest is unspecified; with return_info a fourth value, a dict with
    count (int32, on the device) and road_free_depth_map's info.  Not provided: the reference's plane_normal / plane_offset, which it
    computes but never uses; parsing KITTI3D files stays with the caller."""
    dev = _device(image, lidar)
    if dev.type != "cuda":
        raise _lib.SdfrError("kitti_frame runs on the GPU only; there is no CPU fallback")
    h, w = int(image.shape[0]), int(image.shape[1])
    depth, info = road_free_depth_map(lidar, K, w, h, radius, max_nn, cos_thresh, return_info=True)
    out = reproject_device([image], [depth], [K], device=dev)
    res = (depth, out["points"][0], out["colors"][0])
    return res + (dict(info, count=out["cnt"][0]),) if return_info else res
