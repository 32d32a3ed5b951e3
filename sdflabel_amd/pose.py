"""RANSAC pose initialisation of B crops on the device: the arithmetic of PoseEstimator.init_pose_3d (the reference's
utils/pose.py:85-233, types 'kabsch' and 'procrustes') behind sdfr_ransac_pose (csrc/pose.hip).

`ransac_pose` packs per-crop model / scene clouds into the ragged [B][cap][3] layout, applies the reference's in-dtype model scaling
(`model_pts *= scale_model` for 'kabsch', :126-127), launches the whole estimate on the current stream and returns device tensors.
It does not synchronise: host inputs go up through pinned buffers with asynchronous copies; the caller reads what it needs (pipelines/pose.py reads everything with one copy).
"""
import ctypes

import numpy as np
import torch

from . import _lib

RANSAC_P = 0.99              # utils/pose.py:132-135
RANSAC_OUTLIER_PROB = 0.7
RANSAC_SAMPLE_SIZE = 4
MIN_NUM_INLIERS = 5
TYPES = {"kabsch": 0, "procrustes": 1}


def ransac_iterations(p=RANSAC_P, outlier_prob=RANSAC_OUTLIER_PROB, sample_size=RANSAC_SAMPLE_SIZE):
    """the reference's hypothesis count, int(round(log(1 - p) / log(1 - (1 - outlier_prob)^4) + 0.5)) = 567"""
    return int(round((np.log(1.0 - p) / np.log(1 - pow(1 - outlier_prob, sample_size))) + 0.5))


def _mix64(z):
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def sample_indices_numpy(seed, key, n, T):
    """numpy restatement of the device sampler (csrc/pose.hip rs_sample_kernel): [T][4] int32 distinct indices in [0, n) from a
    splitmix64 hash of (seed, key, hypothesis, draw, attempt); all zero when n < 4.  Independent of any other crop."""
    out = np.zeros((T, 4), np.int32)
    if n < 4:
        return out
    with np.errstate(over="ignore"):
        u = np.uint64
        hk = _mix64(u(seed & 0xFFFFFFFFFFFFFFFF) ^ _mix64(u(key & 0xFFFFFFFFFFFFFFFF) * u(0x9E3779B97F4A7C15) + u(1)))
        for t in range(T):
            d = []
            for k in range(4):
                for c in range(64):
                    h = _mix64(hk ^ u((t << 16) | (k << 8) | c))
                    x = int((int(h) >> 32) * n >> 32)
                    if x not in d:
                        break
                else:
                    while x in d:
                        x = 0 if x + 1 == n else x + 1
                d.append(x)
            out[t] = d
    return out


def _upload(host, device):
    """host tensor -> device without waiting: staged through pinned memory, copied asynchronously on the current stream (a pageable copy
    would make the host wait for the stream).  The caching host allocator keeps the pinned block until the copy has run."""
    if torch.device(device).type != "cuda":
        return host.to(device)
    return host.contiguous().pin_memory().to(device, non_blocking=True)


def _as_tensor(a, device):
    if torch.is_tensor(a):
        a = a.detach()
        return a.to(device) if a.is_cuda else _upload(a, device)
    return _upload(torch.from_numpy(np.ascontiguousarray(a)), device)


def pack_inputs(model_pts, model_cls, scene_pts, scene_cls, type="kabsch", scale_model=1.0, device="cuda"):
    """Lists of per-crop clouds -> padded device arrays.  Model points / colours keep their dtype until the reference's in-place
    `model_pts *= scale_model` ('kabsch' only) has been applied in that dtype (float16 stays float16: numpy rounds the scale and the
    product to float16), then everything is widened to float32 (exact).  Returns (model, model_cls, mcnt, scene, scene_cls, ncnt, f16)."""
    B = len(model_pts)
    if not (len(model_cls) == len(scene_pts) == len(scene_cls) == B):
        raise ValueError("ransac_pose: the four lists need one entry per crop")
    ms, mcs, ss, scs = [], [], [], []
    f16 = None
    for b in range(B):
        m = _as_tensor(model_pts[b], device).reshape(-1, 3)
        if m.dtype not in (torch.float16, torch.float32):
            m = m.float()
        if f16 is None:
            f16 = m.dtype == torch.float16
        elif f16 != (m.dtype == torch.float16):
            raise ValueError("ransac_pose: all crops of a launch need the same model dtype")
        if m.shape[0] < 1:
            raise ValueError("ransac_pose: crop %d has no model points" % b)
        if type == "kabsch":
            m = m * torch.tensor(scale_model, dtype=m.dtype)        # a 0-dim host tensor: its value rounded to the dtype, no copy
        ms.append(m.float())
        mcs.append(_as_tensor(model_cls[b], device).reshape(-1, 3).float())
        ss.append(_as_tensor(scene_pts[b], device).reshape(-1, 3).float())
        scs.append(_as_tensor(scene_cls[b], device).reshape(-1, 3).float())
    mcap = max(1, max(m.shape[0] for m in ms))
    ncap = max(1, max(s.shape[0] for s in ss))

    def pad(lst, cap):
        out = torch.zeros((B, cap, 3), dtype=torch.float32, device=device)
        for b, x in enumerate(lst):
            out[b, :x.shape[0]] = x
        return out

    mcnt = _upload(torch.tensor([m.shape[0] for m in ms], dtype=torch.int32), device)
    ncnt = _upload(torch.tensor([s.shape[0] for s in ss], dtype=torch.int32), device)
    return pad(ms, mcap), pad(mcs, mcap), mcnt, pad(ss, ncap), pad(scs, ncap), ncnt, bool(f16)


def device_sample(ncnt, T, seed=0, keys=None):
    """the device sampler alone: [B][T][4] int32 on ncnt's device (keys: int64 per crop, default the crop's position)"""
    B = ncnt.shape[0]
    idx = torch.empty((B, T, 4), dtype=torch.int32, device=ncnt.device)
    kt = None if keys is None else _upload(torch.from_numpy(np.asarray(keys, dtype=np.int64).reshape(-1)), ncnt.device)
    with _lib.guard(ncnt):
        _lib.check(_lib.lib().sdfr_ransac_sample(int(seed), _lib.ptr(kt), _lib.ptr(ncnt), B, T, _lib.ptr(idx), _lib.stream_ptr()),
                   "sdfr_ransac_sample")
    return idx


def workspace_layout(B, ncap, T):
    """Python mirror of ws_layout (csrc/pose.hip): ([(name, bytes, dtype, shape), ...], total bytes) of the workspace's 256-byte aligned
    segments in their order.  The total equals sdfr_ransac_ws_bytes(B, ncap, T)."""
    al = lambda n: (n + 255) & ~255
    segs = [("cnn_d", al(8 * B * ncap), torch.float64, (B, ncap)), ("hyp", al(4 * 12 * B * T), torch.float32, (B, T, 12)),
            ("plist", al(4 * B * T), torch.int32, (B, T)), ("pcount", al(4 * B), torch.int32, (B,)), ("mask", al(4 * B * ncap), torch.int32, (B, ncap))]
    return segs, sum(s[1] for s in segs)


def workspace_views(out):
    """Typed views of a ransac_pose result's workspace (out["_keep"]), for tests and diagnostics: cnn_d [B][ncap] float64 (distance to the
    nearest model colour), hyp [B][T][12] float32 ([rot*scale | tra] of a hypothesis), plist [B][T] / pcount [B] (the scored hypotheses in
    order), mask [B][ncap] (the winner's inlier mask).  Defined entries only: hyp rows of scored hypotheses (counts >= 0), plist[:pcount],
    cnn_d[:N] and mask[:N] of a crop; everything else is whatever the allocator left there."""
    (B, ncap), T, ws = out["cnn_idx"].shape, out["gate"].shape[1], out["_keep"]
    segs, total = workspace_layout(B, ncap, T)
    if ws.numel() < total:
        raise ValueError("workspace_views: the workspace has %d bytes, the layout needs %d" % (ws.numel(), total))
    views, at = {}, 0
    for name, nbytes, dtype, shape in segs:
        n = 1
        for s in shape:
            n *= s
        views[name] = ws[at:at + n * torch.empty((), dtype=dtype).element_size()].view(dtype).view(shape)
        at += nbytes
    return views


@_lib.traced("ransac_pose")
def ransac_pose(model_pts, model_cls, scene_pts, scene_cls, type="kabsch", scale_model=1.0, sampler="device", seed=0, keys=None, idx=None,
                metric_distance_threshold=0.15, nocs_distance_threshold=0.15, iterations=None, device=None):
    """RANSAC Kabsch / Procrustes pose of every crop (the reference's init_pose_3d, steps 1-7) in one launch sequence, no host sync.

    model_pts, model_cls, scene_pts, scene_cls: lists (one entry per crop) of [n][3] device tensors or numpy arrays, float16 or float32.
    sampler: 'device' (counter-based hash of (seed, keys[b], hypothesis); keys default to the crop's position) or 'numpy' with `idx`
    given: per crop a [T][4] array of the reference's np.random.choice draws (ignored for crops with fewer than 5 scene points).
    Returns a dict of device tensors: found, best, n_inliers, scale, rot [B][3][3], tra [B][3], and the diagnostics idx [B][T][4],
    cnn_idx [B][ncap], gate [B][T] (bit 0 colour gate, bit 1 fit accepted, bit 2 rank-deficient sample), counts [B][T] (-1: not scored).
    """
    if type not in TYPES:
        raise NotImplementedError("ransac_pose: type %r (only 'kabsch' and 'procrustes'; PnP is the unported cv2.solvePnPRansac path)" % (type,))
    if device is None:
        first = model_pts[0] if len(model_pts) else None
        device = first.device if torch.is_tensor(first) and first.is_cuda else torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    if device.type != "cuda":
        raise _lib.SdfrError("ransac_pose runs on the GPU only; there is no CPU fallback")
    T = ransac_iterations() if iterations is None else int(iterations)
    B = len(model_pts)
    model, mcls, mcnt, scene, scls, ncnt, f16 = pack_inputs(model_pts, model_cls, scene_pts, scene_cls, type, scale_model, device)
    ncap, mcap = scene.shape[1], model.shape[1]
    if idx is not None:
        if torch.is_tensor(idx) and idx.dim() == 3:
            idx_t = idx.to(device=device, dtype=torch.int32).contiguous()
        else:
            host = np.zeros((B, T, 4), np.int32)
            for b, a in enumerate(idx):
                if a is not None and len(a):
                    host[b] = np.asarray(a, dtype=np.int32).reshape(T, 4)
            idx_t = _upload(torch.from_numpy(host), device)
        if tuple(idx_t.shape) != (B, T, 4):
            raise ValueError("ransac_pose: idx must be [B][T][4]")
    elif sampler != "device":
        raise ValueError("ransac_pose: sampler=%r needs the draws in idx" % (sampler,))
    else:
        idx_t = torch.empty((B, T, 4), dtype=torch.int32, device=device)
    kt = None if keys is None else _upload(torch.from_numpy(np.asarray(keys, dtype=np.int64).reshape(-1)), device)
    i32 = dict(dtype=torch.int32, device=device)
    f32 = dict(dtype=torch.float32, device=device)
    out = {"found": torch.empty(B, **i32), "best": torch.empty(B, **i32), "n_inliers": torch.empty(B, **i32), "scale": torch.empty(B, **f32),
           "rot": torch.empty((B, 3, 3), **f32), "tra": torch.empty((B, 3), **f32), "cnn_idx": torch.zeros((B, ncap), **i32),
           "gate": torch.empty((B, T), **i32), "counts": torch.empty((B, T), **i32), "idx": idx_t}
    h = _lib.lib()
    with _lib.guard(device):
        ws = torch.empty((max(1, int(h.sdfr_ransac_ws_bytes(B, ncap, T))),), dtype=torch.uint8, device=device)
        thr = (ctypes.c_double * 2)(float(metric_distance_threshold), float(nocs_distance_threshold))     # host array, read at the call
        _lib.check(h.sdfr_ransac_pose(_lib.ptr(model), _lib.ptr(mcls), _lib.ptr(mcnt), mcap, int(f16), _lib.ptr(scene), _lib.ptr(scls),
                                      _lib.ptr(ncnt), ncap, B, None if idx is None else _lib.ptr(idx_t), int(seed), _lib.ptr(kt), T, TYPES[type],
                                      float(scale_model), ctypes.cast(thr, ctypes.c_void_p), _lib.ptr(ws), _lib.ptr(out["found"]), _lib.ptr(out["best"]),
                                      _lib.ptr(out["n_inliers"]), _lib.ptr(out["scale"]), _lib.ptr(out["rot"]), _lib.ptr(out["tra"]),
                                      _lib.ptr(out["cnn_idx"]), _lib.ptr(out["gate"]), _lib.ptr(out["counts"]), _lib.ptr(idx_t),
                                      _lib.stream_ptr()), "sdfr_ransac_pose")
    out["ncnt"], out["mcnt"], out["model_f16"] = ncnt, mcnt, f16
    out["_keep"] = ws            # the workspace lives until the caller drops the result (stream-ordered frees make this belt and braces)
    return out
