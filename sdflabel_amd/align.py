"""Pose and shape fitted to one view under a trained shape prior, batched on the device (csrc/align.hip).

    from sdflabel_amd.align import align_many, align_samples_many, Aligned

complete.complete_many fits a latent at a fixed pose.  Here the pose moves too: yaw, trans (and, as a switch, scale) are fitted with the
latent to the lidar cloud alone, from any rough start -- no CSS network, no rendering.  The observation rows are made once, in the CAMERA
frame and in METRES (align_samples_many: the point with [0, 0], two points offset along its normal with [+-eta, +-eta], free-space points on
its sensor ray with [0, s]), so they stay true whatever the pose becomes.  Per iteration, for all shapes of a staged group at once:
sdfr_align_rows draws rows and takes them through the current pose into the lattice frame, the decoder runs forward with its ReLU masks
saved, sdfr_mlp_jacobian gives d sdf / d (latent, xyz), sdfr_align_reduce forms the interval loss of the metric prediction scale * sdf and
its gradient with respect to latent, yaw, trans and scale, sdfr_align_step applies Adam to both and writes the next pose.  A row that leaves
the lattice cube under the current pose sits out that iteration.  Nothing is read back in the loop.

THE DEFAULTS (four free-space rows per point, eta = 0.02 m, s_max = 1 m, 200 iterations of 2000 rows, learning rates 5e-3 for the latent
and 1e-2 for every pose parameter, clamp 0.2 m) ARE PARAMETERS WITHOUT A CLAIMED OPERATING POINT.  They are what the float64 statement of
the fit was tried with on one fixture; nothing else is claimed of them.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from .complete import MAX_FREE, BoundSamples, _cloud_normals
from .encode import MAX_ITERS, MAX_ROWS, _upload
from .mesh import STAGING_BYTES, _decoder_mode, decoder_rows

EMPTY, NO_ROWS, SKIPPED, BAD_TABLE, BAD_POSE = 1, 2, 4, 8, 16            # Aligned.flags (csrc/encode_cells.h, csrc/align_cells.h)
POSE_KEYS = ("yaw", "tx", "ty", "tz", "scale")                           # the columns of theta
FIT_KEYS = {"yaw": (0,), "trans": (1, 2, 3), "scale": (4,), "latent": ()}


class Aligned:
    """`.params`: per shape a dict {'yaw' [1], 'trans' [3], 'scale' [1], 'latent' [L]} of float32 device tensors (views of `.theta` and
    `.latents`), as the refinement leaves them: labels_many, meshes_many, verify_many and complete_many take them.  `.latents` float32
    [B][L]: the latents as the decoder sees them; `.raw_latents`: the optimised variables.  `.theta` float32 [B][5] = yaw, tx, ty, tz, scale.
    `.loss` float64 [B]: each shape's loss on the rows of the last iteration, before that iteration's step (NaN with iters = 0).  `.flags`
    int32 [B] of the last iteration: 1 no samples, 2 no row with a finite prediction and usable bounds inside the cube, 4 not stepped,
    8 a broken offset-table entry, 16 an unusable pose.  `.history` float32 [iters][B] or None.  `.samples`: the list of BoundSamples (camera
    frame, metric).  All on the device."""

    def __init__(self, latents, raw_latents, theta, loss, flags, history, samples, unit_latents):
        self.latents, self.raw_latents, self.theta, self.loss, self.flags, self.history = latents, raw_latents, theta, loss, flags, history
        self.samples, self.unit_latents = samples, unit_latents
        self.params = [{"yaw": theta[b, 0:1], "trans": theta[b, 1:4], "scale": theta[b, 4:5], "latent": latents[b]} for b in range(int(theta.shape[0]))]


def _clouds_on(clouds, dev):
    pts = []
    for c in clouds:
        t = c.detach() if torch.is_tensor(c) else torch.from_numpy(np.ascontiguousarray(c, dtype=np.float32))
        t = t.reshape(-1, 3).to(torch.float32)
        pts.append(t if t.is_cuda else _upload(t, dev))
    return pts


@_lib.traced("align_samples_many")
def align_samples_many(clouds, normals=None, origin=(0.0, 0.0, 0.0), free_rows=4, eta=0.02, s_max=1.0, seed=0, _device=None):
    """Camera-frame, metric interval rows from what one sensor position sees of each shape: complete.view_samples_many without a pose.

    clouds: per shape the camera-frame points [n][3] of its frustum.  normals: per shape float64 [n][3] camera-frame normals, or None for
    no normal rows.  origin: the sensor's position in the camera frame.  Every point p gives 3 + free_rows rows `q lo hi`: p with [0, 0];
    p +- eta n^ with [+-eta, +-eta] (left out where the normal is not finite or zero); and, for f < free_rows, p - s d^ with [0, s], d^ the
    unit vector from the sensor to p and s = ((f + u) / free_rows) min(s_max, |p - sensor|), u the library's hash of (seed, shape, point, f).
    The rows are camera-frame and metric: q is in the camera frame, [lo, hi] holds the true signed distance at q IN METRES (eta and s_max
    are metres too), which is a fact about the scene and not about any pose; there is no cube test.  A slot whose point is not finite holds
    position 0 and NaN bounds.  Returns a list of BoundSamples on the device, views of one array; `.flags` is 8 for a broken table entry.
    No host read and no synchronisation."""
    clouds = list(clouds)
    B, F = len(clouds), int(free_rows)
    if normals is not None and len(normals) != B:
        raise ValueError("align_samples_many: %d clouds, %d normal arrays" % (B, len(normals)))
    if not 0 <= F <= MAX_FREE:
        raise ValueError("align_samples_many: free_rows must be 0 .. %d (got %d)" % (MAX_FREE, F))
    if not (np.isfinite(eta) and np.isfinite(s_max) and s_max >= 0):
        raise ValueError("align_samples_many: eta must be finite, s_max finite and not negative")
    if B > 65535:
        raise ValueError("align_samples_many: at most 65535 shapes per call")
    if B == 0:
        return []
    device = _device
    if device is None:
        device = next((c.device for c in clouds if torch.is_tensor(c) and c.is_cuda), None)
    dev = torch.device("cuda" if device is None else device)
    if dev.type != "cuda":
        raise _lib.SdfrError("align_samples_many runs on the GPU only; there is no CPU fallback")
    pts = _clouds_on(clouds, dev)
    sizes = [int(t.shape[0]) for t in pts]
    nrm = None
    if normals is not None:
        nrm = []
        for c, n in zip(normals, sizes):
            t = c.detach() if torch.is_tensor(c) else torch.from_numpy(np.ascontiguousarray(c, dtype=np.float64))
            t = t.reshape(-1, 3).to(torch.float64)
            if int(t.shape[0]) != n:
                raise ValueError("align_samples_many: %d normals for %d points" % (int(t.shape[0]), n))
            nrm.append(t if t.is_cuda else _upload(t, dev))
        nrm = torch.cat(nrm).contiguous()
    ptoff = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    N, Pn = int(ptoff[-1]), 3 + F
    points = torch.cat(pts).contiguous()
    d_ptoff = _upload(torch.from_numpy(ptoff), dev)
    org = _upload(torch.tensor([float(v) for v in origin], dtype=torch.float32).reshape(3), dev)
    rows = torch.empty((N * Pn, 5), dtype=torch.float32, device=dev)
    flags = torch.empty((B,), dtype=torch.int32, device=dev)
    Pt = _lib.ptr
    with _lib.guard(dev):
        _lib.check(_lib.lib().sdfr_align_samples(Pt(points) if N else None, Pt(nrm) if (nrm is not None and N) else None, N, Pt(d_ptoff), B, Pt(org), 0, F,
                                                 float(eta), float(s_max), int(seed) & 0x7FFFFFFFFFFFFFFF, Pt(rows) if N else None, Pt(flags),
                                                 _lib.stream_ptr()), "sdfr_align_samples")
    return [BoundSamples(rows[int(ptoff[b]) * Pn:int(ptoff[b + 1]) * Pn], flags[b]) for b in range(B)]


def _rates(fit, lr, lr_pose):
    """(latent rate, the five pose rates) from `fit` and the rates given; a parameter that is not fitted has the rate 0"""
    fit = (fit,) if isinstance(fit, str) else tuple(fit)
    if not fit or any(f not in FIT_KEYS for f in fit):
        raise ValueError("align_many: fit must name some of 'yaw', 'trans', 'scale', 'latent' (got %r)" % (fit,))
    if isinstance(lr_pose, dict):
        if any(k not in FIT_KEYS or k == "latent" for k in lr_pose):
            raise ValueError("align_many: lr_pose may hold 'yaw', 'trans' and 'scale' (got %r)" % (sorted(lr_pose),))
        per = [float(lr_pose.get(k, 1e-2)) for k in ("yaw", "trans", "trans", "trans", "scale")]
    else:
        per = [float(lr_pose)] * 5
    if not (np.isfinite(per).all() and np.isfinite(lr) and min(per) >= 0 and lr >= 0):
        raise ValueError("align_many: the learning rates must be finite and not negative")
    on = {i for f in fit for i in FIT_KEYS[f]}
    return (float(lr) if "latent" in fit else 0.0), [r if i in on else 0.0 for i, r in enumerate(per)]


@_lib.traced("align_many")
def align_many(dsdf, params_list, clouds, normals=None, origin=(0.0, 0.0, 0.0), free_rows=4, eta=0.02, s_max=1.0, seed=0, fit=("yaw", "trans", "latent"),
               iters=200, rows_per_iter=2000, lr=5e-3, lr_pose=1e-2, lr_step=None, lr_factor=0.1, clamp=0.2, code_reg=1e-4, unit_latents=True,
               history=False, staging_bytes=STAGING_BYTES, draw=None, samples=None):
    """Fit pose and shape of every annotation to its lidar cloud alone, under the frozen decoder `dsdf`.

    params_list: per annotation the start {'yaw', 'trans', 'scale', 'latent'} (any rough box with a latent, or what the refinement leaves);
    clouds, normals, origin, free_rows, eta, s_max, seed: align_samples_many's (normals=None estimates them with frame.lidar_normals on each
    cloud, NaN where a point has fewer than 3 neighbours); samples: rows made before (a list of BoundSamples from align_samples_many), instead
    of clouds.  fit: which of 'yaw', 'trans', 'scale', 'latent' move; the others keep their start and their Adam state is never touched.
    lr: the latent's learning rate, lr_pose: the pose's -- one number, or a dict with 'yaw', 'trans', 'scale'; every rate is multiplied by
    lr_factor ** (iteration // lr_step), lr_step = iters // 2 by default.  clamp is in metres.  rows_per_iter, draw, code_reg, unit_latents,
    history, staging_bytes: encode.encode_many's.  The decoder's own mode (exact float32, float16, LayerNorm) runs the decoder pair.

    'scale' IS OFF BY DEFAULT, for a reason: from one side of an object, depth and scale are degenerate.  The lattice position of a point is
    rot^T (q / scale - trans), so a cloud seen from the camera's side fixes yaw, the lateral translation and the product scale * trans_z, and
    little else: with scale free the fit slides along scale * trans_z = const and ends wherever the prior's idea of the hidden side puts it.
    Fit the scale when the start's scale is worse than its depth, or when the cloud wraps the object.

    Returns an Aligned.  See the module docstring for what the defaults are."""
    params_list = list(params_list)
    B = len(params_list)
    iters, k_req, F = int(iters), int(rows_per_iter), int(free_rows)
    lr_lat, lr_p = _rates(fit, lr, lr_pose)
    if iters < 0 or iters >= MAX_ITERS:
        raise ValueError("align_many: iters must be 0 .. 2^24 - 1 (got %d)" % iters)
    if k_req < 1:
        raise ValueError("align_many: rows_per_iter must be at least 1 (got %d)" % k_req)
    if not float(clamp) > 0:
        raise ValueError("align_many: clamp must be positive")
    if lr_step is not None and int(lr_step) < 1:
        raise ValueError("align_many: lr_step must be at least 1")
    if not 0 <= F <= MAX_FREE:
        raise ValueError("align_many: free_rows must be 0 .. %d (got %d)" % (MAX_FREE, F))
    if not (np.isfinite(eta) and np.isfinite(s_max) and s_max >= 0):
        raise ValueError("align_many: eta must be finite, s_max finite and not negative")
    if samples is None:
        clouds = list(clouds)
        if len(clouds) != B:
            raise ValueError("align_many: %d parameter sets, %d clouds" % (B, len(clouds)))
        if normals is not None and len(normals) != B:
            raise ValueError("align_many: %d parameter sets, %d normal arrays" % (B, len(normals)))
    else:
        samples = [samples] if isinstance(samples, BoundSamples) else list(samples)
        if len(samples) != B:
            raise ValueError("align_many: %d parameter sets, %d sample sets" % (B, len(samples)))
        for s in samples:
            if s.rows.dim() != 2 or s.rows.shape[1] != 5:
                raise ValueError("align_many: sample rows must be [n][5] = qx qy qz lo hi")
    Ld = int(dsdf.latent_size)
    if not 1 <= Ld <= 256:
        raise ValueError("align_many: latent sizes 1 .. 256 (the decoder's is %d)" % Ld)
    if B > 65535:
        raise ValueError("align_many: at most 65535 shapes per call")
    for p in params_list:
        if int(np.prod(tuple(p["latent"].shape))) != Ld:
            raise ValueError("align_many: a start latent of %d elements for a decoder of latent size %d" % (int(np.prod(tuple(p["latent"].shape))), Ld))
    dev = next(dsdf.parameters()).device
    if dev.type != "cuda":
        raise _lib.SdfrError("align_many runs on the GPU only (the decoder is on %s); there is no CPU fallback" % dev)
    if samples is None:
        if normals is None:
            normals = [_cloud_normals(c) if len(c) else torch.zeros((0, 3), dtype=torch.float64, device=dev) for c in _clouds_on(clouds, dev)]
        samples = align_samples_many(clouds, normals, origin, F, eta, s_max, seed, _device=dev)
    for s in samples:
        if not s.rows.is_cuda:
            raise _lib.SdfrError("align_many: the sample rows must be on the GPU (BoundSamples.load(path, device))")
    counts = [len(s) for s in samples]
    full = [c for c in counts if c > 0]
    if draw is None:
        draw = not (full and min(full) == max(full) and full[0] <= k_req)
    k = k_req if draw else min([k_req] + full)
    if k > MAX_ROWS:
        raise ValueError("align_many: at most 2^20 rows per shape and iteration")
    lr_step = max(1, iters // 2) if lr_step is None else int(lr_step)

    loss = torch.full((B,), float("nan"), dtype=torch.float64, device=dev)
    flags = torch.zeros((B,), dtype=torch.int32, device=dev)
    hist = torch.zeros((iters, B), dtype=torch.float32, device=dev) if history else None
    if B == 0:
        e = torch.zeros((0, Ld), dtype=torch.float32, device=dev)
        return Aligned(e, e.clone(), torch.zeros((0, 5), dtype=torch.float32, device=dev), loss, flags, hist, [], bool(unit_latents))
    from .verify import _pose_rows
    pose0, z = _pose_rows(params_list, dev)
    z = z.clone().contiguous()
    yaws = [torch.as_tensor(p["yaw"]).detach().reshape(-1)[:1].to(torch.float32) for p in params_list]
    yaw = torch.stack(yaws) if all(y.is_cuda for y in yaws) else _upload(torch.stack([y.cpu() for y in yaws]), dev)
    theta = torch.cat([yaw.to(dev), pose0[:, 2:]], 1).contiguous()
    # the pose row as sdfr_align_step writes it: cos and sin in double of the float32 yaw, rounded once
    pose = torch.cat([torch.cos(theta[:, :1].double()).float(), torch.sin(theta[:, :1].double()).float(), theta[:, 1:]], 1).contiguous()
    zn = torch.empty_like(z)

    L = _lib.lib()
    P, ck = _lib.ptr, _lib.check
    handle, fwd, f16 = _decoder_mode(dsdf, dev)
    NI = Ld + 3
    rows = torch.cat([s.rows for s in samples]).float().contiguous() if sum(counts) else torch.zeros((0, 5), dtype=torch.float32, device=dev)
    S = int(rows.shape[0])
    off = [0]
    for c in counts:
        off.append(off[-1] + c)
    soff = _upload(torch.tensor(off, dtype=torch.int64), dev)
    mask_words = 0 if handle.has_ln else int(L.sdfr_decoder_mask_words(handle.h, k))
    per_shape = k * (4 * (2 * NI + 2 + 5)) + 4 * mask_words
    nb = max(1, min(B, int(staging_bytes) // max(per_shape, 1)))
    n_max = nb * k
    inputs = torch.empty((n_max, NI), dtype=torch.float32, device=dev)
    J = torch.empty((n_max, NI), dtype=torch.float32, device=dev)
    cam = torch.empty((n_max, 3), dtype=torch.float32, device=dev)
    lo, hi, pred, sel = (torch.empty((n_max,), dtype=torch.float32, device=dev) for _ in range(4))
    idx = torch.arange(n_max, dtype=torch.int32, device=dev)
    masks = None if handle.has_ln else torch.empty((int(L.sdfr_decoder_mask_words(handle.h, n_max)),), dtype=torch.int32, device=dev)
    ws_bytes = int(L.sdfr_align_ws_bytes(nb, k, Ld))
    ws = torch.empty((ws_bytes // 8,), dtype=torch.float64, device=dev)
    g = torch.empty((nb, Ld + 5), dtype=torch.float64, device=dev)
    m, v = torch.zeros_like(z), torch.zeros_like(z)
    tm, tv = torch.zeros_like(theta), torch.zeros_like(theta)
    cnts = {n: torch.full((1,), n * k, dtype=torch.int32, device=dev) for n in {nb, B % nb or nb}}
    unit = 1 if unit_latents else 0
    table_flags = torch.empty((nb,), dtype=torch.int32, device=dev)
    seed64 = int(seed) & 0x7FFFFFFFFFFFFFFF
    with _lib.guard(dev):
        st = _lib.stream_ptr()
        for b0 in range(0, B, nb):
            n = min(nb, B - b0)
            zg, so = z[b0:], soff[b0:]
            for it in range(iters):
                f = float(lr_factor) ** (it // lr_step)
                rates = (ctypes.c_float * 5)(*[r * f for r in lr_p])
                ck(L.sdfr_align_rows(P(rows), S, P(so), n, b0, k, 1 if draw else 0, seed64, it, P(zg), Ld, unit, P(pose[b0:]), P(inputs), P(cam), P(lo),
                                     P(hi), P(zn[b0:]), P(flags[b0:]), st), "sdfr_align_rows")
                decoder_rows(handle, fwd, f16, inputs, n * k, pred, J, sel, masks, idx, cnts[n], st)
                ck(L.sdfr_align_reduce(P(pred), P(lo), P(hi), P(J), NI, P(cam), P(pose[b0:]), Ld, n, k, float(clamp), P(ws), ws_bytes, P(loss[b0:]),
                                       P(g), P(flags[b0:]), st), "sdfr_align_reduce")
                ck(L.sdfr_align_step(P(zg), P(m[b0:]), P(v[b0:]), Ld, n, unit, P(theta[b0:]), P(tm[b0:]), P(tv[b0:]), P(pose[b0:]), P(g), P(loss[b0:]),
                                     P(flags[b0:]), float(code_reg), lr_lat * f, rates, it + 1, P(hist[:, b0:]) if hist is not None else None, B, st),
                   "sdfr_align_step")
            # the latents as the decoder sees the final z (and, with iters = 0, the flags of the table and the pose)
            ck(L.sdfr_align_rows(None, S, P(so), n, b0, k, 0, seed64, 0, P(zg), Ld, unit, P(pose[b0:]), None, None, None, None, P(zn[b0:]),
                                 P(flags[b0:] if iters == 0 else table_flags), st), "sdfr_align_rows")
    return Aligned(zn, z, theta, loss, flags, hist, samples, bool(unit_latents))
