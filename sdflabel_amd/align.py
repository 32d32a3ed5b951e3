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
from .complete import BoundSamples, _check_view, _cloud_normals, _on_device, _view_rows
from .encode import _Fit, _fit, _upload
from .mesh import STAGING_BYTES

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
        self.found = self.chosen = self.fits = None                # align_many(search=...): the search.Found, the chosen rank, every kept start's fit
        self.params = [{"yaw": theta[b, 0:1], "trans": theta[b, 1:4], "scale": theta[b, 4:5], "latent": latents[b]} for b in range(int(theta.shape[0]))]


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
    _check_view("align_samples_many", B, F, eta, s_max)
    if B == 0:
        return []
    device = _device
    if device is None:
        device = next((c.device for c in clouds if torch.is_tensor(c) and c.is_cuda), None)
    dev = torch.device("cuda" if device is None else device)
    if dev.type != "cuda":
        raise _lib.SdfrError("align_samples_many runs on the GPU only; there is no CPU fallback")
    return _view_rows("align_samples_many", "sdfr_align_samples", clouds, normals, origin, F, eta, s_max, seed, dev)


def _make_samples(clouds, normals, origin, F, eta, s_max, seed, dev):
    """the observation rows align_many makes of its clouds: normals=None estimates them with frame.lidar_normals on each cloud"""
    if normals is None:
        normals = [_cloud_normals(c) if len(c) else torch.zeros((0, 3), dtype=torch.float64, device=dev) for c in _on_device(clouds, torch.float32, dev)]
    return align_samples_many(clouds, normals, origin, F, eta, s_max, seed, _device=dev)


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


class _PoseFit(_Fit):
    """encode._fit's description of the pose-and-shape fit: the sdfr_align_* calls, the camera-frame point beside lo and hi among a row's side
    arrays, five gradient columns after the latent's, and theta, its Adam state and the pose row as per-shape state beside the latent."""
    step_call, ws_call, extra = "sdfr_align_step", "sdfr_align_ws_bytes", 5

    def __init__(self, params_list, samples, make_samples, lr, lr_pose, seed):
        _Fit.__init__(self, "align_many", "sdfr_align_rows", "sdfr_align_reduce", 5, "qx qy qz lo hi", "BoundSamples.load(path, device)",
                      [] if samples is None else samples, lr, None, seed)
        self.params_list, self.make_samples, self.lr_pose = params_list, make_samples, lr_pose
        self.B, self.row_floats = len(params_list), 5                     # cam (3 words), lo, hi

    def check(self, Ld):
        self.check_rows()
        for p in self.params_list:
            if int(np.prod(tuple(p["latent"].shape))) != Ld:
                raise ValueError("align_many: a start latent of %d elements for a decoder of latent size %d" % (int(np.prod(tuple(p["latent"].shape))), Ld))

    def start(self, dev, Ld):
        if self.make_samples is not None:
            self.samples = self.make_samples(dev)
        if self.B == 0:
            self.theta = torch.zeros((0, 5), dtype=torch.float32, device=dev)
            return torch.zeros((0, Ld), dtype=torch.float32, device=dev)
        from .verify import _pose_rows
        pose0, z = _pose_rows(self.params_list, dev)
        yaws = [torch.as_tensor(p["yaw"]).detach().reshape(-1)[:1].to(torch.float32) for p in self.params_list]
        yaw = torch.stack(yaws) if all(y.is_cuda for y in yaws) else _upload(torch.stack([y.cpu() for y in yaws]), dev)
        self.theta = theta = torch.cat([yaw.to(dev), pose0[:, 2:]], 1).contiguous()
        # the pose row as sdfr_align_step writes it: cos and sin in double of the float32 yaw, rounded once
        self.pose = torch.cat([torch.cos(theta[:, :1].double()).float(), torch.sin(theta[:, :1].double()).float(), theta[:, 1:]], 1).contiguous()
        self.tm, self.tv = torch.zeros_like(theta), torch.zeros_like(theta)
        return z.clone().contiguous()

    def alloc(self, n_max, dev):
        self.cam = torch.empty((n_max, 3), dtype=torch.float32, device=dev)
        self.lo, self.hi = (torch.empty((n_max,), dtype=torch.float32, device=dev) for _ in range(2))

    def group(self, b0, inputs, J, NI):
        P = _lib.ptr
        pose, cam, lo, hi = P(self.pose[b0:]), P(self.cam), P(self.lo), P(self.hi)
        return ((pose, inputs, cam, lo, hi), (pose, None, None, None, None), (lo, hi, J, NI, cam, pose),
                (P(self.theta[b0:]), P(self.tm[b0:]), P(self.tv[b0:]), pose))

    def rates(self, f):
        return self.lr * f, (ctypes.c_float * 5)(*[r * f for r in self.lr_pose])


@_lib.traced("align_many")
def align_many(dsdf, params_list, clouds, normals=None, origin=(0.0, 0.0, 0.0), free_rows=4, eta=0.02, s_max=1.0, seed=0, fit=("yaw", "trans", "latent"),
               iters=200, rows_per_iter=2000, lr=5e-3, lr_pose=1e-2, lr_step=None, lr_factor=0.1, clamp=0.2, code_reg=1e-4, unit_latents=True,
               history=False, staging_bytes=STAGING_BYTES, draw=None, samples=None, *, search=None):
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

    search: None, or a dict for search.search_poses -- `codes` (a codebook [C][L]), `yaws` (yaw offsets, default (0, pi)), `keep` (default 2),
    `rows` (default rows_per_iter) --: the starts of every shape (codes x yaw offsets on the given box) are scored and ranked first, the fit
    runs on B x keep copies of the shapes from the kept starts (the latents of params_list are not used), and search.choose returns, per
    shape, the copy whose fit ended with the lowest loss.  The Aligned then holds the chosen fits, `.found` the search.Found, `.chosen` int64
    [B] the chosen rank (-1: none usable, rank 0 is returned) and `.fits` the Aligned of all B x keep fits, shape-major.

    Returns an Aligned.  See the module docstring for what the defaults are."""
    params_list = list(params_list)
    B, F = len(params_list), int(free_rows)
    lr_lat, lr_p = _rates(fit, lr, lr_pose)
    _check_view("align_many", B, F, eta, s_max)
    if search is not None:
        return _align_searched(dsdf, params_list, clouds, samples, dict(search), dict(normals=normals, origin=origin, free_rows=F, eta=eta, s_max=s_max, seed=seed),
                               dict(fit=fit, iters=iters, rows_per_iter=rows_per_iter, lr=lr, lr_pose=lr_pose, lr_step=lr_step, lr_factor=lr_factor,
                                    clamp=clamp, code_reg=code_reg, unit_latents=unit_latents, history=history, staging_bytes=staging_bytes, draw=draw))
    make = None
    if samples is None:
        clouds = list(clouds)
        if len(clouds) != B:
            raise ValueError("align_many: %d parameter sets, %d clouds" % (B, len(clouds)))
        if normals is not None and len(normals) != B:
            raise ValueError("align_many: %d parameter sets, %d normal arrays" % (B, len(normals)))

        def make(dev):
            return _make_samples(clouds, normals, origin, F, eta, s_max, seed, dev)
    else:
        samples = [samples] if isinstance(samples, BoundSamples) else list(samples)
        if len(samples) != B:
            raise ValueError("align_many: %d parameter sets, %d sample sets" % (B, len(samples)))
    f = _PoseFit(params_list, samples, make, lr_lat, lr_p, seed)
    zn, z, loss, flags, hist, unit = _fit(f, dsdf, iters, rows_per_iter, lr_step, lr_factor, clamp, code_reg, unit_latents, seed, history, staging_bytes, draw)
    return Aligned(zn, z, f.theta, loss, flags, hist, f.samples, unit)


def _align_searched(dsdf, params_list, clouds, samples, search, view_kw, kw):
    """align_many with search=: search.search_poses, the fit of every kept start, search.choose"""
    from . import search as S
    if "codes" not in search or set(search) - {"codes", "yaws", "keep", "rows"}:
        raise ValueError("align_many: search must be a dict with 'codes' and, if wanted, 'yaws', 'keep' and 'rows' (got %r)" % (sorted(search),))
    B, keep = len(params_list), int(search.get("keep", 2))
    if samples is not None:
        samples = [samples] if isinstance(samples, BoundSamples) else list(samples)
    elif len(list(clouds)) != B:
        raise ValueError("align_many: %d parameter sets, %d clouds" % (B, len(list(clouds))))
    found = S.search_poses(dsdf, params_list, clouds, search["codes"], yaws=search.get("yaws", (0.0, float(np.pi))), keep=keep, samples=samples,
                           rows=int(search.get("rows", kw["rows_per_iter"])), clamp=kw["clamp"], unit_latents=kw["unit_latents"], draw=kw["draw"],
                           staging_bytes=kw["staging_bytes"], **view_kw)
    fits = align_many(dsdf, [found.params[b][r] for b in range(B) for r in range(keep)], None, seed=view_kw["seed"],
                      samples=[found.samples[b] for b in range(B) for _ in range(keep)], **kw)
    unusable = torch.full_like(fits.flags, BAD_TABLE)
    chosen = S.choose(fits.loss.reshape(B, keep), torch.where(found.valid.reshape(-1), fits.flags, unusable).reshape(B, keep))
    at = torch.arange(B, device=chosen.device) * keep + chosen.clamp(min=0)
    out = Aligned(fits.latents[at], fits.raw_latents[at], fits.theta[at], fits.loss[at], fits.flags[at],
                  None if fits.history is None else fits.history[:, at], found.samples, fits.unit_latents)
    out.found, out.chosen, out.fits = found, chosen, fits
    return out
