"""One shape fitted to several views of an object under a trained shape prior, batched on the device (csrc/track.hip).

    from sdflabel_amd.track import align_tracks, Tracked

align.align_many sees an object from one sensor position.  A drive shows the same object from several: a VIEW is one cloud of one object in
one camera frame, with its own yaw and trans; a TRACK is the object, an ordered list of one or more views with ONE latent and (by default)
ONE scale.  What the views share is fitted once, what differs per view is fitted per view.  Per iteration, for the views of a staged group
of whole tracks at once: sdfr_align_rows, the decoder pair and sdfr_align_reduce run over the views exactly as align_many runs them over
shapes -- every view's latent row a copy of its track's --, and sdfr_track_step folds each track's views into one loss, one latent gradient
and one scale gradient (weighted means in ascending view order), steps the latent and the scale, steps every view's yaw and trans from the
view's own gradient, and writes the next iteration's latent row and pose row of every view.  Nothing is read back in the loop.  A track of
one view is align_many in every bit.

WHAT IS AND IS NOT CLAIMED.  ALL DEFAULTS (align_many's, with 'scale' among the fitted parameters) ARE PARAMETERS
WITHOUT A CLAIMED OPERATING POINT.  'scale' IS ON HERE, where align_many leaves it off, because several sides of an object determine its
size: the degeneracy of depth and scale that one side leaves is broken as soon as the views see the object from different directions -- it
is NOT broken by views from the same side, and nothing here checks which case a track is.  The size of the shape inside the lattice cube
and `scale` REMAIN COUPLED THROUGH THE PRIOR ALONE: a latent that draws a smaller shape in the cube with a larger scale fits the same
clouds, and only the prior's preference among its shapes separates the two.  No motion model ties the views' poses together, the sensor
origin is one per call, and nothing is claimed about label quality on real drives.
"""
import torch

from . import _lib
from .align import _PoseFit, _rates, align_samples_many
from .complete import BoundSamples, _check_view, _cloud_normals, _on_device
from .encode import _fit, _upload
from .mesh import STAGING_BYTES

NO_VIEWS, NO_USABLE, SKIPPED, BAD_TABLE = 1, 2, 4, 8                     # Tracked.flags (csrc/track_cells.h)
MAX_VIEWS = 1024                                                         # views of one track (TRK_MAX_VIEWS)


class Tracked:
    """`.latents` float32 [T][L]: the tracks' latents as the decoder sees them (the row of each track's first view); `.raw_latents`: the
    optimised variables.  `.scale` float32 [T]: the tracks' scales (with share_scale; else each track's first view's).  `.theta` float32
    [V][5] = yaw, tx, ty, tz, scale per view; `.voff`: a host list, track t owns views voff[t] .. voff[t + 1] - 1.  `.loss` float64 [T]: the
    weighted mean of the usable views' losses on the rows of the last iteration, before its step (NaN with iters = 0); `.view_loss` float64
    [V].  `.flags` int32 [T] of the last iteration: 2 no usable view, 4 not stepped, 8 a broken table entry (align_tracks builds the table, so
    it does not occur here); `.view_flags` int32 [V]: Aligned.flags's bits, 4 for a view that sat the iteration out.  `.history` float32
    [iters][T] or None.  `.samples`: the views' BoundSamples.  `.params`: per track a list with one {'yaw' [1], 'trans' [3], 'scale' [1],
    'latent' [L]} per view, views of the shared tensors: labels_many, meshes_many, verify_many and complete_many take them.  All on the
    device."""

    def __init__(self, latents, raw_latents, scale, theta, voff, loss, view_loss, flags, view_flags, history, samples, unit_latents, share_scale):
        self.latents, self.raw_latents, self.scale, self.theta, self.voff = latents, raw_latents, scale, theta, voff
        self.loss, self.view_loss, self.flags, self.view_flags, self.history = loss, view_loss, flags, view_flags, history
        self.samples, self.unit_latents, self.share_scale = samples, unit_latents, share_scale
        self.params = [[{"yaw": theta[v, 0:1], "trans": theta[v, 1:4], "scale": scale[t:t + 1] if share_scale else theta[v, 4:5], "latent": latents[t]}
                        for v in range(voff[t], voff[t + 1])] for t in range(len(voff) - 1)]


class _TrackFit(_PoseFit):
    """encode._fit's description of the joint fit: the views are its shapes (rows, decoder pair and reduce are align_many's), the groups fall
    on whole tracks, and the step is sdfr_track_step over the tracks of the group, with the tracks' latents, scales and Adam state beside the
    views' state."""
    step_call = "sdfr_track_step"

    def __init__(self, view_params, voff, weights, share, samples, make_samples, lr, lr_pose, seed, history, iters):
        _PoseFit.__init__(self, view_params, samples, make_samples, lr, lr_pose, seed)
        self.who = "align_tracks"
        self.voff, self.weights, self.share, self.want_history, self.iters = voff, weights, share, history, iters
        self.T = len(voff) - 1

    def start(self, dev, Ld):
        z_view = _PoseFit.start(self, dev, Ld)                            # [V][L]: every view starts from its track's latent and scale
        T = self.T
        first = _upload(torch.tensor(self.voff[:-1], dtype=torch.int64), dev)
        self.first = first
        self.z = z_view[first].contiguous() if T else torch.zeros((0, Ld), dtype=torch.float32, device=dev)
        self.m, self.v = torch.zeros_like(self.z), torch.zeros_like(self.z)
        self.scale = self.theta[first, 4].contiguous() if T else torch.zeros((0,), dtype=torch.float32, device=dev)
        self.sm, self.sv = torch.zeros_like(self.scale), torch.zeros_like(self.scale)
        self.loss = torch.full((T,), float("nan"), dtype=torch.float64, device=dev)
        self.flags = torch.zeros((T,), dtype=torch.int32, device=dev)
        self.hist = torch.zeros((self.iters, T), dtype=torch.float32, device=dev) if self.want_history else None
        self.w = None if self.weights is None else _upload(torch.tensor(self.weights, dtype=torch.float32), dev)
        self.tables = {}
        return z_view

    def group_size(self, nb):
        return max([nb] + [self.voff[t + 1] - self.voff[t] for t in range(self.T)])

    def groups(self, nb):
        out, t = [], 0
        while t < self.T:
            e = t + 1
            while e < self.T and self.voff[e + 1] - self.voff[t] <= nb:
                e += 1
            out.append((self.voff[t], self.voff[e] - self.voff[t]))
            self.tables[self.voff[t]] = (t, e - t, [self.voff[i] - self.voff[t] for i in range(t, e + 1)])
            t = e
        return out

    def group(self, b0, inputs, J, NI):
        P = _lib.ptr
        t0, nt, table = self.tables[b0]
        if not torch.is_tensor(table):
            table = _upload(torch.tensor(table, dtype=torch.int64), self.theta.device)
            self.tables[b0] = (t0, nt, table)
        # the tracks' pointers of this group, formed once: the loop slices nothing
        self.head = (P(self.z[t0:]), P(self.m[t0:]), P(self.v[t0:]))
        self.mid = (P(self.scale[t0:]), P(self.sm[t0:]), P(self.sv[t0:]), 1 if self.share else 0, P(table))
        self.tail = (P(self.loss[t0:]), P(self.flags[t0:]))
        self.nt, self.wp, self.hp = nt, None if self.w is None else P(self.w[b0:]), None if self.hist is None else P(self.hist[:, t0:])
        return _PoseFit.group(self, b0, inputs, J, NI)

    def step(self, step_fn, b0, n, z, m, v, Ld, unit, step_mid, g, loss, flags, code_reg, rates, t, hist, B, st):
        return step_fn(*self.head, Ld, self.nt, unit, *self.mid, n, self.wp, *step_mid, z, g, loss, flags, *self.tail, code_reg, *rates, t, self.hp, self.T, st)


def _weights(weights, views, V):
    if weights is None:
        return None
    if isinstance(weights, str):
        if weights != "points":
            raise ValueError("align_tracks: weights must be None, 'points' or one number per view (got %r)" % (weights,))
        return [float(len(v["cloud"])) if "cloud" in v and v["cloud"] is not None else 1.0 for v in views]
    w = [float(x) for x in (weights.tolist() if hasattr(weights, "tolist") else weights)]
    if len(w) != V:
        raise ValueError("align_tracks: %d weights for %d views" % (len(w), V))
    return w


@_lib.traced("align_tracks")
def align_tracks(dsdf, tracks, origin=(0.0, 0.0, 0.0), free_rows=4, eta=0.02, s_max=1.0, seed=0, fit=("yaw", "trans", "scale", "latent"), share_scale=True,
                 weights=None, iters=200, rows_per_iter=2000, lr=5e-3, lr_pose=1e-2, lr_step=None, lr_factor=0.1, clamp=0.2, code_reg=1e-4, unit_latents=True,
                 history=False, staging_bytes=STAGING_BYTES, draw=None, samples=None):
    """Fit one latent and one scale per track, and yaw and trans per view, to the views' lidar clouds alone, under the frozen decoder `dsdf`.

    tracks: a list of {'latent': [L], 'scale': [1], 'views': [{'yaw', 'trans', 'cloud', 'normals' (optional)}, ...]}: the start latent and
    scale of the object and, per view in order, the start pose and the camera-frame cloud (normals: float64 [n][3], else estimated with
    frame.lidar_normals).  A view may carry a 'scale' of its own, used with share_scale=False.  samples: rows made before, one BoundSamples
    per view in track order (align_samples_many over all views, whose hash index is the view's global index), instead of clouds.
    origin, free_rows, eta, s_max, seed: align_samples_many's.  fit, lr, lr_pose, lr_step, lr_factor, clamp, rows_per_iter, draw, code_reg,
    unit_latents, history: align_many's; 'scale' is among the fitted parameters by default (see the module docstring).
    share_scale: one scale per track (the default), or one per view.  weights: None (every view counts once), 'points' (each view's point
    count) or one positive number per view: a view's loss and its latent and scale gradients enter its track's with that weight; a view's own
    yaw and trans do not see it.  staging_bytes: views are staged in groups of whole tracks; a group holds at least one track.

    Returns a Tracked.  The module docstring says what the defaults are and what is not claimed."""
    tracks = list(tracks)
    T, F = len(tracks), int(free_rows)
    lr_lat, lr_p = _rates(fit, lr, lr_pose)
    voff, views, params = [0], [], []
    for t, tr in enumerate(tracks):
        vs = list(tr["views"])
        if not 1 <= len(vs) <= MAX_VIEWS:
            raise ValueError("align_tracks: a track has 1 .. %d views (track %d has %d)" % (MAX_VIEWS, t, len(vs)))
        for v in vs:
            params.append({"yaw": v["yaw"], "trans": v["trans"], "scale": tr["scale"] if share_scale or "scale" not in v else v["scale"], "latent": tr["latent"]})
        views += vs
        voff.append(len(views))
    V = len(views)
    _check_view("align_tracks", V, F, eta, s_max)
    w = _weights(weights, views, V)
    make = None
    if samples is None:
        clouds = [v["cloud"] for v in views]
        normals = [v.get("normals") for v in views]

        def make(dev):
            cl = _on_device(clouds, torch.float32, dev)
            nrm = [(_cloud_normals(c) if len(c) else torch.zeros((0, 3), dtype=torch.float64, device=dev)) if n is None else n for c, n in zip(cl, normals)]
            return align_samples_many(clouds, nrm, origin, F, eta, s_max, seed, _device=dev)
    else:
        samples = [samples] if isinstance(samples, BoundSamples) else list(samples)
        if len(samples) != V:
            raise ValueError("align_tracks: %d views, %d sample sets" % (V, len(samples)))
    f = _TrackFit(params, voff, w, bool(share_scale), samples, make, lr_lat, lr_p, seed, bool(history), max(int(iters), 0))
    zn, z_view, view_loss, vflags, _, unit = _fit(f, dsdf, iters, rows_per_iter, lr_step, lr_factor, clamp, code_reg, unit_latents, seed, False, staging_bytes,
                                                  draw)
    latents = zn[f.first] if T else zn
    return Tracked(latents, f.z, f.scale, f.theta, voff, f.loss, view_loss, f.flags, vflags, f.hist, f.samples, unit, bool(share_scale))
