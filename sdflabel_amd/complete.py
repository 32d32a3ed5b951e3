"""Shape completion from one view under a trained shape prior: DeepSDF's other use of a frozen decoder, batched on the device
(csrc/complete.hip).

    from sdflabel_amd.complete import complete_many, view_samples_many, fit_many, BoundSamples

What a sensor sees of a car is one side of it, and no closed mesh to sign samples with.  A latent can still be fitted to it: to the observed
points (sdf = 0), to points offset by eta along the surface normal (sdf = +-eta), and to free-space points on the sensor's ray in front of
each hit, where only an inequality is known.  One generalisation covers the three: every sample row carries an interval [lo, hi] the true
signed distance lies in.  An exact sample has lo == hi; a free-space point at distance s in front of its ray's hit has [0, s] -- both bounds
hold for any surface, because the hit itself is s away.  The loss of a row is the distance from the clamped prediction to the clamped
interval; a row inside its interval adds nothing.  With lo == hi everywhere the fit is encode.encode_many's in every bit.

view_samples_many turns lidar clouds and poses into such rows (sdfr_view_samples), fit_many is encode_many for them (sdfr_bound_rows,
sdfr_bound_reduce, and encode_many's own decoder launches and Adam step), complete_many chains the two from the parameters the refinement
leaves.

THE DEFAULTS OF THE ROWS (four free-space rows per point, eta = 0.01, s_max = 0.5, all in lattice units) ARE PARAMETERS WITHOUT A CLAIMED
OPERATING POINT.  eta is DeepSDF's shape-completion offset only AS RECALLED; it has not been checked against that paper's code, and the
free-space spacing is ours.  The fit's defaults are encode_many's (see encode.py for what is claimed of them).
"""
import numpy as np
import torch

from . import _lib
from .encode import Encoded, _Fit, _fit, _upload
from .mesh import STAGING_BYTES
from .sdf_samples import SdfSamples

BAD_POSE, BAD_TABLE = 4, 8                 # view flags (csrc/complete_cells.h)
MAX_FREE = 64


class BoundSamples:
    """Interval samples of one shape: `.rows` float32 [n][5] = x y z lo hi in the lattice frame, the true signed distance at x y z lying in
    [lo, hi]; a row whose bounds are NaN is left out of a fit.  `.flags`: the shape's flag word from view_samples_many (a 0-d int32 device
    tensor: 4 an unusable pose, 8 a broken offset-table entry), else None."""

    def __init__(self, rows, flags=None):
        self.rows, self.flags = rows, flags

    def __len__(self):
        return int(self.rows.shape[0])

    def numpy(self):
        return self.rows.detach().cpu().numpy()

    def save(self, path):
        """one .npz file with the key `rows`, float32 [n][5].  One host read."""
        np.savez(path, rows=np.ascontiguousarray(self.numpy(), dtype=np.float32))

    @staticmethod
    def load(path, device=None):
        rows = torch.from_numpy(np.asarray(np.load(path)["rows"], np.float32).reshape(-1, 5))
        return BoundSamples(rows if device is None else rows.to(device))

    @staticmethod
    def from_sdf(samples):
        """exact samples as intervals: lo = hi = sdf"""
        r = samples.rows
        if r.dim() != 2 or r.shape[1] != 4:
            raise ValueError("BoundSamples.from_sdf: sample rows must be [n][4] = x y z sdf")
        return BoundSamples(torch.cat([r, r[:, 3:4]], 1).contiguous())

    @staticmethod
    def concat(*sets):
        """the rows of several sets (BoundSamples, or SdfSamples taken through from_sdf) as one; they must share a device"""
        sets = [BoundSamples.from_sdf(s) if isinstance(s, SdfSamples) else s for s in (sets[0] if len(sets) == 1 and isinstance(sets[0], (list, tuple))
                                                                                      else sets)]
        if not sets:
            raise ValueError("BoundSamples.concat: nothing to join")
        return BoundSamples(torch.cat([s.rows.reshape(-1, 5) for s in sets]).contiguous())


@_lib.traced("view_samples_many")
def view_samples_many(params_list, clouds, normals=None, origin=(0.0, 0.0, 0.0), free_rows=4, eta=0.01, s_max=0.5, seed=0, _device=None):
    """Interval sample rows from what one sensor position sees of each shape.

    params_list, clouds: as verify.band_counts takes them -- per annotation the {'yaw', 'trans', 'scale', 'latent'} of the refinement and the
    camera-frame points [n][3] of its frustum.  normals: per annotation float64 [n][3] camera-frame normals (frame.lidar_normals), or None for
    no normal rows.  origin: the sensor's position in the camera frame.  Every point p goes to the lattice frame,
    x = diag(1, -1, 1) rot_yaw^T (p / scale - trans), and gives 3 + free_rows rows: x with [0, 0]; x +- eta n^ with [+-eta, +-eta] (n^ the
    normal taken to the lattice frame and normalised; left out where it is not finite or zero); and, for f < free_rows,
    x - s d^ with [0, s], d^ the unit vector from the sensor to x and s = ((f + u) / free_rows) min(s_max, |x - sensor|), u in [0, 1) from
    the library's hash of (seed, shape, point, f): one stratified draw per slot.  A row whose float32 position leaves [-1, 1]^3 is left out
    (position 0, NaN bounds).  eta and s_max are in lattice units and are taken as float32; see the module docstring for what the defaults
    are (eta: DeepSDF's only as recalled).  Returns a list of BoundSamples on the device, views of one array.  No host read and no
    synchronisation."""
    params_list, clouds = list(params_list), list(clouds)
    B, F = len(params_list), int(free_rows)
    if len(clouds) != B:
        raise ValueError("view_samples_many: %d parameter sets, %d clouds" % (B, len(clouds)))
    if normals is not None and len(normals) != B:
        raise ValueError("view_samples_many: %d parameter sets, %d normal arrays" % (B, len(normals)))
    _check_view("view_samples_many", B, F, eta, s_max)
    if B == 0:
        return []
    device = _device
    if device is None:
        device = next((c.device for c in clouds if torch.is_tensor(c) and c.is_cuda), None)
        if device is None:
            device = next((p[k].device for p in params_list for k in ("latent", "trans") if torch.is_tensor(p[k]) and p[k].is_cuda), None)
    dev = torch.device("cuda" if device is None else device)
    if dev.type != "cuda":
        raise _lib.SdfrError("view_samples_many runs on the GPU only; there is no CPU fallback")
    from .verify import _pose_rows
    return _view_rows("view_samples_many", "sdfr_view_samples", clouds, normals, origin, F, eta, s_max, seed, dev, (_pose_rows(params_list, dev)[0],))


def _check_view(who, B, F, eta, s_max):
    if not 0 <= F <= MAX_FREE:
        raise ValueError("%s: free_rows must be 0 .. %d (got %d)" % (who, MAX_FREE, F))
    if not (np.isfinite(eta) and np.isfinite(s_max) and s_max >= 0):
        raise ValueError("%s: eta must be finite, s_max finite and not negative" % who)
    if B > 65535:
        raise ValueError("%s: at most 65535 shapes per call" % who)


def _on_device(arrays, dtype, dev):
    """each of `arrays` (tensors or numpy) as a [n][3] tensor of `dtype` on the device, uploaded without waiting"""
    out = []
    for c in arrays:
        t = c.detach() if torch.is_tensor(c) else torch.from_numpy(np.ascontiguousarray(c, dtype=np.float32 if dtype == torch.float32 else np.float64))
        t = t.reshape(-1, 3).to(dtype)
        out.append(t if t.is_cuda else _upload(t, dev))
    return out


def _view_rows(who, call, clouds, normals, origin, F, eta, s_max, seed, dev, pose=()):
    """The sample rows of view_samples_many and align.align_samples_many: clouds and normals onto the device, the offset table, the C entry
    point `call` (`pose`: its pose rows, or none) and the BoundSamples, views of one array."""
    B = len(clouds)
    pts = _on_device(clouds, torch.float32, dev)
    sizes = [int(t.shape[0]) for t in pts]
    nrm = None
    if normals is not None:
        nrm = _on_device(normals, torch.float64, dev)
        for t, n in zip(nrm, sizes):
            if int(t.shape[0]) != n:
                raise ValueError("%s: %d normals for %d points" % (who, int(t.shape[0]), n))
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
        _lib.check(getattr(_lib.lib(), call)(Pt(points) if N else None, Pt(nrm) if (nrm is not None and N) else None, N, Pt(d_ptoff), B,
                                             *[Pt(p) for p in pose], Pt(org), 0, F, float(eta), float(s_max), int(seed) & 0x7FFFFFFFFFFFFFFF,
                                             Pt(rows) if N else None, Pt(flags), _lib.stream_ptr()), call)
    return [BoundSamples(rows[int(ptoff[b]) * Pn:int(ptoff[b + 1]) * Pn], flags[b]) for b in range(B)]


@_lib.traced("fit_many")
def fit_many(dsdf, samples, iters=800, rows_per_iter=8000, lr=5e-3, lr_step=None, lr_factor=0.1, clamp=0.1, code_reg=1e-4, unit_latents=True, init=None,
             seed=0, history=False, staging_bytes=STAGING_BYTES, draw=None, *, search=None):
    """encode.encode_many for interval samples: fit one latent per shape to `samples` (a list of BoundSamples, or one) under the frozen
    decoder.  The keywords, the staging, the random stream and the returned Encoded are encode_many's; the loss of a row is the distance from
    the clamped prediction to the clamped interval, `.flags` bit 1 (2) means no row with a finite prediction and usable bounds.  On
    BoundSamples.from_sdf(s) the results are encode_many's on s in every bit.

    search: None, or a dict for search.search_many -- `codes` (a codebook [C][L]), `keep` (default 3), `rows` (default rows_per_iter) --:
    the starts of every shape are scored and ranked first, the fit then runs on B x keep copies of the shapes from the kept starts (`init`
    with a search is refused), and search.choose returns, per shape, the copy whose fit ended with the lowest loss.  The Encoded then holds the chosen
    fits, `.found` the search.Found, `.chosen` int64 [B] the chosen rank (-1: none usable, rank 0 is returned) and `.fits` the Encoded of
    all B x keep fits, shape-major.  The cost is the scoring pass plus keep times the fit."""
    samples = [samples] if isinstance(samples, BoundSamples) else list(samples)
    if search is not None:
        if init is not None:
            raise ValueError("fit_many: give init or search, not both (with a search the fit starts from the found latents)")
        return _fit_searched(dsdf, samples, dict(search), dict(iters=iters, rows_per_iter=rows_per_iter, lr=lr, lr_step=lr_step, lr_factor=lr_factor,
                                                               clamp=clamp, code_reg=code_reg, unit_latents=unit_latents, seed=seed, history=history,
                                                               staging_bytes=staging_bytes, draw=draw))
    fit = _Fit("fit_many", "sdfr_bound_rows", "sdfr_bound_reduce", 5, "x y z lo hi", "BoundSamples.load(path, device)", samples, lr, init, seed)
    return Encoded(*_fit(fit, dsdf, iters, rows_per_iter, lr_step, lr_factor, clamp, code_reg, unit_latents, seed, history, staging_bytes, draw))


def _fit_searched(dsdf, samples, search, kw):
    """fit_many with search=: search.search_many, the fit of every kept start, search.choose"""
    from . import search as S
    if "codes" not in search or set(search) - {"codes", "keep", "rows"}:
        raise ValueError("fit_many: search must be a dict with 'codes' and, if wanted, 'keep' and 'rows' (got %r)" % (sorted(search),))
    keep = int(search.get("keep", 3))
    found = S.search_many(dsdf, samples, search["codes"], keep=keep, rows=int(search.get("rows", kw["rows_per_iter"])), clamp=kw["clamp"],
                          unit_latents=kw["unit_latents"], seed=kw["seed"], draw=kw["draw"], staging_bytes=kw["staging_bytes"])
    B = len(samples)
    fits = fit_many(dsdf, [samples[b] for b in range(B) for _ in range(keep)], init=found.latents.reshape(B * keep, -1), **kw)
    unusable = torch.full_like(fits.flags, BAD_TABLE)
    chosen = S.choose(fits.loss.reshape(B, keep), torch.where(found.valid.reshape(-1), fits.flags, unusable).reshape(B, keep))
    at = torch.arange(B, device=chosen.device) * keep + chosen.clamp(min=0)
    enc = Encoded(fits.latents[at], fits.raw_latents[at], fits.loss[at], fits.flags[at], None if fits.history is None else fits.history[:, at],
                  fits.unit_latents)
    enc.found, enc.chosen, enc.fits = found, chosen, fits
    return enc


def _cloud_normals(cloud, radius=1.0, max_nn=30):
    """frame.lidar_normals of one annotation's cloud among its own points, float64 [n][3] on the device; a point with fewer than 3
    neighbours gets a NaN normal (lidar_normals' placeholder (0, 0, 1) would be taken for a measurement).  No host synchronisation."""
    from .frame import lidar_normals
    n, info = lidar_normals(cloud, radius=radius, max_nn=max_nn, return_info=True)
    return torch.where((info["nn_count"] < 3)[:, None], torch.full_like(n, float("nan")), n)


@_lib.traced("complete_many")
def complete_many(dsdf, params_list, clouds, normals=None, origin=(0.0, 0.0, 0.0), free_rows=4, eta=0.01, s_max=0.5, seed=0, *, search=None, **fit_kw):
    """A latent per annotation from its lidar cloud alone: view_samples_many, then fit_many.  params_list gives the pose (and, as the default
    `init`, the latent the fit starts from); normals=None estimates them with frame.lidar_normals on each cloud (NaN where a
    point has fewer than 3 neighbours, so its normal rows are left out).  fit_kw: fit_many's keywords.  search: fit_many's -- the start then
    comes from the scored codebook and not from the parameters' latent.  Returns the Encoded, with the rows as `.samples`."""
    params_list, clouds = list(params_list), list(clouds)
    dev = next(dsdf.parameters()).device
    if dev.type != "cuda":
        raise _lib.SdfrError("complete_many runs on the GPU only (the decoder is on %s); there is no CPU fallback" % dev)
    if normals is None:
        normals = [_cloud_normals(c if torch.is_tensor(c) else torch.from_numpy(np.ascontiguousarray(c, dtype=np.float32)).to(dev)) if len(c) else
                   torch.zeros((0, 3), dtype=torch.float64, device=dev) for c in clouds]
    samples = view_samples_many(params_list, clouds, normals, origin, free_rows, eta, s_max, seed, _device=dev)
    if search is not None:
        fit_kw["search"] = search
    elif fit_kw.get("init") is None and params_list:
        from .verify import _pose_rows
        fit_kw["init"] = _pose_rows(params_list, dev)[1]
    fit_kw.setdefault("seed", seed)
    enc = fit_many(dsdf, samples, **fit_kw)
    enc.samples = samples
    return enc


def _latent_cosine(a, b):
    """float64 [B] on the device: the cosine between the rows of a and b"""
    a, b = a.double(), b.double()
    return (torch.nn.functional.normalize(a, dim=1) * torch.nn.functional.normalize(b, dim=1)).sum(1)
