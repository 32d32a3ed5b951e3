"""Encoding shapes under a trained shape prior: DeepSDF's "reconstruct" step, batched on the device (csrc/encode.hip).

    from sdflabel_amd.encode import encode_many, encode_meshes

The decoder is frozen; one latent per shape is fitted to the shape's SDF samples with Adam.  Per iteration, for all shapes of a staged group
at once: sdfr_encode_rows draws the rows and writes the decoder's inputs, the decoder runs forward with its ReLU masks saved, sdfr_mlp_jacobian
turns the masks into d sdf / d input (its first L columns are d sdf / d latent), sdfr_encode_reduce forms one clamped-L1 loss and one latent
gradient per shape, sdfr_encode_step takes the gradient through the unit normalisation and applies Adam.  Nothing is read back in the loop.

THE DEFAULTS ARE DeepSDF's RECONSTRUCTION SETTINGS AS RECALLED -- 800 iterations, 8 000 rows per iteration, learning rate 5e-3 cut by ten
halfway, clamp 0.1, latent regulariser 1e-4, start drawn from N(0, 0.01).  They are parameters; they have not been checked against that
paper's code.  The rows are drawn from the library's own random stream (an integer hash of seed, iteration, shape and row), not torch's.

unit_latents=True (the default here): the decoder is fed z / ||z||, for the reason pipelines.train_prior.PriorTrainer gives -- the refinement
normalises the latent before the decoder and the CSS head projects its latent onto the unit sphere; the regulariser is then off.

_fit is the one driver of the frozen-decoder fits: complete.fit_many, align.align_many and track.align_tracks hand it a _Fit of their own.
"""
import torch

from . import _lib
from .mesh import STAGING_BYTES, _decoder_mode, decoder_rows
from .sdf_samples import SdfSamples

EMPTY, NO_ROWS, SKIPPED, BAD_TABLE = 1, 2, 4, 8            # Encoded.flags (csrc/encode_cells.h)
MAX_ROWS = 1 << 20
MAX_ITERS = 1 << 24


class Encoded:
    """`.latents` float32 [B][L]: the latents as the decoder sees them (normalised with unit_latents) -- what meshes_many, prior_residuals,
    synth.draw_scenes and the refinement take.  `.raw_latents` float32 [B][L]: the optimised variables.  `.loss` float64 [B]: each shape's
    clamped-L1 loss on the rows of the last iteration, before that iteration's step (NaN with iters = 0).  `.flags` int32 [B] of the last
    iteration: 1 the shape has no samples, 2 no row with a finite prediction and target, 4 the latent was not stepped, 8 a broken offset-table
    entry (encode_many builds the table itself, so it does not occur here).  `.history` float32
    [iters][B] or None.  All on the device.  `.samples`: the list of SdfSamples encode_meshes drew (None from encode_many)."""

    def __init__(self, latents, raw_latents, loss, flags, history, unit_latents):
        self.latents, self.raw_latents, self.loss, self.flags, self.history = latents, raw_latents, loss, flags, history
        self.unit_latents = unit_latents
        self.samples = None
        self.found = self.chosen = self.fits = None        # complete.fit_many(search=...): the search.Found, the chosen rank, every kept start's fit


def _upload(host, device):
    """host tensor -> device without waiting (pinned staging, asynchronous copy on the current stream)"""
    return host.contiguous().pin_memory().to(device, non_blocking=True)


class _Fit:
    """What a fit hands _fit.  This one is a latent fit to samples of `width` floats, x y z and width - 3 target words: rows_call writes the
    decoder's inputs and one array per target word, reduce_call takes the decoder's values and those arrays, sdfr_encode_step steps the
    latent.  align.py's subclass adds a pose."""
    step_call, ws_call = "sdfr_encode_step", "sdfr_encode_ws_bytes"
    extra = 0                                      # gradient columns beyond the latent's

    def __init__(self, who, rows_call, reduce_call, width, layout, loader, samples, lr, init, seed):
        self.who, self.rows_call, self.reduce_call, self.width, self.layout, self.loader = who, rows_call, reduce_call, width, layout, loader
        self.samples, self.lr, self.init, self.seed = samples, float(lr), init, seed
        self.row_floats = width - 3                # float32 words a row of the side arrays
        self.B = len(samples)

    def check(self, Ld):
        """the fit's own argument checks: nothing here touches the device"""
        if self.init is not None:
            self.init = torch.as_tensor(self.init)
            if self.init.dim() != 2 or tuple(self.init.shape) != (self.B, Ld):
                raise ValueError("%s: init must be [%d][%d] (shapes x the decoder's latent size), got %s" % (self.who, self.B, Ld, tuple(self.init.shape)))
        self.check_rows()

    def check_rows(self):
        for s in self.samples:
            if s.rows.dim() != 2 or s.rows.shape[1] != self.width:
                raise ValueError("%s: sample rows must be [n][%d] = %s" % (self.who, self.width, self.layout))

    def start(self, dev, Ld):
        """the start latents [B][Ld] on the device, a tensor of the fit's own; self.samples are final after this"""
        if self.init is None:
            return _upload(torch.randn((self.B, Ld), generator=torch.Generator().manual_seed(int(self.seed)), dtype=torch.float32) * 0.1, dev)
        return self.init.detach().to(dev).float().clone().contiguous()

    def alloc(self, n_max, dev):
        """the side arrays of a staged group"""
        self.sides = [torch.empty((n_max,), dtype=torch.float32, device=dev) for _ in range(self.row_floats)]

    def group(self, b0, inputs, J, NI):
        """for the shapes from b0 on: the rows call's arguments between `unit` and `zn` in the loop and in the closing call, the reduce's
        between `pred` and `L`, the step's between `unit` and `g`"""
        t = tuple(_lib.ptr(a) for a in self.sides)
        return (inputs,) + t, (None,) * (1 + len(t)), t + (J, NI), ()

    def rates(self, f):
        """the step's learning-rate arguments on an iteration whose schedule factor is f"""
        return (self.lr * f,)

    def group_size(self, nb):
        """shapes of a staged group at the most, from the number the staging buffers allow"""
        return nb

    def groups(self, nb):
        """the staged groups as (first shape, shapes): whole shapes, in order"""
        return [(b0, min(nb, self.B - b0)) for b0 in range(0, self.B, nb)]

    def step(self, step_fn, b0, n, z, m, v, Ld, unit, step_mid, g, loss, flags, code_reg, rates, t, hist, B, st):
        """the step call of the group's n shapes from b0 on (z, m, v, loss, flags, hist: pointers at shape b0)"""
        return step_fn(z, m, v, Ld, n, unit, *step_mid, g, loss, flags, code_reg, *rates, t, hist, B, st)


@_lib.traced("encode_many")
def encode_many(dsdf, samples, iters=800, rows_per_iter=8000, lr=5e-3, lr_step=None, lr_factor=0.1, clamp=0.1, code_reg=1e-4, unit_latents=True,
                init=None, seed=0, history=False, staging_bytes=STAGING_BYTES, draw=None):
    """Fit one latent per shape to `samples` (a list of SdfSamples, or one) under the frozen decoder `dsdf`.  See the module docstring for the
    defaults.  The decoder's mlp_precision picks the forward kernel (exact float32, float16 or split), as in meshes_many.

    lr_step: the learning rate is lr * lr_factor ** (iteration // lr_step); default iters // 2.  init: [B][L] start latents, or N(0, 0.01)
    from a host torch.Generator seeded with `seed`.  draw: None draws rows_per_iter rows per shape and iteration with replacement, unless every
    shape with samples has the same number n <= rows_per_iter of them -- then every iteration takes every row, in order; True always draws;
    False takes the first min(rows_per_iter, smallest count) rows of every shape on every iteration.  Shapes are staged in groups of whole
    shapes whose buffers stay under staging_bytes; the buffers are allocated once.  iters = 0 returns the start.  Returns an Encoded."""
    samples = [samples] if isinstance(samples, SdfSamples) else list(samples)
    fit = _Fit("encode_many", "sdfr_encode_rows", "sdfr_encode_reduce", 4, "x y z sdf", "SdfSamples.load(path, device)", samples, lr, init, seed)
    return Encoded(*_fit(fit, dsdf, iters, rows_per_iter, lr_step, lr_factor, clamp, code_reg, unit_latents, seed, history, staging_bytes, draw))


def _fit(fit, dsdf, iters, rows_per_iter, lr_step, lr_factor, clamp, code_reg, unit_latents, seed, history, staging_bytes, draw):
    """The loop of encode_many, complete.fit_many, align.align_many and track.align_tracks over what `fit` (a _Fit) says of them.  Returns (latents, raw latents,
    loss, flags, history, unit_latents)."""
    who, B = fit.who, fit.B
    iters, k_req = int(iters), int(rows_per_iter)
    if iters < 0 or iters >= MAX_ITERS:
        raise ValueError("%s: iters must be 0 .. 2^24 - 1 (got %d)" % (who, iters))
    if k_req < 1:
        raise ValueError("%s: rows_per_iter must be at least 1 (got %d)" % (who, k_req))
    if not float(clamp) > 0:
        raise ValueError("%s: clamp must be positive" % who)
    if lr_step is not None and int(lr_step) < 1:
        raise ValueError("%s: lr_step must be at least 1" % who)
    Ld = int(dsdf.latent_size)
    if not 1 <= Ld <= 256:
        raise ValueError("%s: latent sizes 1 .. 256 (the decoder's is %d)" % (who, Ld))
    if B > 65535:
        raise ValueError("%s: at most 65535 shapes per call" % who)
    fit.check(Ld)
    dev = next(dsdf.parameters()).device
    if dev.type != "cuda":
        raise _lib.SdfrError("%s runs on the GPU only (the decoder is on %s); there is no CPU fallback" % (who, dev))
    z = fit.start(dev, Ld)
    samples = fit.samples
    for s in samples:
        if not s.rows.is_cuda:
            raise _lib.SdfrError("%s: the sample rows must be on the GPU (%s)" % (who, fit.loader))
    counts = [len(s) for s in samples]
    full = [c for c in counts if c > 0]
    if draw is None:
        draw = not (full and min(full) == max(full) and full[0] <= k_req)
    k = k_req if draw else min([k_req] + full)
    if k > MAX_ROWS:
        raise ValueError("%s: at most 2^20 rows per shape and iteration" % who)
    lr_step = max(1, iters // 2) if lr_step is None else int(lr_step)

    zn = torch.empty_like(z)
    loss = torch.full((B,), float("nan"), dtype=torch.float64, device=dev)
    flags = torch.zeros((B,), dtype=torch.int32, device=dev)
    hist = torch.zeros((iters, B), dtype=torch.float32, device=dev) if history else None
    out = (zn, z, loss, flags, hist, bool(unit_latents))
    if B == 0:
        return out

    L = _lib.lib()
    rows_fn, reduce_fn, step_fn = getattr(L, fit.rows_call), getattr(L, fit.reduce_call), getattr(L, fit.step_call)
    P, ck = _lib.ptr, _lib.check
    handle, fwd, f16 = _decoder_mode(dsdf, dev)
    NI = Ld + 3
    rows = torch.cat([s.rows for s in samples]).float().contiguous() if sum(counts) else torch.zeros((0, fit.width), dtype=torch.float32, device=dev)
    S = int(rows.shape[0])
    off = [0]
    for c in counts:
        off.append(off[-1] + c)
    soff = _upload(torch.tensor(off, dtype=torch.int64), dev)
    mask_words = 0 if handle.has_ln else int(L.sdfr_decoder_mask_words(handle.h, k))
    per_shape = k * (4 * (2 * NI + 2 + fit.row_floats)) + 4 * mask_words
    nb = fit.group_size(max(1, min(B, int(staging_bytes) // max(per_shape, 1))))
    groups = fit.groups(nb)
    n_max = nb * k
    inputs = torch.empty((n_max, NI), dtype=torch.float32, device=dev)
    J = torch.empty((n_max, NI), dtype=torch.float32, device=dev)
    fit.alloc(n_max, dev)
    pred, sel = (torch.empty((n_max,), dtype=torch.float32, device=dev) for _ in range(2))
    idx = torch.arange(n_max, dtype=torch.int32, device=dev)
    masks = None if handle.has_ln else torch.empty((int(L.sdfr_decoder_mask_words(handle.h, n_max)),), dtype=torch.int32, device=dev)
    ws_bytes = int(getattr(L, fit.ws_call)(nb, k, Ld))
    ws = torch.empty((ws_bytes // 8,), dtype=torch.float64, device=dev)
    g = torch.empty((nb, Ld + fit.extra), dtype=torch.float64, device=dev)
    m, v = torch.zeros_like(z), torch.zeros_like(z)
    cnts = {n: torch.full((1,), n * k, dtype=torch.int32, device=dev) for n in {n for _, n in groups}}
    unit = 1 if unit_latents else 0
    table_flags = torch.empty((nb,), dtype=torch.int32, device=dev)          # the last call's flag output when the loop's flags are kept
    seed64 = int(seed) & 0x7FFFFFFFFFFFFFFF
    with _lib.guard(dev):
        st = _lib.stream_ptr()
        for b0, n in groups:
            zg, so, znb, lb, fb = P(z[b0:]), P(soff[b0:]), P(zn[b0:]), P(loss[b0:]), P(flags[b0:])
            hb = P(hist[:, b0:]) if hist is not None else None
            rows_mid, rows_end, reduce_mid, step_mid = fit.group(b0, P(inputs), P(J), NI)
            for it in range(iters):
                ck(rows_fn(P(rows), S, so, n, b0, k, 1 if draw else 0, seed64, it, zg, Ld, unit, *rows_mid, znb, fb, st), fit.rows_call)
                decoder_rows(handle, fwd, f16, inputs, n * k, pred, J, sel, masks, idx, cnts[n], st)
                ck(reduce_fn(P(pred), *reduce_mid, Ld, n, k, float(clamp), P(ws), ws_bytes, lb, P(g), fb, st), fit.reduce_call)
                ck(fit.step(step_fn, b0, n, zg, P(m[b0:]), P(v[b0:]), Ld, unit, step_mid, P(g), lb, fb, float(code_reg),
                            fit.rates(float(lr_factor) ** (it // lr_step)), it + 1, hb, B, st), fit.step_call)
            # the latents as the decoder sees the final z (and, with iters = 0, the flags of the table)
            ck(rows_fn(None, S, so, n, b0, k, 0, seed64, 0, zg, Ld, unit, *rows_end, znb, fb if iters == 0 else P(table_flags), st), fit.rows_call)
    return out


def encode_meshes(dsdf, meshes, n=500000, generator=None, **kw):
    """draw_sdf_samples(meshes, n, generator) followed by encode_many(dsdf, samples, **kw): the meshes in the lattice frame (sdf_samples.fit_frame /
    normalize), a host torch.Generator for the draw.  Returns the Encoded, with the drawn samples as `.samples`."""
    from .sdf_samples import draw_sdf_samples
    samples = draw_sdf_samples(meshes, n=n, generator=generator)
    enc = encode_many(dsdf, samples, **kw)
    enc.samples = samples
    return enc
