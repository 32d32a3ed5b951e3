"""Choosing the start of a frozen-decoder fit on the device: scored codebooks (csrc/search.hip).

    from sdflabel_amd.search import sphere_codes, score_many, search_many, choose

encode, complete, align and track are LOCAL fits: from a far start they end in another minimum (profiles/complete_notes.md: from the
antipodal latent the completion ends at cosine -0.18 to the true latent).  More iterations do not help; a better start does.  A START is a
candidate (latent, pose) for one shape, and many starts share one shape's samples.  score_many scores all starts of all shapes on the SAME
drawn rows per shape -- sdfr_search_rows, the decoder's forward alone (no Jacobian, no saved masks, no optimiser step), sdfr_search_reduce --,
search_many crosses every shape with a codebook and ranks the starts per shape on the device (sdfr_search_select), and choose picks, after
the fits, the start whose fit ended lowest.  complete.fit_many / complete_many take it all as `search=dict(codes=..., keep=3, rows=2000)`;
search_poses does the same for the pose-and-shape fit (codes x yaw offsets on a rough box), and align.align_many and
pipelines.scan.label_scan take it as `search=dict(codes=..., yaws=..., keep=2)`.

The rows a start is scored on are the rows the fit draws on its first iteration with the same seed: the draw's hash takes the SHAPE, not the
start, so the losses of a shape's starts are losses of the same rows and can be compared.

NOTHING IS CLAIMED about an operating point: keep, rows and the size of the codebook are parameters.  Nothing here reads the device back
or synchronises with it.
"""
import math

import torch

from . import _lib
from .encode import _upload
from .mesh import STAGING_BYTES, _decoder_mode

MAX_KEEP, MAX_STARTS = 64, 4096                   # csrc/search_cells.h
UNUSABLE = 1 | 2 | 8 | 16                         # flags that keep a start from being ranked: no samples, no ok row, a broken table, a bad pose
GOLDEN_ANGLE = math.pi * (3.0 - math.sqrt(5.0))


class Scores:
    """`.loss` float64 [N]: each start's interval loss on its shape's drawn rows (0 for a start without an ok row).  `.flags` int32 [N]: the
    bits of the fits' flags -- 1 no samples, 2 no ok row, 8 a broken table entry or an owner outside the shapes, 16 an unusable pose.
    `.zn` float32 [N][L]: the latents as the decoder saw them.  All on the device."""

    def __init__(self, loss, flags, zn):
        self.loss, self.flags, self.zn = loss, flags, zn


class Found:
    """`.order` int32 [B][keep]: the start (an index into the scored starts) of rank r of shape b, -1 beyond `.count` int32 [B] (the usable
    starts of the shape, at most keep; -1 for a broken table entry).  `.loss` float64 [B][keep]: their scores, NaN beyond count.  `.latents`
    float32 [B][keep][L]: their latents as given (raw: what a fit takes as `init`); beyond count the shape's first start, so that a fit of
    every rank runs on something -- choose() leaves such ranks out by their flags.  `.valid` bool [B][keep].  `.scores`: the Scores of all
    starts.  From search_poses also `.theta` float32 [B][keep][5] = yaw, tx, ty, tz, scale of the kept starts, `.params`: per shape a list of
    keep refinement-shaped dicts {'yaw', 'trans', 'scale', 'latent'} (views of theta and latents: what align.align_many takes), and
    `.samples`: the observation rows the starts were scored on.  All on the device."""

    def __init__(self, order, count, loss, latents, valid, scores, theta=None, samples=None):
        self.order, self.count, self.loss, self.latents, self.valid, self.scores = order, count, loss, latents, valid, scores
        self.theta, self.samples, self.params = theta, samples, None
        if theta is not None:
            self.params = [[{"yaw": theta[b, r, 0:1], "trans": theta[b, r, 1:4], "scale": theta[b, r, 4:5], "latent": latents[b, r]}
                            for r in range(int(theta.shape[1]))] for b in range(int(theta.shape[0]))]


def sphere_codes(L, C, seed=0):
    """C unit rows of size L, float32 [C][L] on the host: a codebook for search_many.  L == 3: the Fibonacci lattice, deterministic (seed is
    not used) -- for i < C, in float64, z = 1 - (2 i + 1) / C, r = sqrt(1 - z z), phi = i pi (3 - sqrt(5)), code_i = (r cos phi, r sin phi, z),
    rounded to float32 and normalised once more there.  Any other L: standard normal draws from a host torch.Generator seeded with `seed`,
    normalised.  Any [C][L] tensor is a codebook too -- a saved prior's latents, for instance."""
    L, C = int(L), int(C)
    if L < 1 or C < 1:
        raise ValueError("sphere_codes: L and C must be at least 1 (got %d, %d)" % (L, C))
    if L == 3:
        i = torch.arange(C, dtype=torch.float64)
        z = 1.0 - (2.0 * i + 1.0) / C
        r = torch.sqrt(1.0 - z * z)
        phi = i * GOLDEN_ANGLE
        codes = torch.stack([r * torch.cos(phi), r * torch.sin(phi), z], 1).float()
    else:
        codes = torch.randn((C, L), generator=torch.Generator().manual_seed(int(seed)), dtype=torch.float32)
    return torch.nn.functional.normalize(codes, dim=1)


def yaw_offsets(H):
    """H yaw offsets 2 pi h / H, float32 [H] on the host"""
    if int(H) < 1:
        raise ValueError("yaw_offsets: H must be at least 1")
    return (2.0 * math.pi * torch.arange(int(H), dtype=torch.float64) / int(H)).float()


def pose_rows(theta):
    """pose rows [N][6] = cos(yaw), sin(yaw), trans, scale from theta [N][5] = yaw, tx, ty, tz, scale, as sdfr_align_step writes them: cos
    and sin in double of the float32 yaw, rounded once"""
    theta = theta.float()
    return torch.cat([torch.cos(theta[:, :1].double()).float(), torch.sin(theta[:, :1].double()).float(), theta[:, 1:]], 1).contiguous()


def _draw_and_k(samples, rows, draw):
    """encode._fit's rule: draw unless every shape with samples has the same number n <= rows of them"""
    full = [len(s) for s in samples if len(s) > 0]
    if draw is None:
        draw = not (full and min(full) == max(full) and full[0] <= rows)
    return bool(draw), (rows if draw else min([rows] + full))


@_lib.traced("score_many")
def score_many(dsdf, samples, latents, own, poses=None, rows=2000, clamp=0.1, unit_latents=True, seed=0, draw=None, staging_bytes=STAGING_BYTES):
    """The interval loss of N starts under the frozen decoder `dsdf`, forward only.

    samples: a list of B BoundSamples -- lattice-frame rows (complete.view_samples_many) with poses=None, else the camera-frame observation
    rows of align.align_samples_many.  latents [N][L]: each start's latent; own [N]: the shape each start belongs to; poses [N][6]: each
    start's pose row (pose_rows), then the loss is that of the metric prediction scale * sdf, clamp in metres.  rows, clamp, unit_latents,
    seed, draw: as the fit takes rows_per_iter and the others; a start is scored on the rows its shape's fit draws on iteration 0.  The
    starts are staged in groups under staging_bytes -- a group may end anywhere --, the buffers are allocated once, and there is no host
    read and no synchronisation.  The decoder's own mode (exact float32, float16, split, LayerNorm) runs the forward.  Returns a Scores."""
    samples = list(samples)
    B, k_req = len(samples), int(rows)
    if k_req < 1:
        raise ValueError("score_many: rows must be at least 1 (got %d)" % k_req)
    if not float(clamp) > 0:
        raise ValueError("score_many: clamp must be positive")
    if B > 65535:
        raise ValueError("score_many: at most 65535 shapes per call")
    Ld = int(dsdf.latent_size)
    latents = torch.as_tensor(latents)
    if latents.dim() != 2 or int(latents.shape[1]) != Ld:
        raise ValueError("score_many: latents must be [N][%d] (starts x the decoder's latent size), got %s" % (Ld, tuple(latents.shape)))
    N = int(latents.shape[0])
    if N > 65535:
        raise ValueError("score_many: at most 65535 starts per call")
    own = torch.as_tensor(own)
    if own.dim() != 1 or int(own.shape[0]) != N or own.dtype.is_floating_point:
        raise ValueError("score_many: own must hold one shape index per start")
    poses = None if poses is None else torch.as_tensor(poses)
    if poses is not None and (poses.dim() != 2 or tuple(poses.shape) != (N, 6)):
        raise ValueError("score_many: poses must be [%d][6] = cos(yaw), sin(yaw), trans, scale" % N)
    for s in samples:
        if s.rows.dim() != 2 or s.rows.shape[1] != 5:
            raise ValueError("score_many: sample rows must be [n][5] = x y z lo hi")
    dev = next(dsdf.parameters()).device
    if dev.type != "cuda":
        raise _lib.SdfrError("score_many runs on the GPU only (the decoder is on %s); there is no CPU fallback" % dev)
    for s in samples:
        if not s.rows.is_cuda:
            raise _lib.SdfrError("score_many: the sample rows must be on the GPU (BoundSamples.load(path, device))")
    draw, k = _draw_and_k(samples, k_req, draw)
    if k > (1 << 20):
        raise ValueError("score_many: at most 2^20 rows per start")

    def on_dev(t, dtype):
        t = t.detach().to(dtype).contiguous()
        return t if t.is_cuda else _upload(t, dev)

    z, d_own = on_dev(latents, torch.float32), on_dev(own, torch.int32)
    pose = None if poses is None else on_dev(poses, torch.float32)
    zn = torch.empty_like(z)
    loss = torch.zeros((N,), dtype=torch.float64, device=dev)
    flags = torch.zeros((N,), dtype=torch.int32, device=dev)
    out = Scores(loss, flags, zn)
    if N == 0:
        return out
    L = _lib.lib()
    P, ck = _lib.ptr, _lib.check
    handle, fwd, _ = _decoder_mode(dsdf, dev)
    NI = Ld + 3
    counts = [len(s) for s in samples]
    srows = torch.cat([s.rows for s in samples]).float().contiguous() if sum(counts) else torch.zeros((0, 5), dtype=torch.float32, device=dev)
    S = int(srows.shape[0])
    off = [0]
    for c in counts:
        off.append(off[-1] + c)
    soff = _upload(torch.tensor(off, dtype=torch.int64), dev)
    ng = max(1, min(N, int(staging_bytes) // max(4 * k * (NI + 3), 1)))
    inputs = torch.empty((ng * k, NI), dtype=torch.float32, device=dev)
    pred, lo, hi = (torch.empty((ng * k,), dtype=torch.float32, device=dev) for _ in range(3))
    ws_bytes = int(L.sdfr_search_ws_bytes(ng, k))
    ws = torch.empty((ws_bytes // 8,), dtype=torch.float64, device=dev)
    seed64 = int(seed) & 0x7FFFFFFFFFFFFFFF
    with _lib.guard(dev):
        st = _lib.stream_ptr()
        for s0 in range(0, N, ng):
            n = min(ng, N - s0)
            ps = None if pose is None else P(pose[s0:])
            ck(L.sdfr_search_rows(P(srows) if S else None, S, P(soff), B, P(d_own[s0:]), n, 0, k, 1 if draw else 0, seed64, 0, P(z[s0:]), Ld,
                                  1 if unit_latents else 0, ps, P(inputs), None, P(lo), P(hi), P(zn[s0:]), P(flags[s0:]), st), "sdfr_search_rows")
            ck(fwd(handle.h, P(inputs), n * k, P(pred), None, st), fwd.__name__)
            ck(L.sdfr_search_reduce(P(pred), P(lo), P(hi), ps, n, k, float(clamp), P(ws), ws_bytes, P(loss[s0:]), P(flags[s0:]), st), "sdfr_search_reduce")
    return out


def select(loss, flags, coff, keep):
    """sdfr_search_select on device tensors: loss float64 [N], flags int32 [N], coff int64 [B + 1] -> (order int32 [B][keep], count int32 [B])"""
    keep = int(keep)
    if not 1 <= keep <= MAX_KEEP:
        raise ValueError("search: keep must be 1 .. %d (got %d)" % (MAX_KEEP, keep))
    if not (loss.is_cuda and flags.is_cuda and coff.is_cuda):
        raise _lib.SdfrError("search runs on the GPU only; there is no CPU fallback")
    loss, flags, coff = loss.to(torch.float64).contiguous(), flags.to(torch.int32).contiguous(), coff.to(torch.int64).contiguous()
    B, N = int(coff.shape[0]) - 1, int(loss.shape[0])
    if B < 0 or int(flags.shape[0]) != N:
        raise ValueError("search: coff must hold B + 1 entries, and flags one word per loss")
    order = torch.empty((B, keep), dtype=torch.int32, device=loss.device)
    count = torch.empty((B,), dtype=torch.int32, device=loss.device)
    with _lib.guard(loss.device):
        _lib.check(_lib.lib().sdfr_search_select(_lib.ptr(loss) if N else None, _lib.ptr(flags) if N else None, _lib.ptr(coff), B, N, keep, _lib.ptr(order),
                                                 _lib.ptr(count), _lib.stream_ptr()), "sdfr_search_select")
    return order, count


def _found(scores, starts, coff, keep, theta=None, samples=None):
    """the Found of `scores` over the table coff: the select, and the gathers with torch ops on the device"""
    order, count = select(scores.loss, scores.flags, coff, keep)
    valid = torch.arange(int(keep), device=order.device)[None, :] < count[:, None]
    idx = torch.where(valid, order.long(), coff[:-1, None].expand(-1, int(keep)))
    loss = torch.where(valid, scores.loss[idx], torch.full_like(scores.loss[idx], float("nan")))
    return Found(order, count, loss, starts[idx], valid, scores, None if theta is None else theta[idx], samples)


@_lib.traced("search_many")
def search_many(dsdf, samples, codes, keep=1, **score_kw):
    """Every shape of `samples` (a list of BoundSamples in the lattice frame) crossed with every row of the codebook `codes` [C][L]: score_many
    on the B C starts (score_kw: its keywords), the ranking per shape on the device, and the best `keep` starts of every shape as a Found.
    No host read and no synchronisation."""
    samples = list(samples)
    codes = torch.as_tensor(codes)
    if codes.dim() != 2 or int(codes.shape[0]) < 1:
        raise ValueError("search_many: codes must be [C][L] with C >= 1, got %s" % (tuple(codes.shape),))
    B, C = len(samples), int(codes.shape[0])
    if C > MAX_STARTS:
        raise ValueError("search_many: at most %d codes" % MAX_STARTS)
    if not 1 <= int(keep) <= MAX_KEEP:
        raise ValueError("search: keep must be 1 .. %d (got %d)" % (MAX_KEEP, int(keep)))
    if B * C > 65535:
        raise ValueError("search_many: at most 65535 starts per call (%d shapes x %d codes)" % (B, C))
    dev = next(dsdf.parameters()).device
    codes = codes.detach().float().contiguous()
    codes = codes if codes.is_cuda else _upload(codes, dev)
    starts = codes.repeat(B, 1)
    own = _upload(torch.arange(B, dtype=torch.int32).repeat_interleave(C), dev)
    coff = _upload(torch.arange(B + 1, dtype=torch.int64) * C, dev)
    scores = score_many(dsdf, samples, starts, own, **score_kw)
    return _found(scores, starts, coff, keep)


@_lib.traced("search_poses")
def search_poses(dsdf, params_list, clouds, codes, yaws=(0.0, math.pi), keep=2, normals=None, samples=None, origin=(0.0, 0.0, 0.0), free_rows=4, eta=0.02,
                 s_max=1.0, seed=0, rows=2000, clamp=0.2, **score_kw):
    """search_many for the pose-and-shape fit (align.align_many): the starts of every shape are the codebook `codes` [C][L] crossed with the
    yaw offsets `yaws` [H] added to the rough box's yaw (float32), trans and scale taken from the box -- C H starts a shape, code-major.
    params_list: per shape the rough {'yaw', 'trans', 'scale', 'latent'} (its latent is not used); clouds, normals, origin, free_rows, eta,
    s_max, seed: align.align_samples_many's (normals=None estimates them as align_many does), or samples: rows made before.  rows, clamp
    (metres) and score_kw (unit_latents, draw, staging_bytes): score_many's.  Returns a Found with `.theta`, `.params` and `.samples`.
    No host read and no synchronisation."""
    from . import align as A
    from .verify import _pose_rows
    params_list = list(params_list)
    B = len(params_list)
    codes = torch.as_tensor(codes)
    if codes.dim() != 2 or int(codes.shape[0]) < 1:
        raise ValueError("search_poses: codes must be [C][L] with C >= 1, got %s" % (tuple(codes.shape),))
    yaws = torch.as_tensor(yaws, dtype=torch.float32).reshape(-1)
    C, H = int(codes.shape[0]), int(yaws.shape[0])
    if H < 1 or C * H > MAX_STARTS:
        raise ValueError("search_poses: between 1 and %d starts a shape (%d codes x %d yaws)" % (MAX_STARTS, C, H))
    if not 1 <= int(keep) <= MAX_KEEP:
        raise ValueError("search: keep must be 1 .. %d (got %d)" % (MAX_KEEP, int(keep)))
    if B * C * H > 65535:
        raise ValueError("search_poses: at most 65535 starts per call (%d shapes x %d codes x %d yaws)" % (B, C, H))
    dev = next(dsdf.parameters()).device
    if dev.type != "cuda":
        raise _lib.SdfrError("search_poses runs on the GPU only (the decoder is on %s); there is no CPU fallback" % dev)
    if samples is None:
        samples = A._make_samples(list(clouds), normals, origin, int(free_rows), eta, s_max, seed, dev)
    samples = list(samples)
    if len(samples) != B:
        raise ValueError("search_poses: %d parameter sets, %d sample sets" % (B, len(samples)))
    Ld = int(codes.shape[1])
    codes = codes.detach().float().contiguous()
    codes = codes if codes.is_cuda else _upload(codes, dev)
    yaws = yaws if yaws.is_cuda else _upload(yaws, dev)
    if B == 0:
        z = torch.zeros((0, Ld), dtype=torch.float32, device=dev)
        sc = Scores(torch.zeros((0,), dtype=torch.float64, device=dev), torch.zeros((0,), dtype=torch.int32, device=dev), z)
        e = torch.zeros((0, int(keep)), device=dev)
        return Found(e.int(), torch.zeros((0,), dtype=torch.int32, device=dev), e.double(), z.reshape(0, int(keep), Ld), e.bool(), sc,
                     torch.zeros((0, int(keep), 5), dtype=torch.float32, device=dev), samples)
    pose0, _ = _pose_rows(params_list, dev)
    yaw_l = [torch.as_tensor(p["yaw"]).detach().reshape(-1)[:1].to(torch.float32) for p in params_list]
    yaw = torch.stack(yaw_l) if all(y.is_cuda for y in yaw_l) else _upload(torch.stack([y.cpu() for y in yaw_l]), dev)
    base = torch.cat([yaw.to(dev), pose0[:, 2:]], 1)                                                   # [B][5], as align_many starts
    theta = base[:, None, None, :].repeat(1, C, H, 1)
    theta[..., 0] = theta[..., 0] + yaws[None, None, :]
    theta = theta.reshape(B * C * H, 5).contiguous()
    starts = codes[None, :, None, :].expand(B, C, H, Ld).reshape(B * C * H, Ld).contiguous()
    own = _upload(torch.arange(B, dtype=torch.int32).repeat_interleave(C * H), dev)
    coff = _upload(torch.arange(B + 1, dtype=torch.int64) * (C * H), dev)
    scores = score_many(dsdf, samples, starts, own, poses=pose_rows(theta), rows=rows, clamp=clamp, seed=seed, **score_kw)
    return _found(scores, starts, coff, keep, theta, samples)


def choose(loss, flags):
    """The rank whose fit ended lowest: loss float64 [B][keep] and flags int32 [B][keep] of the fits of every shape's kept starts -> int64 [B]
    on the device.  A NaN loss or a flagged start (bits 0, 1, 3, 4) loses, the first wins a tie; -1 where no rank is left.  sdfr_search_select
    with keep = 1."""
    if loss.dim() != 2 or tuple(flags.shape) != tuple(loss.shape):
        raise ValueError("choose: loss and flags must both be [B][keep]")
    B, keep = int(loss.shape[0]), int(loss.shape[1])
    coff = torch.arange(B + 1, dtype=torch.int64, device=loss.device) * keep
    order, _ = select(loss.reshape(-1), flags.reshape(-1), coff, 1)
    first = order[:, 0].long()
    return torch.where(first >= 0, first - coff[:-1], first)
