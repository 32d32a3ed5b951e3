"""Augmentation of the CSS network's training crops on the device: the transforms of the reference's datasets/crops.py (ColorJitter,
RandomRotation(10, expand=True), Resize((128, 128)), RandomResizedCrop(128, scale=(0.5, 1)), ToTensor, Normalize; bilinear for the RGB image,
nearest for the UVW label image) for a ragged batch of source crops in four launches (csrc/augment.hip).

  draw_params(sizes, generator)             the random parameters of a batch, drawn on the host
  augment_many(rgb_list, uvw_list, params)  -> rgb float32 [B][3][128][128], uvw uint8 [B][3][128][128], mask uint8 [B][128][128]
  pack_batch, run_batch                     its host half (checks, tables, uploads) and its device half (four launches)
  rotation_matrix(w, h, angle)              the host arithmetic of Image.rotate(angle, expand=True)

Given the same parameters every byte is Pillow 12's (tests/test_augment_cpu.py pins a numpy restatement to Pillow itself, including
convert('HSV') over all 2^24 colours; tests/test_gpu_augment.py pins the kernels to that restatement).  Two things are NOT reproduced or
tested: the stream of random numbers is our own and not torchvision's (a torch.Generator on the host; the reference seeds Python's `random`),
and torchvision is not installed where this project is built, so the mapping "torchvision call -> Pillow call" is written from its PIL
backend (functional_pil.py) and not tested against it."""
import math

import numpy as np
import torch

from . import _lib
from .pose import _upload

P, ck = _lib.ptr, _lib.check
OUT = 128
N_PARAMS = 13                        # a row of `params`: brightness, contrast, saturation, hue, order[4], angle, box i, j, h, w
_ROW = 20                            # SDFR_AUG_PARAMS of include/sdfr.h
_ORDER, _MATRIX, _BOX = 4, 8, 14     # SDFR_AUG_ORDER, SDFR_AUG_MATRIX, SDFR_AUG_BOX_I


def rotation_matrix(w, h, angle):
    """Image.rotate(angle, resample, expand=True) of a w x h image, as Pillow's Python computes it in float64: (matrix, nw, nh) with the six
    entries of the re-centred affine matrix (output pixel -> source position) and the expanded size; (None, w, h) when angle % 360 == 0,
    where Pillow returns a copy."""
    angle = angle % 360.0
    if angle == 0:
        return None, int(w), int(h)
    if angle in (90, 180, 270):
        raise ValueError("augment: a rotation by %g degrees is a transpose in Pillow, which the kernels do not implement" % angle)
    a = -math.radians(angle)
    m = [round(math.cos(a), 15), round(math.sin(a), 15), 0.0, round(-math.sin(a), 15), round(math.cos(a), 15), 0.0]

    def tf(x, y):
        return m[0] * x + m[1] * y + m[2], m[3] * x + m[4] * y + m[5]
    cx, cy = w / 2, h / 2
    m[2], m[5] = tf(-cx, -cy)
    m[2] += cx
    m[5] += cy
    xs, ys = zip(*(tf(x, y) for x, y in ((0, 0), (w, 0), (w, h), (0, h))))
    nw = math.ceil(max(xs)) - math.floor(min(xs))
    nh = math.ceil(max(ys)) - math.floor(min(ys))
    m[2], m[5] = tf(-(nw - w) / 2.0, -(nh - h) / 2.0)
    return m, int(nw), int(nh)


def _uniform(gen, lo, hi):
    return lo + (hi - lo) * float(torch.rand((), generator=gen, dtype=torch.float64))


def draw_params(sizes, generator=None):
    """The random parameters of the reference's transforms for len(sizes) samples: float64 [B][13] rows of brightness, contrast, saturation
    ~ U(0.6, 1.4), hue ~ U(-0.2, 0.2), a uniform permutation of the four jitter operations (0 brightness, 1 contrast, 2 saturation, 3 hue, in
    the order applied), angle ~ U(-10, 10) degrees, and RandomResizedCrop's box (i, j, h, w) inside the 128 x 128 intermediate: up to ten
    tries of area ~ U(0.5, 1) * 128^2 with a log-uniform aspect ratio in (3/4, 4/3), then the centre fallback (the whole image for a
    square).  One geometric draw per sample serves its RGB and its UVW image, as the reference arranges through its seed.

    sizes: one (w, h) per sample; the draws do not depend on them (the crop box lives in the fixed-size intermediate), they fix B.
    The stream of random numbers is our own, a torch.Generator on the host, not torchvision's."""
    B = len(sizes)
    out = np.zeros((B, N_PARAMS), np.float64)
    area = float(OUT * OUT)
    log_lo, log_hi = math.log(3.0 / 4.0), math.log(4.0 / 3.0)
    for b in range(B):
        out[b, 0:3] = [_uniform(generator, 0.6, 1.4) for _ in range(3)]
        out[b, 3] = _uniform(generator, -0.2, 0.2)
        out[b, 4:8] = torch.randperm(4, generator=generator).numpy()
        out[b, 8] = _uniform(generator, -10.0, 10.0)
        box = None
        for _ in range(10):
            target = area * _uniform(generator, 0.5, 1.0)
            ratio = math.exp(_uniform(generator, log_lo, log_hi))
            w = int(round(math.sqrt(target * ratio)))
            h = int(round(math.sqrt(target / ratio)))
            if 0 < w <= OUT and 0 < h <= OUT:
                i = int(torch.randint(0, OUT - h + 1, (), generator=generator))
                j = int(torch.randint(0, OUT - w + 1, (), generator=generator))
                box = (i, j, h, w)
                break
        out[b, 9:13] = box if box is not None else (0, 0, OUT, OUT)      # centre fallback: in-ratio of a square is 1, inside (3/4, 4/3)
    return out


def _host_u8(img, what, b):
    a = img.detach().cpu().numpy() if torch.is_tensor(img) else np.asarray(img)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError("augment_many: %s %d must be a uint8 [h][w][3] image, got %s %s" % (what, b, a.dtype, a.shape))
    return np.ascontiguousarray(a)


def pack_batch(rgb_list, uvw_list, params, device):
    """The host half of augment_many: checks, Image.rotate's matrices, and the two uploads (images; parameter and size tables).  Returns the
    device-resident batch that run_batch takes, None for an empty batch."""
    B = len(rgb_list)
    prm = np.asarray(params.detach().cpu().numpy() if torch.is_tensor(params) else params, dtype=np.float64).reshape(-1, N_PARAMS)
    if len(uvw_list) != B or prm.shape[0] != B:
        raise ValueError("augment_many: one UVW image and one parameter row per RGB image")
    if B == 0:
        return None
    meta = np.zeros((B, 8), np.int32)
    rows = np.zeros((B, _ROW), np.float64)
    srcs, labs = [], []
    first = extent = 0
    for b in range(B):
        r, u = _host_u8(rgb_list[b], "RGB image", b), _host_u8(uvw_list[b], "UVW image", b)
        if r.shape != u.shape:
            raise ValueError("augment_many: sample %d has an RGB image of %s and a UVW image of %s" % (b, r.shape, u.shape))
        h, w = r.shape[:2]
        order = prm[b, 4:8]
        if sorted(order.tolist()) != [0.0, 1.0, 2.0, 3.0]:
            raise ValueError("augment_many: sample %d: the jitter order %s is not a permutation of 0 ... 3" % (b, order.tolist()))
        if not -0.5 <= prm[b, 3] <= 0.5 or (prm[b, 0:3] < 0).any():
            raise ValueError("augment_many: sample %d: hue factor outside [-0.5, 0.5] or a negative jitter factor" % b)
        i, j, bh, bw = prm[b, 9:13]
        if not (np.array_equal(prm[b, 9:13], np.trunc(prm[b, 9:13])) and 0 <= i and 0 <= j and bh >= 1 and bw >= 1
                and i + bh <= OUT and j + bw <= OUT):
            raise ValueError("augment_many: sample %d: crop box (i, j, h, w) = %s is not inside %d x %d" % (b, prm[b, 9:13].tolist(), OUT, OUT))
        m, nw, nh = rotation_matrix(w, h, float(prm[b, 8]))
        meta[b] = (h, w, first, nw, nh, 1 if m is None else 0, 0, 0)
        rows[b, 0:8] = prm[b, 0:8]
        rows[b, _MATRIX:_MATRIX + 6] = m if m is not None else (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)
        rows[b, _BOX:_BOX + 4] = prm[b, 9:13]
        srcs.append(r.reshape(-1))
        labs.append(u.reshape(-1))
        first += h * w
        extent = max(extent, nw, nh)
    if 3 * first >= 2 ** 31:
        raise ValueError("augment_many: the batch holds %d source pixels, more than one call takes" % first)
    # one upload each: [RGB sources | UVW sources] as bytes, [params | meta] as float64 words
    packed = _upload(torch.from_numpy(np.concatenate(srcs + labs)), device)
    table = _upload(torch.from_numpy(np.concatenate((rows.reshape(-1), meta.reshape(-1).view(np.float64)))), device)
    return {"B": B, "pixels": first, "meta": meta, "ksize": 2 * int(math.ceil(max(extent / float(OUT), 1.0))) + 1,
            "rgb_src": packed[:3 * first], "uvw_src": packed[3 * first:], "rows_d": table[:B * _ROW], "meta_d": table[B * _ROW:]}


def run_batch(batch, return_stages=False):
    """The device half of augment_many: the workspaces, the outputs and sdfr_augment's four launches on a batch from pack_batch."""
    B, dev, ksize = batch["B"], batch["rgb_src"].device, batch["ksize"]
    rgb = torch.empty((B, 3, OUT, OUT), dtype=torch.float32, device=dev)
    uvw = torch.empty((B, 3, OUT, OUT), dtype=torch.uint8, device=dev)
    mask = torch.empty((B, OUT, OUT), dtype=torch.uint8, device=dev)
    rgb_u8 = torch.empty((B, OUT, OUT, 3), dtype=torch.uint8, device=dev) if return_stages else None
    tab = torch.empty((B, 4, OUT, 3 + ksize), dtype=torch.int32, device=dev)
    jit = torch.empty((3 * batch["pixels"],), dtype=torch.uint8, device=dev)
    mid = torch.empty((2, B, OUT, OUT, 3), dtype=torch.uint8, device=dev)
    with _lib.guard(dev):
        ck(_lib.lib().sdfr_augment(P(batch["rgb_src"]), P(batch["uvw_src"]), P(batch["meta_d"]), P(batch["rows_d"]), B, ksize, P(tab), P(jit),
                                   P(mid[0]), P(mid[1]), P(rgb), P(uvw), P(mask), P(rgb_u8), _lib.stream_ptr()), "sdfr_augment")
    if not return_stages:
        return rgb, uvw, mask
    return rgb, uvw, mask, {"rgb_u8": rgb_u8, "jitter": [jit[3 * int(m[2]):3 * int(m[2] + m[0] * m[1])].view(int(m[0]), int(m[1]), 3)
                                                         for m in batch["meta"]]}


@_lib.traced("augment_many")
def augment_many(rgb_list, uvw_list, params, device=None, return_stages=False):
    """The reference's training augmentation of B samples on the device, byte for byte what Pillow computes for the same parameters.

    rgb_list, uvw_list: per sample the source RGB image and its UVW label image, uint8 [h][w][3] (numpy or CPU tensors), the same size for
    both; sizes differ between samples.  params: [B][13] rows as draw_params returns them.
    Returns (rgb float32 [B][3][128][128] normalised with the ImageNet constants, uvw uint8 [B][3][128][128] labels,
    mask uint8 [B][128][128] = (u + v + w > 0)) on the device; with return_stages additionally a dict with 'rgb_u8' [B][128][128][3], the
    final image before ToTensor, and 'jitter', the list of the B images after the colour jitter.
    One upload for the images and one for the tables, four launches whatever B, no host synchronisation.  Workspaces: the jittered sources
    (the size of the sources), two uint8 [B][128][128][3] intermediates and the resample tables; no rotated image is stored."""
    if not torch.cuda.is_available():
        raise _lib.SdfrError("augment_many runs on the GPU only; there is no CPU fallback")
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    if dev.type != "cuda":
        raise _lib.SdfrError("augment_many runs on the GPU only (got device %s); there is no CPU fallback" % dev)
    batch = pack_batch(rgb_list, uvw_list, params, dev)
    if batch is None:
        out = (torch.empty((0, 3, OUT, OUT), dtype=torch.float32, device=dev), torch.empty((0, 3, OUT, OUT), dtype=torch.uint8, device=dev),
               torch.empty((0, OUT, OUT), dtype=torch.uint8, device=dev))
        return out + ({"rgb_u8": torch.empty((0, OUT, OUT, 3), dtype=torch.uint8, device=dev), "jitter": []},) if return_stages else out
    return run_batch(batch, return_stages)
