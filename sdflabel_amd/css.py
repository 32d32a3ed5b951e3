"""The CSS network's output head on the device (csrc/css_head.hip): what networks/resnet_css.py:194-196 and :203-249 of the reference
compute from the decoder features, in one launch each.

INFERENCE ONLY: the outputs are detached and no gradient flows to the features or the weights.  Training the network
(pipelines/train_css.py of the reference) is out of scope; train with the reference's module and load its state_dict into
sdflabel_amd.networks.resnet_css, which keeps the reference's parameter names."""
import torch

from . import _lib
from ._lib import SdfrError, check, guard, lib, ptr, stream_ptr

N_FEAT, N_CLASS, N_LAT_FEAT = 64, 256, 256


def _f32_cuda(t, what, shape=None):
    if not torch.is_tensor(t):
        raise SdfrError("%s must be a torch tensor (got %s)" % (what, type(t).__name__))
    if not t.is_cuda:
        raise SdfrError("%s: sdflabel_amd runs on the GPU only (got a %s tensor); there is no CPU fallback" % (what, t.device))
    if t.dtype != torch.float32:
        raise SdfrError("%s must be float32 (got %s)" % (what, t.dtype))
    if not t.is_contiguous():
        raise SdfrError("%s must be contiguous (NCHW); got strides %s for shape %s" % (what, tuple(t.stride()), tuple(t.shape)))
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise SdfrError("%s must have shape %s (got %s)" % (what, tuple(shape), tuple(t.shape)))
    return t.detach()


def _linear(wb, what, n_out, n_in, device):
    """(weight, bias) of a 1x1 convolution as contiguous float32 [n_out][n_in] / [n_out] on `device` (a conv weight [n_out][n_in][1][1] is viewed)"""
    w, b = wb
    w, b = w.detach(), b.detach()
    if w.dim() == 4 and tuple(w.shape[2:]) == (1, 1):
        w = w.reshape(w.shape[0], w.shape[1])
    if tuple(w.shape) != (n_out, n_in) or tuple(b.shape) != (n_out,):
        raise SdfrError("%s: weight %s / bias %s, expected (%d, %d) / (%d,)" % (what, tuple(w.shape), tuple(b.shape), n_out, n_in, n_out))
    if w.dtype != torch.float32 or b.dtype != torch.float32:
        raise SdfrError("%s: weight and bias must be float32 (got %s, %s)" % (what, w.dtype, b.dtype))
    return w.to(device).contiguous(), b.to(device).contiguous()


@_lib.traced("css_head")
def css_head(x_u, x_v, x_w, x_mask, weights, logprobs=False):
    """The fused output head.  x_u, x_v, x_w, x_mask: contiguous float32 GPU tensors [B][64][H][W] (the outputs of up4_u / up4_v / up4_w /
    up4_mask).  weights: {'u': (W, b), 'v': (W, b), 'w': (W, b), 'mask': (W, b)} with W [256][64] (or the conv's [256][64][1][1]), b [256], and
    [2][64], [2] for the mask.  Returns a dict of new, DETACHED tensors (inference only, see the module docstring):
      'uvw_sm' [B][3][H][W]         sum_k k softmax_k(100 logit)
      'uvw_sm_masked' [B][3][H][W]  uvw_sm where mask[1] > mask[0], else 0
      'mask' [B][2][H][W]           the raw mask logits
      'mask_sm' [B][1][H][W]        softmax(100 mask)[1]
      'u', 'v', 'w' [B][256][H][W]  log_softmax(logit), only with logprobs=True
    A crop's result does not depend on the batch it is computed in.  Anything but float32, 64 channels and contiguous NCHW is refused."""
    x_u = _f32_cuda(x_u, "css_head: x_u")
    if x_u.dim() != 4:
        raise SdfrError("css_head: x_u must be [B][64][H][W] (got shape %s)" % (tuple(x_u.shape),))
    B, C, H, W = (int(v) for v in x_u.shape)
    x_v = _f32_cuda(x_v, "css_head: x_v", x_u.shape)
    x_w = _f32_cuda(x_w, "css_head: x_w", x_u.shape)
    x_mask = _f32_cuda(x_mask, "css_head: x_mask", x_u.shape)
    dev = x_u.device
    for t, n in ((x_v, "x_v"), (x_w, "x_w"), (x_mask, "x_mask")):
        if t.device != dev:
            raise SdfrError("css_head: %s lives on %s, x_u on %s" % (n, t.device, dev))
    if C != N_FEAT:
        raise SdfrError("css_head: the head takes %d feature channels (got %d)" % (N_FEAT, C))
    wu, bu = _linear(weights['u'], "css_head: weights['u']", N_CLASS, N_FEAT, dev)
    wv, bv = _linear(weights['v'], "css_head: weights['v']", N_CLASS, N_FEAT, dev)
    ww, bw = _linear(weights['w'], "css_head: weights['w']", N_CLASS, N_FEAT, dev)
    wm, bm = _linear(weights['mask'], "css_head: weights['mask']", 2, N_FEAT, dev)
    new = lambda c: torch.empty((B, c, H, W), dtype=torch.float32, device=dev)       # noqa: E731
    out = {'uvw_sm': new(3), 'uvw_sm_masked': new(3), 'mask': new(2), 'mask_sm': new(1)}
    if logprobs:
        out.update(u=new(N_CLASS), v=new(N_CLASS), w=new(N_CLASS))
    with guard(x_u):
        check(lib().sdfr_css_head(ptr(x_u), ptr(x_v), ptr(x_w), ptr(x_mask), B, C, H, W, ptr(wu), ptr(bu), ptr(wv), ptr(bv), ptr(ww), ptr(bw),
                                  ptr(wm), ptr(bm), ptr(out['uvw_sm']), ptr(out['uvw_sm_masked']), ptr(out['mask']), ptr(out['mask_sm']),
                                  ptr(out.get('u')), ptr(out.get('v')), ptr(out.get('w')), stream_ptr()), "sdfr_css_head")
    return out


@_lib.traced("css_latent")
def css_latent(x4, w, b):
    """out_lat of the reference on x4 [B][256][h][w] (contiguous float32, GPU): the 1x1 convolution w [3][256] (or [3][256][1][1]), b [3], the
    mean over the pixels and the projection onto the unit sphere, v * (1 / (|v| + 1e-8)).  Returns a new, detached [B][3] tensor."""
    x4 = _f32_cuda(x4, "css_latent: x4")
    if x4.dim() != 4:
        raise SdfrError("css_latent: x4 must be [B][256][h][w] (got shape %s)" % (tuple(x4.shape),))
    B, C, h, wd = (int(v) for v in x4.shape)
    if C != N_LAT_FEAT:
        raise SdfrError("css_latent: out_lat takes %d feature channels (got %d)" % (N_LAT_FEAT, C))
    wl, bl = _linear((w, b), "css_latent: out_lat", 3, N_LAT_FEAT, x4.device)
    out = torch.empty((B, 3), dtype=torch.float32, device=x4.device)
    with guard(x4):
        check(lib().sdfr_css_latent(ptr(x4), B, C, h, wd, ptr(wl), ptr(bl), ptr(out), stream_ptr()), "sdfr_css_latent")
    return out
