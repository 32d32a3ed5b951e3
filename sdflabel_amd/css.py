"""The CSS network's output head on the device (csrc/css_head.hip): what networks/resnet_css.py:194-196 and :203-249 of the reference
compute from the decoder features, in one launch each.

css_head / css_latent are the inference path: their outputs are detached.  Training runs through css_head_loss / css_latent_loss
(csrc/css_train.hip): the losses of the reference's pipelines/train_css.py:71-80 as torch.autograd.Functions whose forward makes one fused
call that returns the loss AND the gradients for unit upstream gradient; backward only scales them.  Nothing [B][256][H][W] is ever
allocated.  sdflabel_amd.networks.resnet_css.ResNet.loss and sdflabel_amd.pipelines.train_css build the training step on them."""
import torch

from . import _lib
from ._lib import SdfrError, check, guard, lib, ptr, stream_ptr

N_FEAT, N_CLASS, N_LAT_FEAT = 64, 256, 256
# css_head_loss's workspace: the workgroups' partial dW / db / loss sums on a fixed grid (csrc/css_train.hip: CT_GX workgroups per colour head,
# CT_MGX for the mask head; include/sdfr.h SDFR_CSS_LOSS_WS_FIXED) plus one float32 log-sum-exp per pixel and colour head.  Nothing else is
# allocated besides the outputs.
_GX, _MGX = 80, 128
HEAD_LOSS_WORKSPACE_FIXED_BYTES = ((3 * _GX * 2 + _MGX) * 8
                                   + (3 * _GX * N_CLASS * N_FEAT + 3 * _GX * N_CLASS + _MGX * 2 * N_FEAT + _MGX * 2) * 4)
HEAD_LOSS_WORKSPACE_BYTES_PER_PIXEL = 12
LATENT_LOSS_WORKSPACE_BYTES_PER_CROP = 8 + (3 * 256 + 3) * 4


def head_loss_workspace_bytes(B, H, W):
    """bytes of device memory css_head_loss allocates besides the tensors it returns"""
    return HEAD_LOSS_WORKSPACE_FIXED_BYTES + HEAD_LOSS_WORKSPACE_BYTES_PER_PIXEL * int(B) * int(H) * int(W)


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


_HEADS = ('u', 'v', 'w', 'mask')


def _head_inputs(fn, x_u, x_v, x_w, x_mask, weights):
    """what css_head and head_loss_raw (`fn`: the caller's name in the messages) check alike: B, C, H, W, the device, the four features and
    the (weight, bias) pairs of u, v, w, mask"""
    x_u = _f32_cuda(x_u, "%s: x_u" % fn)
    if x_u.dim() != 4:
        raise SdfrError("%s: x_u must be [B][64][H][W] (got shape %s)" % (fn, tuple(x_u.shape)))
    B, C, H, W = (int(v) for v in x_u.shape)
    x_v = _f32_cuda(x_v, "%s: x_v" % fn, x_u.shape)
    x_w = _f32_cuda(x_w, "%s: x_w" % fn, x_u.shape)
    x_mask = _f32_cuda(x_mask, "%s: x_mask" % fn, x_u.shape)
    dev = x_u.device
    for t, n in ((x_v, "x_v"), (x_w, "x_w"), (x_mask, "x_mask")):
        if t.device != dev:
            raise SdfrError("%s: %s lives on %s, x_u on %s" % (fn, n, t.device, dev))
    if C != N_FEAT:
        raise SdfrError("%s: the head takes %d feature channels (got %d)" % (fn, N_FEAT, C))
    wb = [_linear(weights[h], "%s: weights['%s']" % (fn, h), 2 if h == 'mask' else N_CLASS, N_FEAT, dev) for h in _HEADS]
    return B, C, H, W, dev, (x_u, x_v, x_w, x_mask), wb


def _latent_inputs(fn, x4, w, b):
    """what css_latent and latent_loss_raw check alike: B, C, h, w, the feature map and out_lat's (weight, bias)"""
    x4 = _f32_cuda(x4, "%s: x4" % fn)
    if x4.dim() != 4:
        raise SdfrError("%s: x4 must be [B][256][h][w] (got shape %s)" % (fn, tuple(x4.shape)))
    B, C, h, wd = (int(v) for v in x4.shape)
    if C != N_LAT_FEAT:
        raise SdfrError("%s: out_lat takes %d feature channels (got %d)" % (fn, N_LAT_FEAT, C))
    return B, C, h, wd, x4, _linear((w, b), "%s: out_lat" % fn, 3, N_LAT_FEAT, x4.device)


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
    B, C, H, W, dev, (x_u, x_v, x_w, x_mask), ((wu, bu), (wv, bv), (ww, bw), (wm, bm)) = _head_inputs("css_head", x_u, x_v, x_w, x_mask, weights)
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
    B, C, h, wd, x4, (wl, bl) = _latent_inputs("css_latent", x4, w, b)
    out = torch.empty((B, 3), dtype=torch.float32, device=x4.device)
    with guard(x4):
        check(lib().sdfr_css_latent(ptr(x4), B, C, h, wd, ptr(wl), ptr(bl), ptr(out), stream_ptr()), "sdfr_css_latent")
    return out


def _target_u8(t, what, shape, device):
    """ground-truth classes as contiguous uint8 on the device: uint8 as given, the dataset's int64 converted on the device"""
    if not torch.is_tensor(t):
        raise SdfrError("%s must be a torch tensor (got %s)" % (what, type(t).__name__))
    if not t.is_cuda:
        raise SdfrError("%s: sdflabel_amd runs on the GPU only (got a %s tensor); there is no CPU fallback" % (what, t.device))
    if t.device != device:
        raise SdfrError("%s lives on %s, the features on %s" % (what, t.device, device))
    if t.dtype not in (torch.uint8, torch.int64):
        raise SdfrError("%s must be uint8 or int64 (got %s)" % (what, t.dtype))
    if tuple(t.shape) != tuple(shape):
        raise SdfrError("%s must have shape %s (got %s)" % (what, tuple(shape), tuple(t.shape)))
    if t.dtype == torch.int64:
        t = t.to(torch.uint8)
    elif not t.is_contiguous():
        raise SdfrError("%s must be contiguous; got strides %s for shape %s" % (what, tuple(t.stride()), tuple(t.shape)))
    return t.detach().contiguous()


def _new(shape, device, empty_input):
    """an output buffer; zeros when the input is empty, because the library then writes nothing"""
    return (torch.zeros if empty_input else torch.empty)(shape, dtype=torch.float32, device=device)


def head_loss_raw(x_u, x_v, x_w, x_mask, weights, uvw_gt, mask_gt):
    """The fused call behind css_head_loss, without autograd: returns {'loss': float32 [4] (u, v, w, mask), 'dx': {'u', 'v', 'w', 'mask'}
    [B][64][H][W], 'dw': {...} [256][64] ([2][64] for the mask), 'db': {...}}, the gradients of each head's own loss for unit upstream gradient.
    Allocates head_loss_workspace_bytes(B, H, W) besides what it returns."""
    B, C, H, W, dev, (x_u, x_v, x_w, x_mask), wb = _head_inputs("css_head_loss", x_u, x_v, x_w, x_mask, weights)
    wb = dict(zip(_HEADS, wb))
    uvw = _target_u8(uvw_gt, "css_head_loss: uvw_gt", (B, 3, H, W), dev)
    msk = _target_u8(mask_gt, "css_head_loss: mask_gt", (B, H, W), dev)
    f = lambda *shape: _new(shape, dev, B * H * W == 0)                                # noqa: E731
    out = {'loss': f(4), 'dx': {h: f(B, C, H, W) for h in wb}, 'dw': {h: f(*wb[h][0].shape) for h in wb}, 'db': {h: f(*wb[h][1].shape) for h in wb}}
    ws_bytes = head_loss_workspace_bytes(B, H, W)
    ws = torch.empty((ws_bytes + 7) // 8, dtype=torch.float64, device=dev)
    with guard(x_u):
        check(lib().sdfr_css_head_loss(ptr(x_u), ptr(x_v), ptr(x_w), ptr(x_mask), B, C, H, W, ptr(wb['u'][0]), ptr(wb['u'][1]), ptr(wb['v'][0]),
                                       ptr(wb['v'][1]), ptr(wb['w'][0]), ptr(wb['w'][1]), ptr(wb['mask'][0]), ptr(wb['mask'][1]), ptr(uvw),
                                       ptr(msk), ptr(out['loss']), ptr(out['dx']['u']), ptr(out['dx']['v']), ptr(out['dx']['w']),
                                       ptr(out['dx']['mask']), ptr(out['dw']['u']), ptr(out['db']['u']), ptr(out['dw']['v']), ptr(out['db']['v']),
                                       ptr(out['dw']['w']), ptr(out['db']['w']), ptr(out['dw']['mask']), ptr(out['db']['mask']), ptr(ws),
                                       ws_bytes, stream_ptr()), "sdfr_css_head_loss")
    return out


def latent_loss_raw(x4, w, b, latent_gt):
    """The fused call behind css_latent_loss: {'loss': float32 [1], 'dx': [B][256][h][w], 'dw': [3][256], 'db': [3]} for unit upstream gradient"""
    B, C, h, wd, x4, (wl, bl) = _latent_inputs("css_latent_loss", x4, w, b)
    gt = _f32_cuda(latent_gt, "css_latent_loss: latent_gt", (B, 3))
    if gt.device != x4.device:
        raise SdfrError("css_latent_loss: latent_gt lives on %s, x4 on %s" % (gt.device, x4.device))
    f = lambda *shape: _new(shape, x4.device, B * h * wd == 0)                         # noqa: E731
    out = {'loss': f(1), 'dx': f(B, C, h, wd), 'dw': f(3, N_LAT_FEAT), 'db': f(3)}
    ws_bytes = LATENT_LOSS_WORKSPACE_BYTES_PER_CROP * B
    ws = torch.empty(max((ws_bytes + 7) // 8, 1), dtype=torch.float64, device=x4.device)
    with guard(x4):
        check(lib().sdfr_css_latent_loss(ptr(x4), B, C, h, wd, ptr(wl), ptr(bl), ptr(gt), ptr(out['loss']), ptr(out['dx']), ptr(out['dw']),
                                         ptr(out['db']), ptr(ws), ws_bytes, stream_ptr()), "sdfr_css_latent_loss")
    return out


class _HeadLoss(torch.autograd.Function):
    """inputs: 4 features, then (weight, bias) of u, v, w, mask, then the two targets; outputs: the four losses"""

    @staticmethod
    def forward(ctx, x_u, x_v, x_w, x_mask, wu, bu, wv, bv, ww, bw, wm, bm, uvw_gt, mask_gt):
        r = head_loss_raw(x_u, x_v, x_w, x_mask, {'u': (wu, bu), 'v': (wv, bv), 'w': (ww, bw), 'mask': (wm, bm)}, uvw_gt, mask_gt)
        saved = []
        for h, wt in zip(_HEADS, (wu, wv, ww, wm)):
            saved += [r['dx'][h], r['dw'][h].view(wt.shape), r['db'][h]]
        ctx.save_for_backward(*saved)
        return tuple(r['loss'][i].clone() for i in range(4))

    @staticmethod
    def backward(ctx, *up):
        s = ctx.saved_tensors
        need = ctx.needs_input_grad
        sc = lambda g, i, wanted: g * up[i] if wanted else None                            # noqa: E731
        dx = [sc(s[3 * i], i, need[i]) for i in range(4)]
        dwb = []
        for i in range(4):
            dwb += [sc(s[3 * i + 1], i, need[4 + 2 * i]), sc(s[3 * i + 2], i, need[5 + 2 * i])]
        return tuple(dx) + tuple(dwb) + (None, None)


class _LatentLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x4, w, b, latent_gt):
        r = latent_loss_raw(x4, w, b, latent_gt)
        ctx.save_for_backward(r['dx'], r['dw'].view(w.shape), r['db'])
        return r['loss'][0].clone()

    @staticmethod
    def backward(ctx, up):
        need = ctx.needs_input_grad
        return tuple(g * up if n else None for g, n in zip(ctx.saved_tensors, need[:3])) + (None,)


@_lib.traced("css_head_loss")
def css_head_loss(x_u, x_v, x_w, x_mask, weights, uvw_gt, mask_gt):
    """The training losses of the output head (pipelines/train_css.py:71-76 of the reference), differentiable.  x_*: contiguous float32 GPU
    tensors [B][64][H][W]; weights as for css_head (the conv's own [256][64][1][1] parameters are fine); uvw_gt [B][3][H][W] and mask_gt
    [B][H][W] (nonzero: foreground) as uint8, or the dataset's int64, which is converted on the device.  Returns {'u', 'v', 'w', 'mask'}: four
    scalar tensors, CrossEntropyLoss(log_softmax(logits) * mask_gt, uvw_gt[:, h] * mask_gt) per colour head and 2 CrossEntropyLoss(mask
    logits, mask_gt).  Gradients reach the four features and the eight weight and bias tensors.  The same refusals as css_head."""
    flat = []
    for h in _HEADS:
        flat += list(weights[h])
    lu, lv, lw, lm = _HeadLoss.apply(x_u, x_v, x_w, x_mask, *flat, uvw_gt, mask_gt)
    return {'u': lu, 'v': lv, 'w': lw, 'mask': lm}


@_lib.traced("css_latent_loss")
def css_latent_loss(x4, w, b, latent_gt):
    """MSELoss(latent, latent_gt) of the reference (train_css.py:77) for x4 [B][256][h][w], out_lat's w, b and latent_gt float32 [B][3] on the
    GPU, differentiable towards x4, w and b.  The latent's length is a constant of the backward, as in the reference's
    project_vecs_onto_sphere (which detaches it)."""
    return _LatentLoss.apply(x4, w, b, latent_gt)
