"""Training the DeepSDF decoder on the device: the decoder's forward with stored activations and its gradients with respect to the input
rows and the weights (csrc/mlp_train.hip through sdfr_decoder_train_forward / _backward), as a torch.autograd.Function.

Only the three GEMM passes are kernels.  The weight-norm fold W = v g / ||v||, cat(latent[shape], xyz), the loss and Adam stay torch ops
under autograd: they are small, and autograd differentiates them (pipelines/train_prior.py).  DESIGN.md 7j.

Dropout is the library's OWN random stream -- an integer hash of (seed, layer, row, feature), include/sdfr.h -- not torch's: a run with
drop_p > 0 is repeatable from its seeds but does not reproduce nn.Dropout's masks.
"""
import ctypes

import torch

from .. import _lib

CHUNK = 1024          # rows per partial of dW / db (csrc/train_cells.h TRAIN_CHUNK)
HEADER_WORDS = 16     # words in front of the workspace (TRAIN_HEADER_FLOATS)


class TrainDesc:
    """The decoder description the training entry points take (as sdfr_decoder_create: in_dim / out_dim of every linear, the injection
    table, n_inputs, use_tanh), `drop_layers` the bit mask of the layers with dropout, and the workspace cached per row count."""

    def __init__(self, in_dim, out_dim, inj, n_inputs, use_tanh=False, drop_layers=0):
        self.in_dim = [int(v) for v in in_dim]
        self.out_dim = [int(v) for v in out_dim]
        self.inj = [(int(a), int(b)) for a, b in inj]
        self.n_lin = len(self.in_dim)
        self.n_inputs = int(n_inputs)
        self.use_tanh = bool(use_tanh)
        self.drop_layers = int(drop_layers)
        n = self.n_lin
        self._c = ((ctypes.c_int * n)(*self.in_dim), (ctypes.c_int * n)(*self.out_dim), (ctypes.c_int * n)(*[i[0] for i in self.inj]),
                   (ctypes.c_int * n)(*[i[1] for i in self.inj]))
        self._ws = {}

    @classmethod
    def from_decoder(cls, dec):
        """of an sdflabel_amd Decoder (its `dropout` list becomes drop_layers).  LayerNorm decoders are refused: no training kernels."""
        if any(getattr(dec, "bn" + str(l), None) is not None for l in range(dec.num_layers - 1)):
            raise _lib.SdfrError("decoder training: LayerNorm decoders are not supported")
        if dec.latent_dropout:
            raise _lib.SdfrError("decoder training: latent_dropout is not supported")
        lins = [getattr(dec, "lin" + str(l)) for l in range(dec.num_layers - 1)]
        drop = 0
        for l in (dec.dropout or ()):
            if 0 <= int(l) < dec.num_layers - 2:
                drop |= 1 << int(l)
        return cls([m.in_features for m in lins], [m.out_features for m in lins], dec._inject_table(), dec.latent_size + 3, dec.use_tanh, drop)

    def macs(self):
        return sum(i * o for i, o in zip(self.in_dim, self.out_dim))

    def args(self):
        return (self.n_lin,) + self._c + (self.n_inputs,)

    def bytes(self, n):
        b = int(_lib.lib().sdfr_decoder_train_bytes(*self.args(), int(n)))
        if b < 0:
            raise _lib.SdfrError("sdfr_decoder_train_bytes: %s" % _lib.lib().sdfr_last_error().decode())
        return b

    def act_offset(self, l, n):
        """first word of act[l] ([n][in_dim[l + 1]]) in the workspace, as include/sdfr.h states it"""
        return HEADER_WORDS + int(n) * sum(self.in_dim[:l + 1])

    def workspace(self, n, device):
        key = (int(n), str(device))
        ws = self._ws.get(key)
        if ws is None:
            if len(self._ws) >= 4:
                self._ws.clear()
            ws = self._ws[key] = torch.empty((self.bytes(n) // 4,), dtype=torch.float32, device=device)
        return ws


def _ptrs(tensors):
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def train_forward(desc, weights, biases, inputs, drop_p, seed, ws, sdf):
    n = int(inputs.shape[0])
    with _lib.guard(inputs):
        _lib.check(_lib.lib().sdfr_decoder_train_forward(*desc.args(), int(desc.use_tanh), _ptrs(weights), _ptrs(biases), _lib.ptr(inputs), n,
                                                         float(drop_p), desc.drop_layers, int(seed), _lib.ptr(sdf), _lib.ptr(ws),
                                                         ws.numel() * 4, _lib.stream_ptr()), "sdfr_decoder_train_forward")


def train_backward(desc, weights, g_sdf, ws, dW, db, g_inputs):
    n = int(g_sdf.shape[0])
    with _lib.guard(g_sdf):
        _lib.check(_lib.lib().sdfr_decoder_train_backward(*desc.args(), int(desc.use_tanh), _ptrs(weights), _lib.ptr(g_sdf), n, _lib.ptr(ws),
                                                          ws.numel() * 4, _ptrs(dW), _ptrs(db), _lib.ptr(g_inputs), _lib.stream_ptr()),
                   "sdfr_decoder_train_backward")


class _DecoderTrainFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, inputs, desc, drop_p, seed, *wb):
        nl = desc.n_lin
        weights = [w.detach().contiguous() for w in wb[:nl]]
        biases = [b.detach().contiguous() for b in wb[nl:]]
        x = inputs.detach().contiguous()
        n = int(x.shape[0])
        sdf = torch.empty((n,), dtype=torch.float32, device=x.device)
        ws = desc.workspace(n, x.device)
        if n > 0:
            train_forward(desc, weights, biases, x, drop_p, seed, ws, sdf)
        ctx.desc, ctx.ws, ctx.weights, ctx.n = desc, ws, weights, n
        ctx.ws_version = ws._version
        return sdf.view(n, 1)

    @staticmethod
    def backward(ctx, g):
        desc, n = ctx.desc, ctx.n
        dev = g.device
        dW = [torch.zeros_like(w) if n == 0 else torch.empty_like(w) for w in ctx.weights]
        db = [torch.zeros((o,), dtype=torch.float32, device=dev) if n == 0 else torch.empty((o,), dtype=torch.float32, device=dev)
              for o in desc.out_dim]
        g_in = torch.empty((n, desc.n_inputs), dtype=torch.float32, device=dev)
        if n > 0:
            train_backward(desc, ctx.weights, g.contiguous().float().view(-1), ctx.ws, dW, db, g_in)
        return (g_in, None, None, None) + tuple(dW) + tuple(db)


def decoder_train(inputs, weights, biases, desc, drop_p=0.0, seed=0):
    """sdf [n][1] of the decoder `desc` with the EFFECTIVE float32 weights [out][in] and biases (lists of device tensors, one per linear) on
    the rows inputs [n][n_inputs], differentiable with respect to inputs, weights and biases.  The forward keeps its activations in a
    workspace cached per n in `desc`: ONE forward may be pending per (desc, n) -- call backward before the next forward of the same size.
    drop_p: dropout probability of the layers in desc.drop_layers; seed: the step's seed of the hash (our own stream, not torch's)."""
    _lib.require_gpu_float(inputs)
    if inputs.dim() != 2 or inputs.shape[1] != desc.n_inputs:
        raise _lib.SdfrError("decoder_train: inputs must be (n, %d)" % desc.n_inputs)
    if len(weights) != desc.n_lin or len(biases) != desc.n_lin:
        raise _lib.SdfrError("decoder_train: %d linear layers described, %d weights and %d biases given" % (desc.n_lin, len(weights), len(biases)))
    for l, (w, b) in enumerate(zip(weights, biases)):
        if tuple(w.shape) != (desc.out_dim[l], desc.in_dim[l]) or tuple(b.shape) != (desc.out_dim[l],) or w.dtype != torch.float32 or \
                b.dtype != torch.float32 or w.device != inputs.device or b.device != inputs.device:
            raise _lib.SdfrError("decoder_train: layer %d needs float32 weights (%d, %d) and biases on %s" %
                                 (l, desc.out_dim[l], desc.in_dim[l], inputs.device))
    return _DecoderTrainFn.apply(inputs.float(), desc, float(drop_p), int(seed), *weights, *biases)


def segmented_sum(g, n_shapes):
    """[S][L] from [S * k][L]: the sum over each shape's k contiguous rows, in a fixed order (a reshape and one sum; no index_add, whose
    backward-style scatter uses atomics)."""
    return g.view(n_shapes, -1, g.shape[1]).sum(1)


class _ExpandLatents(torch.autograd.Function):
    """z [S][L] -> [S * k][L], every latent repeated for its shape's k contiguous samples; the backward is the segmented sum."""

    @staticmethod
    def forward(ctx, z, k):
        ctx.S = z.shape[0]
        return z.repeat_interleave(k, 0)

    @staticmethod
    def backward(ctx, g):
        return segmented_sum(g.contiguous(), ctx.S), None


def expand_latents(z, k):
    return _ExpandLatents.apply(z, int(k))
