"""Decoders and rows of the decoder reference tests (tests/test_decoder_refs_cpu.py, tests/test_gpu_decoder_ref.py): the smallest set
that reaches every code path of csrc/mlp*.hip -- padded widths 128 / 256 / 512, K-side and generic re-injection (8 / 9 input columns),
xyz_in_all + use_tanh, LayerNorm at the three padded widths, a layer that is dead on every row.  Built on the CPU; nothing here needs a GPU.
"""
import copy
import functools

import numpy as np
import torch

from sdflabel_amd.deepsdf.networks.deep_sdf_decoder_scale import Decoder
from sdflabel_amd.deepsdf.workspace import setup_dsdf
from sdflabel_amd.fixtures import ASSET

from tests._decoder_ref import Net, evaluate

N_ROWS = 300
LAUNCH_SIZES = (1, 17, 64, 65, 129, 300)          # cross the 16-, 32-, 64- and 128-row tiles and the 128-row mask block
# the batched Jacobian layout: crop b selects cnt[b] of its rows_per_crop rows
JAC_B, JAC_ROWS, JAC_CAP, JAC_CNT = 3, 100, 48, (0, 1, 37)
SENTINEL = -777.25
SATURATED_Y = 10.0


def _random(seed, **kw):
    """torch's default init plus 0.05 randn, seeded"""
    torch.manual_seed(seed)
    d = Decoder(**kw)
    g = torch.Generator().manual_seed(1000 + seed)
    with torch.no_grad():
        for name, p in d.named_parameters():
            if name.startswith(("lin", "bn")):
                p.add_(0.05 * torch.randn(p.shape, generator=g))
    return d.eval()


def _build():
    out = {}
    out["asset"] = setup_dsdf(ASSET + ".pt", precision=torch.float32)[0].eval()            # 8x512, weight norm, latent_in = [4]
    w260 = dict(dims=[260] * 3, dropout=None, norm_layers=(), latent_in=[1, 2], weight_norm=False)
    out["w260"] = _random(1, latent_size=5, **w260)                                          # 8 input columns: the K-side limit
    out["w260_9"] = _random(2, latent_size=6, **w260)                                        # 9 columns: generic injection
    out["xyz_tanh"] = _random(3, latent_size=5, dims=[260] * 3, dropout=None, norm_layers=(), latent_in=[2], weight_norm=False,
                              xyz_in_all=True, use_tanh=True)
    for i, w in enumerate((200, 48, 128)):                                                   # padded 256, 128, 128
        out["w%d" % w] = _random(4 + i, latent_size=3, dims=[w] * 4, dropout=None, norm_layers=(), latent_in=[2], weight_norm=False)
    for i, w in enumerate((64, 200, 512)):
        out["ln%d" % w] = _random(7 + i, latent_size=3, dims=[w] * 3, dropout=None, norm_layers=[0, 1, 2], latent_in=[2], weight_norm=False)
    dead = copy.deepcopy(out["w260"])
    with torch.no_grad():
        dead.lin1.bias.fill_(-50.0)                                                          # the second layer is dead on every row
    out["dead"] = dead
    return out


@functools.lru_cache(maxsize=None)
def decoders():
    return _build()


NAMES = ("asset", "w260", "w260_9", "xyz_tanh", "w200", "w48", "w128", "ln64", "ln200", "ln512", "dead")
NAMES_512 = ("asset", "w260", "w260_9", "xyz_tanh", "dead")                                # padded 512, no LayerNorm: half and split paths


@functools.lru_cache(maxsize=None)
def net(name):
    return Net.from_decoder(decoders()[name])


@functools.lru_cache(maxsize=None)
def rows(name):
    """(300, n_inputs) float32: a third 0.6 randn; a third unit latent + uniform cube; the zero row and rows of magnitude 4.  The
    magnitude-4 rows do not saturate tanh on these decoders (largest |out| 0.998), so the last row is replaced by one of them scaled by the smallest power of two
    (at most 64: activations stay far inside half's range) that takes the reference's pre-tanh value beyond 10 -- float32 tanh then
    returns 1 and the output derivative is 0.  LayerNorm decoders cannot be driven there by their inputs: their last row stays as it is."""
    ni = net(name).n_inputs
    rng = np.random.default_rng(100 + NAMES.index(name))
    a = 0.6 * rng.standard_normal((100, ni))
    lat = rng.standard_normal((100, ni - 3))
    lat /= np.linalg.norm(lat, axis=1, keepdims=True)
    b = np.concatenate([lat, rng.uniform(-1, 1, (100, 3))], 1)
    c = rng.standard_normal((100, ni))
    c *= 4.0 / np.linalg.norm(c, axis=1, keepdims=True)
    c[0] = 0.0
    x = np.concatenate([a, b, c], 0).astype(np.float32)
    for k in range(1, 7):
        scaled = x[201:] * np.float32(2 ** k)
        y = np.abs(evaluate(net(name), scaled, want_masses=False).y)
        if y.max() > SATURATED_Y:
            x[-1] = scaled[int(y.argmax())]
            break
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def jac_layout():
    """idx int32 [B][cap] (crop 1: one row; crop 2: 37 rows, ascending then shuffled -- the kernels take any order), unused slots hold a
    valid row so that a kernel that read them would not fault"""
    rng = np.random.default_rng(7)
    idx = np.zeros((JAC_B, JAC_CAP), np.int32)
    idx[1, 0] = 99
    sel = np.sort(np.append(rng.choice(JAC_ROWS - 1, JAC_CNT[2] - 1, replace=False), JAC_ROWS - 1)).astype(np.int32)    # with the saturated row
    idx[2, :JAC_CNT[2]] = rng.permutation(sel)
    idx.setflags(write=False)
    return idx
