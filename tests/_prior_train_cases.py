"""Decoders, rows and (decoder, n, p) cases of the prior-training tests (tests/test_prior_train_cpu.py calibrates on them with the float32
emulation, tests/test_gpu_prior_train.py runs the kernels on them): the smallest set at which each mechanism can go wrong.  Padded widths
128 / 256 / 512 (the 506-wide layer), the full 8x512 fixture, xyz_in_all, use_tanh, a latent of 8 (n_inputs 11); rows 1, 63, 64, 65, 200
(the 64-row tile) and, on the small decoder only -- the chunk rule does not depend on the width --, chunk - 1, chunk, chunk + 1 and
2 chunk + 76 (three partials, a ragged last one).  Built on the CPU.
"""
import functools

import numpy as np
import torch

from sdflabel_amd.deepsdf.networks.deep_sdf_decoder_scale import Decoder
from sdflabel_amd.deepsdf.workspace import setup_dsdf
from sdflabel_amd.fixtures import ASSET

from tests._decoder_ref import Net
from tests._prior_train_ref import CHUNK

SEED = 0x5DF0A11CE
P = 0.2


def _random(seed, **kw):
    torch.manual_seed(seed)
    d = Decoder(**kw)
    g = torch.Generator().manual_seed(2000 + seed)
    with torch.no_grad():
        for name, p in d.named_parameters():
            if name.startswith("lin"):
                p.add_(0.05 * torch.randn(p.shape, generator=g))
    return d.eval()


@functools.lru_cache(maxsize=None)
def decoders():
    out = {}
    common = dict(dropout=[0, 1, 2], dropout_prob=P, norm_layers=(), weight_norm=False)
    out["w128"] = _random(11, latent_size=3, dims=[128] * 3, latent_in=[2], **common)
    out["w256"] = _random(12, latent_size=3, dims=[256] * 3, latent_in=(), **common)
    out["w512"] = _random(13, latent_size=3, dims=[512] * 3, latent_in=[2], **common)
    out["asset"] = setup_dsdf(ASSET + ".pt", precision=torch.float32)[0].eval()             # 8x512, weight norm, latent_in = [4], dropout 0..7
    out["xyz"] = _random(14, latent_size=3, dims=[128] * 3, latent_in=[1], xyz_in_all=True, **common)
    out["tanh"] = _random(15, latent_size=3, dims=[128] * 3, latent_in=[2], use_tanh=True, **common)
    out["lat8"] = _random(16, latent_size=8, dims=[128] * 3, latent_in=[2], **common)
    return out


NAMES = ("w128", "w256", "w512", "asset", "xyz", "tanh", "lat8")
TILE_ROWS = (1, 63, 64, 65, 200)
CHUNK_ROWS = (CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 76)


def cases():
    """(name, n, p)"""
    out = []
    for n in TILE_ROWS + CHUNK_ROWS:
        for p in (0.0, P):
            out.append(("w128", n, p))
    for name in NAMES[1:]:
        for n, p in ((65, 0.0), (200, P)):
            out.append((name, n, p))
    return out


@functools.lru_cache(maxsize=None)
def net(name):
    return Net.from_decoder(decoders()[name])


def drop_layers(name):
    d = decoders()[name]
    m = 0
    for l in (d.dropout or ()):
        if l < d.num_layers - 2:
            m |= 1 << l
    return m


@functools.lru_cache(maxsize=None)
def rows(name, n):
    """(n, n_inputs) float32: unit latents (a few per batch, contiguous blocks) and xyz uniform in the cube; g_sdf (n,) float32 of mixed
    sign and size, some exactly zero (the clamped L1's gradient is +-1/n or 0)"""
    ni = net(name).n_inputs
    rng = np.random.default_rng(300 + NAMES.index(name) * 17 + n)
    lat = rng.standard_normal((4, ni - 3))
    lat /= np.linalg.norm(lat, axis=1, keepdims=True)
    x = np.concatenate([lat[(np.arange(n) * 4) // max(n, 1)], rng.uniform(-1, 1, (n, 3))], 1).astype(np.float32)
    g = (rng.choice([-1.0, 0.0, 1.0], n, p=[0.45, 0.1, 0.45]) * rng.uniform(0.5, 1.5, n) / n).astype(np.float32)
    if n == 1:
        g[:] = 1.0
    x.setflags(write=False)
    g.setflags(write=False)
    return x, g
