"""GPU tests of the exact-f32 grid forward's per-tile K compaction (mlp_kernel.h, KC): features that are zero at every
point of a 64-row tile are left out of the next layer's K chain.  Every sdf value, every saved ReLU mask word and one full BatchRenderer
step must be bit for bit what the full chain (SDFR_FWD_COMPACT=0) gives."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import sdflabel_amd
from sdflabel_amd import _lib
from sdflabel_amd.fixtures import ASSET, ASSET_ELLIPSOID, K_for

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _decoder(asset=ASSET):
    d, _ = sdflabel_amd.setup_dsdf(asset + ".pt", precision=torch.float32)
    return d.to(DEV)


@pytest.fixture(scope="module")
def dec():
    return _decoder()


def grid_inputs(latents, density=40):
    """[B * G][L + 3] rows: the crop's normalised latent and the grid point, as the batched path builds them"""
    pts = sdflabel_amd.Grid3D(density, DEV).points.detach()
    lat = F.normalize(torch.as_tensor(np.asarray(latents, np.float32), device=DEV), p=2, dim=1)
    rows = [torch.cat([l.expand(pts.shape[0], -1), pts], 1) for l in lat]
    return torch.cat(rows, 0).contiguous()


def forward(dec, inputs, n, compact, monkeypatch, masks=True):
    L = _lib.lib()
    h = dec.handle(torch.device(DEV)).h
    sdf = torch.full((n,), float("nan"), device=DEV)
    mw = torch.zeros(int(L.sdfr_decoder_mask_words(h, n)), dtype=torch.int32, device=DEV) if masks else None
    monkeypatch.setenv("SDFR_FWD_COMPACT", "1" if compact else "0")
    _lib.check(L.sdfr_mlp_forward(h, _lib.ptr(inputs), n, _lib.ptr(sdf), _lib.ptr(mw) if masks else None, _lib.stream_ptr()),
               "sdfr_mlp_forward")
    torch.cuda.synchronize()
    return sdf, mw


def assert_same_bits(dec, inputs, n, monkeypatch):
    for masks in (True, False):                  # MODE 1 (masks saved) and the same launch without a mask buffer (MODE 0 use)
        s0, m0 = forward(dec, inputs, n, False, monkeypatch, masks)
        s1, m1 = forward(dec, inputs, n, True, monkeypatch, masks)
        assert torch.equal(s0.view(torch.int32), s1.view(torch.int32))
        if masks:
            assert torch.equal(m0, m1)
    return s1


@pytest.mark.parametrize("lat", [[0.3, -0.5, 0.8], [1.0, 0.2, -0.4], [-0.7, -0.7, 0.1], [0.0, 0.0, 1.0]])
def test_bench_fixture_grid_bitwise(dec, lat, monkeypatch):
    inp = grid_inputs([lat])
    s = assert_same_bits(dec, inp, inp.shape[0], monkeypatch)
    assert torch.isfinite(s).all()


def test_ellipsoid_fixture_grid_bitwise(monkeypatch):
    d = _decoder(ASSET_ELLIPSOID)
    for lat in ([0.3, -0.5, 0.8], [0.9, 0.1, 0.3]):
        inp = grid_inputs([lat])
        assert_same_bits(d, inp, inp.shape[0], monkeypatch)


@pytest.mark.parametrize("n", [1, 31, 32, 33, 63, 65, 1000, 64000 - 17])
def test_ragged_row_counts_bitwise(dec, n, monkeypatch):
    """partial tiles: one row, the edges of a point tile (32 rows) and of a tile (64), a launch that ends 17 rows short"""
    inp = grid_inputs([[0.3, -0.5, 0.8]])
    s = assert_same_bits(dec, inp, n, monkeypatch)
    assert torch.isfinite(s).all()


def test_batch_of_64_crops_bitwise(dec, monkeypatch):
    rng = np.random.default_rng(7)
    inp = grid_inputs(rng.standard_normal((64, 3)), density=20)
    assert_same_bits(dec, inp, inp.shape[0], monkeypatch)


def test_random_rows_bitwise(dec, monkeypatch):
    """rows with no spatial coherence: few features are dead across a tile (long K lists)"""
    g = torch.Generator(device=DEV).manual_seed(3)
    inp = torch.rand(64 * 50 + 5, 6, device=DEV, generator=g) * 2 - 1
    assert_same_bits(dec, inp, inp.shape[0], monkeypatch)


def _shifted(layer, shift):
    d = _decoder()
    with torch.no_grad():
        getattr(d, "lin%d" % layer).bias.add_(shift)
    return d


def test_layer_with_every_feature_zero(monkeypatch):
    """layer 3 (in front of latent_in) all off: layer 4's K list holds only the re-injected latent / xyz columns"""
    d = _decoder()
    inp = grid_inputs([[0.3, -0.5, 0.8]])
    ref, _ = forward(d, inp, inp.shape[0], True, monkeypatch)
    d = _shifted(3, -1.0e4)
    s = assert_same_bits(d, inp, inp.shape[0], monkeypatch)
    assert not torch.equal(s, ref)               # (the shift did change the decoder)
    d = _shifted(5, -1.0e4)                      # a plain layer all off: an empty K list (bias only downstream)
    assert_same_bits(d, inp, inp.shape[0], monkeypatch)


def test_layer_with_no_feature_zero(monkeypatch):
    """layer 1 all on at every point: the next K list is the full width"""
    d = _shifted(1, 1.0e3)
    inp = grid_inputs([[0.3, -0.5, 0.8]])
    assert_same_bits(d, inp, inp.shape[0], monkeypatch)


def test_batch_renderer_step_bitwise(dec, monkeypatch):
    """one full fwd + bwd step of the headline workload (256x256, grid 40): images, points, band, gradients"""
    H = W = 256
    K = K_for(H, W)
    br = sdflabel_amd.BatchRenderer(dec, 40, K, (W, H), 1, device=DEV)
    args = (torch.tensor([0.6], device=DEV), torch.tensor([[0.0, 0.0, 3.5]], device=DEV), torch.tensor([[0.3, -0.5, 0.8]], device=DEV))
    res = []
    for compact in (False, True):
        monkeypatch.setenv("SDFR_FWD_COMPACT", "1" if compact else "0")
        out = br.forward(*args)
        out = {k: v.clone() for k, v in out.items() if torch.is_tensor(v)}
        grads = [g.clone() for g in br.backward(g_color=torch.ones(1, 3, H, W, device=DEV), g_xyzf=torch.ones(1, br.cap, 3, device=DEV))]
        torch.cuda.synchronize()
        res.append((out, grads, br.sdf.clone(), br.mask_ws.clone()))
    (o0, g0, s0, m0), (o1, g1, s1, m1) = res
    assert int(o1["n"][0]) > 0
    assert o0.keys() == o1.keys()
    for k in o0:
        assert torch.equal(o0[k], o1[k]), k
    for a, b in zip(g0, g1):
        assert torch.equal(a, b)
    assert torch.equal(s0.view(torch.int32), s1.view(torch.int32)) and torch.equal(m0, m1)
