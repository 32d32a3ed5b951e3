"""GPU tests of the exact-f32 grid forward's two tile geometries (mlp_fwd32.hip): 64-row tiles, one workgroup per CU
(SDFR_FWD_TILE=64), and 32-row tiles, two resident workgroups per CU (SDFR_FWD_TILE=32).  With and without per-tile K compaction
(SDFR_FWD_COMPACT), with and without a mask buffer, every sdf value and every saved ReLU mask word of every row of the launch must be bit
for bit the same under both geometries, and so must one full BatchRenderer step.

Mask words are compared for the rows of the launch.  The mask buffer is padded to whole 128-row blocks; what a launch leaves in the padding
rows behind its last row depends on its tile size (a partial tile writes the bits of mirrored rows up to the end of the TILE) and nothing
reads it."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import sdflabel_amd
from sdflabel_amd import _lib
from sdflabel_amd.fixtures import ASSET, ASSET_ELLIPSOID, K_for

pytestmark = pytest.mark.gpu
DEV = "cuda"
TILES = ("64", "32")


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


@pytest.fixture(scope="module")
def grid40():
    return grid_inputs([[0.3, -0.5, 0.8]])


def forward(dec, inputs, n, tile, compact, monkeypatch, masks=True):
    L = _lib.lib()
    h = dec.handle(torch.device(DEV)).h
    sdf = torch.full((n,), float("nan"), device=DEV)
    mw = torch.zeros(int(L.sdfr_decoder_mask_words(h, n)), dtype=torch.int32, device=DEV) if masks else None
    monkeypatch.setenv("SDFR_FWD_TILE", tile)
    monkeypatch.setenv("SDFR_FWD_COMPACT", "1" if compact else "0")
    _lib.check(L.sdfr_mlp_forward(h, _lib.ptr(inputs), n, _lib.ptr(sdf), _lib.ptr(mw) if masks else None, _lib.stream_ptr()),
               "sdfr_mlp_forward")
    torch.cuda.synchronize()
    return sdf, mw


def mask_rows(mw, n, n_layers=8, hp32=16):
    """the mask words of rows 0 .. n-1 (layout v2: [block of 128 rows][layer][row in block][HP / 32 dwords]) as [layer][row][dword]"""
    v = mw.view(-1, n_layers, 128, hp32).permute(1, 0, 2, 3).reshape(n_layers, -1, hp32)
    return v[:, :n]


def assert_same_bits(dec, inputs, n, monkeypatch):
    """tile 64 against tile 32, compaction off and on, with and without a mask buffer: one set of bits"""
    ref_s = ref_m = None
    for masks in (True, False):                  # MODE 1 (masks saved) and the same launch without a mask buffer (MODE 0 use)
        for compact in (False, True):
            for tile in TILES:
                s, m = forward(dec, inputs, n, tile, compact, monkeypatch, masks)
                if ref_s is None:
                    ref_s, ref_m = s, mask_rows(m, n)
                    assert ref_m.shape[1] == n
                    continue
                assert torch.equal(ref_s.view(torch.int32), s.view(torch.int32)), (tile, compact, masks)
                if masks:
                    assert torch.equal(ref_m, mask_rows(m, n)), (tile, compact, masks)
    return ref_s


@pytest.mark.parametrize("n", [1, 31, 32, 33, 63, 65, 1000])
def test_row_counts_bitwise(dec, grid40, n, monkeypatch):
    """partial-tile edges of both tile sizes"""
    s = assert_same_bits(dec, grid40, n, monkeypatch)
    assert torch.isfinite(s).all()


@pytest.mark.parametrize("asset", [ASSET, ASSET_ELLIPSOID])
def test_whole_grid_bitwise(asset, monkeypatch):
    d = _decoder(asset)
    inp = grid_inputs([[0.3, -0.5, 0.8]], density=20)
    assert inp.shape[0] == 8000
    s = assert_same_bits(d, inp, inp.shape[0], monkeypatch)
    assert torch.isfinite(s).all()


def test_batch_of_three_crops_bitwise(dec, monkeypatch):
    """12^3 = 1728 rows per crop = 54 tiles of 32: tiles of both sizes span crop boundaries"""
    inp = grid_inputs([[0.3, -0.5, 0.8], [1.0, 0.2, -0.4], [-0.7, -0.7, 0.1]], density=12)
    assert inp.shape[0] == 3 * 1728
    assert_same_bits(dec, inp, inp.shape[0], monkeypatch)


def test_random_rows_bitwise(dec, monkeypatch):
    """rows with no spatial coherence: few features are dead across a tile (long K lists)"""
    g = torch.Generator(device=DEV).manual_seed(3)
    inp = torch.rand(32 * 50 + 5, 6, device=DEV, generator=g) * 2 - 1
    assert_same_bits(dec, inp, inp.shape[0], monkeypatch)


def _shifted(layer, shift):
    d = _decoder()
    with torch.no_grad():
        getattr(d, "lin%d" % layer).bias.add_(shift)
    return d


@pytest.mark.parametrize("layer", [3, 5])
def test_layer_with_every_feature_zero(dec, grid40, layer, monkeypatch):
    """layer 3 (in front of latent_in) all off: the next K list holds only the re-injected columns; layer 5: an empty K list"""
    n = 2000
    ref, _ = forward(dec, grid40, n, "64", True, monkeypatch)
    s = assert_same_bits(_shifted(layer, -1.0e4), grid40, n, monkeypatch)
    assert not torch.equal(s, ref)               # (the shift did change the decoder)


def test_layer_with_no_feature_zero(grid40, monkeypatch):
    """layer 1 all on at every point: the next K list is the full width"""
    assert_same_bits(_shifted(1, 1.0e3), grid40, 2000, monkeypatch)


def test_batch_renderer_step_bitwise(dec, monkeypatch):
    """one full fwd + bwd step at 64x64 pixels, grid 20: every output tensor and every gradient, tile 64 against tile 32"""
    H = W = 64
    K = K_for(H, W)
    br = sdflabel_amd.BatchRenderer(dec, 20, K, (W, H), 1, device=DEV)
    args = (torch.tensor([0.6], device=DEV), torch.tensor([[0.0, 0.0, 3.5]], device=DEV), torch.tensor([[0.3, -0.5, 0.8]], device=DEV))
    res = []
    for tile in TILES:
        monkeypatch.setenv("SDFR_FWD_TILE", tile)
        out = br.forward(*args)
        out = {k: v.clone() for k, v in out.items() if torch.is_tensor(v)}
        grads = [g.clone() for g in br.backward(g_color=torch.ones(1, 3, H, W, device=DEV), g_xyzf=torch.ones(1, br.cap, 3, device=DEV))]
        torch.cuda.synchronize()
        res.append((out, grads, br.sdf.clone(), mask_rows(br.mask_ws, 8000).clone()))
    (o0, g0, s0, m0), (o1, g1, s1, m1) = res
    assert int(o1["n"][0]) > 0
    assert o0.keys() == o1.keys()
    for k in o0:
        assert torch.equal(o0[k], o1[k]), k
    assert len(g0) == len(g1) and len(g0) > 0
    for a, b in zip(g0, g1):
        assert torch.equal(a, b)
    assert torch.equal(s0.view(torch.int32), s1.view(torch.int32)) and torch.equal(m0, m1)
