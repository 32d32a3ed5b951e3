"""The tile order of the exact-f32 grid forward (include/sdfr.h: sdfr_grid_tile_order, sdfr_mlp_forward_ordered), without a GPU:
the order is a permutation made of 4x4x4 blocks, the ordered entry refuses bad arguments before it touches the device, and on the committed
decoders the blocked tiles leave the per-tile K compaction clearly less work than 64 consecutive rows do."""
import ctypes

import numpy as np
import pytest
import torch

import sdflabel_amd
from sdflabel_amd import _lib
from sdflabel_amd.fixtures import ASSET, ASSET_ELLIPSOID, crop_start


def tile_order(D):
    out = np.full(D ** 3, -1, np.int32)
    assert _lib.lib().sdfr_grid_tile_order(D, out.ctypes.data) == 0
    return out


@pytest.mark.parametrize("D", [1, 3, 4, 5, 8, 40])
def test_order_is_a_permutation(D):
    o = tile_order(D)
    assert np.array_equal(np.sort(o), np.arange(D ** 3))


def test_order_walks_clipped_blocks_in_lexicographic_order():
    """D = 5: blocks (0,0,0) 4x4x4, (0,0,1) 4x4x1, (0,1,0) 4x1x4, ... each in (x, y, z) order"""
    D = 5
    expect = []
    for bx in range(0, D, 4):
        for by in range(0, D, 4):
            for bz in range(0, D, 4):
                for x in range(bx, min(bx + 4, D)):
                    for y in range(by, min(by + 4, D)):
                        for z in range(bz, min(bz + 4, D)):
                            expect.append((x * D + y) * D + z)
    assert tile_order(D).tolist() == expect


@pytest.mark.parametrize("D", [8, 40])
def test_every_64_entries_are_one_block(D):
    o = tile_order(D).reshape(-1, 64).astype(np.int64)
    x, y, z = o // (D * D), (o // D) % D, o % D
    for c in (x, y, z):
        assert (c.min(1) % 4 == 0).all() and (c.max(1) - c.min(1) == 3).all()
    # blocks in lexicographic order, rows inside a block in (x, y, z) order; a 32-row tile is the 2x4x4 half of a block
    key = (x[:, 0] // 4 * (D // 4) + y[:, 0] // 4) * (D // 4) + z[:, 0] // 4
    assert np.array_equal(key, np.arange(o.shape[0]))
    assert (np.diff(o, axis=1) > 0).all()
    assert (x[:, :32].max(1) - x[:, :32].min(1) == 1).all()


def test_order_refuses_bad_arguments():
    L = _lib.lib()
    buf = np.zeros(8, np.int32)
    assert L.sdfr_grid_tile_order(2, None) == -1 and b"NULL" in L.sdfr_last_error()
    assert L.sdfr_grid_tile_order(0, buf.ctypes.data) == -1 and b"D=0" in L.sdfr_last_error()
    assert L.sdfr_grid_tile_order(1025, buf.ctypes.data) == -1
    assert not buf.any()


def test_ordered_entry_validates_before_any_device_call():
    """no decoder is ever dereferenced and no HIP call is made: these checks need no GPU"""
    L = _lib.lib()
    fake = ctypes.create_string_buffer(64)                      # stands in for every pointer; a refused call reads none of them
    p = ctypes.addressof(fake)
    cases = [((None, p, 64, p, None, p, 64, None), b"NULL"),
             ((p, None, 64, p, None, p, 64, None), b"NULL"),
             ((p, p, 64, None, None, p, 64, None), b"NULL"),
             ((p, p, 64, p, None, None, 64, None), b"NULL"),
             ((p, p, 64, p, None, p, 0, None), b"order_rows=0"),
             ((p, p, 64, p, None, p, -5, None), b"order_rows=-5"),
             ((p, p, 100, p, None, p, 64, None), b"not a multiple"),
             ((p, p, -64, p, None, p, 64, None), b"out of range")]
    for args, msg in cases:
        assert L.sdfr_mlp_forward_ordered(*args) == -1, args
        assert msg in L.sdfr_last_error(), (msg, L.sdfr_last_error())


def _alive(asset, latents, D=40):
    """The decoder restated in float32 torch on the fixture's effective weights: per hidden layer lin1 .. lin7, which operand features are
    non-zero at each grid row ([layer] -> bool [rows, features]); re-injected input columns always count (the kernel keeps them)."""
    dec, _ = sdflabel_amd.setup_dsdf(asset + ".pt", precision=torch.float32)
    layers, inject = dec.effective_layers(), dec._inject_table()
    pts = sdflabel_amd.Grid3D(D, "cpu").points.detach()
    out = []
    for lat in latents:
        lat = torch.nn.functional.normalize(torch.as_tensor(lat, dtype=torch.float32).view(1, -1), p=2, dim=1)
        x0 = torch.cat([lat.expand(pts.shape[0], -1), pts], 1)
        x, per_layer = x0, []
        for l, ((W, b), (inj_n, inj_off)) in enumerate(zip(layers, inject)):
            if inj_n:
                x = torch.cat([x, x0[:, inj_off:inj_off + inj_n]], 1)
            if l == len(layers) - 1:                            # the last linear reads the full operand: no compaction in front of it
                break
            if l > 0:
                nz = x != 0
                nz[:, x.shape[1] - inj_n:] = True
                per_layer.append(nz)
            x = torch.relu(x @ torch.from_numpy(W).t() + torch.from_numpy(b))
        assert len(per_layer) == 7
        out.append(per_layer)
    return out


def _k_share(alive, order):
    """share of the hidden layers' K work the compaction leaves: per 64-slot tile and layer the features alive at some row, rounded up to 16"""
    work = tiles = 0
    for per_layer in alive:
        for nz in per_layer:
            t = nz[order].view(-1, 64, nz.shape[1]).any(1).sum(1)
            work += int(((t + 15) // 16 * 16).sum())
            tiles += t.shape[0]
    return work / (512.0 * tiles)


@pytest.mark.parametrize("asset", [ASSET, ASSET_ELLIPSOID])
def test_blocked_tiles_leave_less_k_work(asset):
    """Start latents of crops 0 and 5 at D = 40.  Measured when this test was written: consecutive 0.538 / 0.538, blocked 0.466 / 0.462 of the
    full K work, ratio 0.867 (deepsdf_synth) and 0.859 (ellipsoid).  The bound 0.90 only guards against an order that silently stops being
    blocked."""
    alive = _alive(asset, [crop_start(0)[2], crop_start(5)[2]])
    order = torch.from_numpy(tile_order(40).astype(np.int64))
    plain, blocked = _k_share(alive, torch.arange(64000)), _k_share(alive, order)
    print("K share left, %s: consecutive %.4f, 4x4x4 blocks %.4f, ratio %.4f" % (asset.rsplit("/", 1)[-1], plain, blocked, blocked / plain))
    assert 0.0 < blocked / plain < 0.90
