"""The K compaction of the band Jacobian (16-row float32 mask-fed kernel: mlp_kernel.h KCJ, csrc/kcj_slots.h) against the full
K chain and the float64 reference.  sdfr_mlp_jacobian is driven with CRAFTED mask buffers (layout v2, tests/_decoder_ref.mask_encode; the
masks need not come from a forward), so that every survivor pattern is reached with at most 33 selected rows of Grid3D(8): J and sdf_sel
are compared bit for bit between SDFR_JAC_COMPACT=1 and =0, and J against the float64 Jacobian of the same masks within the bound of
tests/test_gpu_decoder_ref.py::test_mask_fed_jacobian_every_entry (judge_jac_masks, ratio <= 1)."""
import functools

import numpy as np
import pytest
import torch

import sdflabel_amd
from sdflabel_amd import _lib
from sdflabel_amd.fixtures import ASSET, K_for
from tests import _decoder_cases as C
from tests import _decoder_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAME = "asset"                              # 8 x 512, latent_in = [4]: layer 3 has 506 outputs, layer 4 re-injects the input row
G, CAP, HP = 512, 40, 512
T = lambda a, dt=torch.float32: torch.as_tensor(np.array(a), dtype=dt, device=DEV)
N = lambda t: t.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def setup():
    """net, handle, the rows (unit latent + Grid3D(8) points) on host and device"""
    net = C.net(NAME)
    h = C.decoders()[NAME].handle(torch.device(DEV))
    pts = N(sdflabel_amd.Grid3D(8, DEV).points).astype(np.float32)
    assert pts.shape == (G, 3)
    lat = np.array([0.3, -0.5, 0.8], np.float32)
    lat /= np.linalg.norm(lat)
    x = np.concatenate([np.broadcast_to(lat, (G, net.n_inputs - 3)), pts], 1).astype(np.float32)
    return net, h, x, T(x)


def forward_values(bits, rows):
    """the decoder output the forward would have saved next to these masks: the reference's value on the branch the masks select (G floats,
    0 at the rows not selected) -- the kernel takes d out / d y = 1 - out^2 from it"""
    net, h, x, d_x = setup()
    rm = R.evaluate(net, x[rows], "f32", masks=[bits[rows, l, :od] for l, od in enumerate(net.out_dims)], bwd="f32", want_masses=False)
    sdf = np.zeros(G, np.float32)
    sdf[rows] = rm.out.astype(np.float32)
    return sdf


def launch(bits, sdf, crops, rpc, compact, monkeypatch):
    """crops: per crop the selected rows (relative to the crop's rows_per_crop = rpc rows).  Returns {absolute row: (J row, sdf_sel)}."""
    net, h, x, d_x = setup()
    d_sdf = T(sdf)
    L = _lib.lib()
    monkeypatch.setenv("SDFR_JAC_COMPACT", compact)
    B = len(crops)
    idx = np.zeros((B, CAP), np.int32)
    cnt = np.array([len(c) for c in crops], np.int32)
    assert cnt.max() < CAP
    for b, c in enumerate(crops):
        idx[b, :len(c)] = c
    ws = T(R.mask_encode(bits).view(np.int32), torch.int32)
    assert ws.numel() == int(L.sdfr_decoder_mask_words(h.h, G))
    J = torch.full((B, CAP, net.n_inputs), C.SENTINEL, device=DEV)
    sel = torch.full((B, CAP), C.SENTINEL, device=DEV)
    d_idx, d_cnt = T(idx, torch.int32), T(cnt, torch.int32)
    _lib.check(L.sdfr_mlp_jacobian(h.h, _lib.ptr(d_x), rpc, B, _lib.ptr(d_idx), CAP, _lib.ptr(d_cnt), _lib.ptr(J), _lib.ptr(sel), _lib.ptr(d_sdf),
                                   _lib.ptr(ws), 0, _lib.stream_ptr()), "sdfr_mlp_jacobian")
    torch.cuda.synchronize()
    J, sel = N(J), N(sel)
    live = np.arange(CAP)[None, :] < cnt[:, None]
    assert (J[~live] == C.SENTINEL).all() and (sel[~live] == C.SENTINEL).all(), "slots beyond cnt[b] written"
    out = {}
    for b, c in enumerate(crops):
        for s, r in enumerate(c):
            out[b * rpc + int(r)] = (J[b, s].copy(), sel[b, s])
    return out


def both_ways(bits, crops, rpc, monkeypatch):
    """compacted and full chain: bit-equal; the compacted J within the reference bound; sdf_sel the supplied value.  Returns the compacted result."""
    net, h, x, d_x = setup()
    rows = np.sort(np.concatenate([b * rpc + np.asarray(c) for b, c in enumerate(crops)]))
    sdf = forward_values(bits, rows)
    a = launch(bits, sdf, crops, rpc, "1", monkeypatch)
    b = launch(bits, sdf, crops, rpc, "0", monkeypatch)
    assert sorted(a) == rows.tolist()
    Ja, Jb = np.stack([a[r][0] for r in rows]), np.stack([b[r][0] for r in rows])
    assert np.array_equal(Ja.view(np.uint32), Jb.view(np.uint32)), "compacted J differs from the full chain's"
    assert all(a[r][1] == sdf[r] and b[r][1] == sdf[r] for r in rows), "sdf_sel is not the supplied value"
    masks = [bits[rows, l, :od] for l, od in enumerate(net.out_dims)]
    ratio = R.judge_jac_masks(net, x[rows], masks, Ja, "f32", "f32")
    print("JACCOMPACT max ratio %.4f over %d rows" % (float(ratio.max()), len(rows)))
    assert ratio.max() <= 1, (np.unravel_index(ratio.argmax(), ratio.shape), float(ratio.max()))
    return a


def spread(rng, rows, alive, p=0.6):
    """bits (G, HP) of one layer: feature j of `alive` is set in each selected row with probability p and surely in one of them"""
    out = np.zeros((G, HP), bool)
    alive = np.asarray(alive, np.int64)
    if len(alive):
        sub = rng.random((len(rows), len(alive))) < p
        sub[rng.integers(0, len(rows), len(alive)), np.arange(len(alive))] = True
        out[np.ix_(rows, alive)] = sub
    return out


def layer_bits(rng, rows, per_layer):
    """per_layer: for each hidden layer the surviving features"""
    return np.stack([spread(rng, rows, a) for a in per_layer], 1)


ROWS17 = np.array([3, 77, 78, 79, 130, 131, 200, 255, 256, 257, 300, 383, 384, 400, 470, 510, 511])


# different survivor counts in different layers of one launch; 0 directly above and below 512 (layer 3 has 506 outputs: "512" is all of them)
COUNTS = [(512, 0, 512, 1, 15, 16, 17, 31), (32, 33, 512, 512, 0, 512, 16, 1), (17, 31, 32, 33, 512, 15, 0, 512), (1, 1, 1, 1, 1, 1, 1, 1),
          (512, 512, 512, 512, 512, 512, 512, 512), (16, 32, 64, 48, 63, 65, 128, 129)]


@pytest.mark.parametrize("counts", COUNTS)
def test_survivor_counts_per_layer(counts, monkeypatch):
    net = setup()[0]
    rng = np.random.default_rng(sum(counts))
    per_layer = [rng.permutation(od)[:min(c, od)] for c, od in zip(counts, net.out_dims)]
    both_ways(layer_bits(rng, ROWS17, per_layer), [ROWS17], G, monkeypatch)


PLACEMENTS = {"wave3": lambda j: j >= 384, "lane_group3": lambda j: (j >> 2) & 3 == 3, "component3": lambda j: j & 3 == 3,
              "first_tile": lambda j: j < 16, "last_tile_of_wave0": lambda j: (j >= 112) & (j < 128)}


@pytest.mark.parametrize("where", sorted(PLACEMENTS))
def test_survivor_placement(where, monkeypatch):
    net = setup()[0]
    rng = np.random.default_rng(5)
    per_layer = [np.flatnonzero(PLACEMENTS[where](np.arange(od))) for od in net.out_dims]
    both_ways(layer_bits(rng, ROWS17, per_layer), [ROWS17], G, monkeypatch)


def test_union_over_rows_each_survivor_alive_in_one_row_only(monkeypatch):
    """a union taken over too few lanes loses survivors: feature number i of a layer's survivors lives in row i % 16 of the tile alone"""
    net = setup()[0]
    rng = np.random.default_rng(6)
    rows = ROWS17[:16]
    bits = np.zeros((G, len(net.out_dims), HP), bool)
    for l, od in enumerate(net.out_dims):
        alive = np.sort(rng.permutation(od)[:48])
        bits[rows[(np.arange(48) + l) % 16], l, alive] = True
    both_ways(bits, [rows], G, monkeypatch)


@pytest.mark.parametrize("set_bits", [True, False])
def test_reinjection_layer_bits_beyond_the_layer_width(set_bits, monkeypatch):
    """mask bits of features 506 ... 511 of layer 3 (padding and the slots of the re-injected latent) set or clear: the same J either way"""
    net = setup()[0]
    assert net.out_dims[3] == 506
    rng = np.random.default_rng(7)
    bits = np.zeros((G, len(net.out_dims), HP), bool)
    bits[ROWS17] = rng.random((len(ROWS17), len(net.out_dims), HP)) < 0.5
    for l, od in enumerate(net.out_dims):
        bits[:, l, od:] = False
    bits[ROWS17, 3, 506:] = set_bits
    got = both_ways(bits, [ROWS17], G, monkeypatch)
    bits[ROWS17, 3, 506:] = False
    ref = launch(bits, forward_values(bits, ROWS17), [ROWS17], G, "0", monkeypatch)
    assert all(np.array_equal(got[r][0].view(np.uint32), ref[r][0].view(np.uint32)) for r in ref)


def random_bits(seed, density, rows):
    net = setup()[0]
    rng = np.random.default_rng(seed)
    bits = np.zeros((G, len(net.out_dims), HP), bool)
    bits[rows] = rng.random((len(rows), len(net.out_dims), HP)) < density
    for l, od in enumerate(net.out_dims):
        bits[:, l, od:] = False
    return bits


@pytest.mark.parametrize("density", [0.3, 0.5])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_random_masks(seed, density, monkeypatch):
    both_ways(random_bits(seed, density, ROWS17), [ROWS17], G, monkeypatch)


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("n", [1, 15, 16, 17, 33])
def test_selected_row_counts(n, B, monkeypatch):
    rng = np.random.default_rng(10 * n + B)
    rpc = G // B
    crops = [np.sort(rng.permutation(rpc)[:n]) if b == 0 else np.sort(rng.permutation(rpc)[:max(1, n - 1)]) for b in range(B)]
    rows = np.concatenate([b * rpc + c for b, c in enumerate(crops)])
    both_ways(random_bits(n, 0.1, rows), crops, rpc, monkeypatch)


def test_32_row_geometry_returns_the_compacted_bits(monkeypatch):
    """the same rows through the 32-row kernel (8 crops per launch; it keeps the full chain): bit-equal to the compacted 16-row result"""
    rng = np.random.default_rng(11)
    rows = np.sort(rng.permutation(G)[:33])
    bits = random_bits(12, 0.4, rows)
    one = both_ways(bits, [rows], G, monkeypatch)
    rpc = G // 8
    crops = [rows[(rows >= b * rpc) & (rows < (b + 1) * rpc)] - b * rpc for b in range(8)]
    many = launch(bits, forward_values(bits, rows), crops, rpc, "1", monkeypatch)
    assert sorted(many) == sorted(one)
    assert all(np.array_equal(many[r][0].view(np.uint32), one[r][0].view(np.uint32)) for r in one)


def test_masks_of_a_real_forward(monkeypatch):
    """BatchRenderer.forward() at D = 8: the Jacobian of its band from its own masks, compacted and not"""
    net = setup()[0]
    dec = sdflabel_amd.setup_dsdf(ASSET + ".pt", precision=torch.float32)[0].to(DEV)        # (a decoder of its own: the cached one stays on the host)
    br = sdflabel_amd.BatchRenderer(dec, 8, K_for(64, 64), (64, 64), 1, device=DEV)
    br.set_params(torch.full((1,), 0.7, device=DEV), torch.tensor([[0.05, 0.02, 3.3]], device=DEV), torch.tensor([[0.3, -0.5, 0.8]], device=DEV))
    br.forward()
    torch.cuda.synchronize()
    cnt = int(br.cnt[0])
    assert 0 < cnt <= br.cap
    L, P = _lib.lib(), _lib.ptr
    got = {}
    for compact in ("1", "0"):
        monkeypatch.setenv("SDFR_JAC_COMPACT", compact)
        br.J.fill_(C.SENTINEL)
        _lib.check(L.sdfr_mlp_jacobian(br.handle.h, P(br.inputs), br.G, 1, P(br.idx), br.cap, P(br.cnt), P(br.J), P(br.sdf_band), P(br.sdf), P(br.mask_ws),
                                       0, _lib.stream_ptr()), "sdfr_mlp_jacobian")
        torch.cuda.synchronize()
        got[compact] = N(br.J)[0, :cnt].copy()
    assert np.array_equal(got["1"].view(np.uint32), got["0"].view(np.uint32))
    rows = N(br.idx)[0, :cnt]
    bits = R.mask_decode(N(br.mask_ws), rows, len(net.out_dims), HP)
    masks = [bits[:, l, :od] for l, od in enumerate(net.out_dims)]
    ratio = R.judge_jac_masks(net, N(br.inputs)[rows], masks, got["1"], "f32", "f32")
    print("JACCOMPACT real forward: %d band rows, max ratio %.4f" % (cnt, float(ratio.max())))
    assert ratio.max() <= 1, float(ratio.max())
