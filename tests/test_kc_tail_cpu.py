"""CPU tests of the tails of the compacted products (csrc/kc_slots.h: sdfr_kc_steps; csrc/kcj_slots.h: sdfr_kcj_tiles; mlp_kernel.h:
gemm_kc_body of the 64-row kernels and gemm_kcj).  The products run the whole trips of their ring loops and the steps that are
left over behind the loop's exit, from the stages the ring has filled by then, and stop behind the last chain step (forward: two chain
positions) or k tile (Jacobian: sixteen) that holds a survivor.

tests/kc_tail_host walks prologue, loop and tail with the headers' own arithmetic for every survivor total 0 .. 512, tail on and off, and
logs every consumed group of matrix instructions with what its emulated registers hold.  The rule is restated here, from the log alone:
the consumed (tile, component) pairs are exactly those that hold a live chain position (tail off: exactly the padded extent), each once
and in order, each from the fragment gathered for its own tile, and the k word a lane group meets there is the survivor of that chain
position or a pad entry.  The program's k list and operand have exactly the padded extent, and it also runs under ASan and UBSan.

The second half recomputes the model the change was chosen by: the decoder restated on the CPU (tests/test_fwd_order_cpu.py for the grid
forward, the rule of tools/jac_survivors.py for the band), per tile and layer the survivors, and the share of the hidden layers' K chain
the products execute under each padding rule."""
import subprocess

import numpy as np
import pytest
import torch

from sdflabel_amd.fixtures import ASSET, ASSET_ELLIPSOID, crop_start
from tests._util import build_host_program
from tests.test_fwd_order_cpu import _alive, tile_order

SRC = "kc_tail_host/kc_tail_host.cpp"
TOTALS = list(range(513))
PAD = -1


def run(exe, tmp):
    dst = str(tmp / "tail.bin")
    r = subprocess.run([exe, dst], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    assert r.stdout.split() == ["cases", str(2 * len(TOTALS)), "bad", "0"]
    rec = np.fromfile(dst, np.int32).reshape(-1, 8)
    return {(k, tail): rec[(rec[:, 0] == k) & (rec[:, 1] == tail)][:, 2:] for k in (0, 1) for tail in (0, 1)}


def by_total(ev):
    """{tot: {lane group: [(tile the loop is at, tile of the fragment, component / operand tile, word)]}} in the order of the log"""
    out = {t: {} for t in TOTALS}
    for tot, lg, at, frag, comp, word in ev.tolist():
        out[tot].setdefault(lg, []).append((at, frag, comp, word))
    return out


def check_forward(tot, tail, groups):
    """chain step (t, ks) reads the chain positions 8 t + 2 ks + lane group"""
    padded = (tot + 15) // 16 * 16
    if tot == 0:
        assert groups == {}                                                         # no product at all
        return
    live = sorted({(p // 8, (p % 8) // 2) for p in range(tot)})
    want = live if tail else [(t, c) for t in range(padded // 8) for c in range(4)]
    assert len(want) == ((tot + 1) // 2 if tail else padded // 2)
    for lg in (0, 1):
        ev = groups[lg]
        assert [(at, comp) for at, _, comp, _ in ev] == want                        # exactly these, each once, in order
        assert all(frag == at for at, frag, _, _ in ev)                             # ... from the fragment gathered for that tile
        for at, _, comp, word in ev:
            pos = 8 * at + 2 * comp + lg
            assert pos < padded and word == (pos if pos < tot else PAD)             # the survivor of that chain position, or a pad


def check_jacobian(tot, tail, groups):
    """k tile t holds the chain positions 16 t .. 16 t + 15"""
    padded = max(64, (tot + 63) // 64 * 64)
    want = list(range(max(1, (tot + 15) // 16))) if tail else list(range(padded // 16))
    assert set(want) >= {p // 16 for p in range(tot)}
    for lg in range(4):
        ev = groups[lg]
        assert [at for at, _, _, _ in ev] == want
        assert all(frag == at and oper == at for at, frag, oper, _ in ev)           # its own tile's weights and operand
        for at, _, _, word in ev:
            pos = 16 * at + lg
            assert pos < padded and word == (pos if pos < tot else PAD)


@pytest.fixture(scope="module")
def events(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("kc_tail_host")
    return {k: by_total(v) for k, v in run(build_host_program(tmp, SRC, "kc_tail_host"), tmp).items()}


@pytest.mark.parametrize("tail", [1, 0])
def test_forward_steps(tail, events):
    for tot in TOTALS:
        check_forward(tot, tail, events[(0, tail)][tot])


@pytest.mark.parametrize("tail", [1, 0])
def test_jacobian_tiles(tail, events):
    for tot in TOTALS:
        check_jacobian(tot, tail, events[(1, tail)][tot])


def test_the_check_itself_sees_a_lost_step_and_a_wrong_stage(events):
    g = {lg: list(ev) for lg, ev in events[(0, 1)][21].items()}                     # 21 survivors: one trip and a tail of three steps
    check_forward(21, 1, g)
    with pytest.raises(AssertionError):
        check_forward(21, 1, {0: g[0][:-1], 1: g[1]})                               # the last chain step lost
    at, frag, comp, word = g[0][8]
    with pytest.raises(AssertionError):
        check_forward(21, 1, {0: g[0][:8] + [(at, frag + 1, comp, word)] + g[0][9:], 1: g[1]})      # the first tail step from stage 1
    j = {lg: list(ev) for lg, ev in events[(1, 1)][65].items()}
    check_jacobian(65, 1, j)
    with pytest.raises(AssertionError):
        check_jacobian(65, 1, {**j, 2: j[2][:-1]})


def test_header_on_the_host_under_the_sanitizers(tmp_path):
    exe = build_host_program(tmp_path, SRC, "kc_tail_host_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    ev = {k: by_total(v) for k, v in run(exe, tmp_path).items()}
    for tot in (0, 1, 15, 16, 17, 63, 64, 65, 511, 512):
        check_forward(tot, 1, ev[(0, 1)][tot])
        check_jacobian(tot, 1, ev[(1, 1)][tot])


# ---- the model ------------------------------------------------------------------------------------------------------------------------
def forward_shares(alive, order):
    """share of the seven hidden products' K chain that is executed when a tile's survivors are padded to 16, 8, 2 and 1: per 64-slot tile
    of the order and layer the features alive at some row; mean over tiles, layers and latents"""
    counts = torch.cat([nz[order].view(-1, 64, nz.shape[1]).any(1).sum(1) for per_layer in alive for nz in per_layer]).numpy().astype(np.int64)
    return {g: float(((counts + g - 1) // g * g).sum()) / (512.0 * counts.size) for g in (16, 8, 2, 1)}


def jacobian_shares(asset, latent, D=40, thr=0.03):
    """the band |sdf| < thr in grid order cut into tiles of 16 rows, the ReLU masks of the layers 1 .. 7 (the seven compacted products), per
    tile and layer the features whose mask bit is set in some row: K executed with whole trips of 64 and with whole k tiles of 16 (at least
    one), as (mean over tiles, slowest tile) of the share of 7 x 512"""
    import sdflabel_amd
    dec, _ = sdflabel_amd.setup_dsdf(asset + ".pt", precision=torch.float32)
    layers, inject = dec.effective_layers(), dec._inject_table()
    pts = sdflabel_amd.Grid3D(D, "cpu").points.detach()
    lat = torch.nn.functional.normalize(torch.as_tensor(latent, dtype=torch.float32).view(1, -1), p=2, dim=1)
    x0 = torch.cat([lat.expand(pts.shape[0], -1), pts], 1)
    x, masks = x0, []
    for l, ((W, b), (inj_n, inj_off)) in enumerate(zip(layers, inject)):
        if inj_n:
            x = torch.cat([x, x0[:, inj_off:inj_off + inj_n]], 1)
        x = x @ torch.from_numpy(W).t() + torch.from_numpy(b)
        if l < len(layers) - 1:
            masks.append(x > 0)
            x = torch.relu(x)
    band = torch.nonzero(torch.tanh(x)[:, 0].abs() < thr)[:, 0] if dec.use_tanh else torch.nonzero(x[:, 0].abs() < thr)[:, 0]
    n_tiles = (band.numel() + 15) // 16
    counts = np.stack([[int(m[band[16 * t:16 * t + 16]].any(0).sum()) for t in range(n_tiles)] for m in masks[1:]], 1)      # [tile][layer]
    assert counts.shape == (n_tiles, 7)
    out = {"rows": int(band.numel())}
    for g in (64, 16):
        per_tile = np.maximum(g, (counts + g - 1) // g * g).sum(1) / (7 * 512.0)
        out[g] = (float(per_tile.mean()), float(per_tile.max()))
    return out


@pytest.mark.parametrize("asset", [ASSET, ASSET_ELLIPSOID], ids=["rounded_box", "ellipsoid"])
def test_the_model_recomputed(asset):
    """Start latents of crops 0 and 5 at D = 40.  Measured when this test was written (rounded box / ellipsoid): see profiles/kc_tail_notes.md,
    section 1.  The bound on the 8-k share against the 16-k share, ratio inside [0.975, 0.995], guards against a model that silently stops
    measuring padding: without padding the ratio is 1, and a tile whose counts were uniform over the residues of 16 would lose 4 of a mean
    of about 240, ratio 0.983."""
    latents = [crop_start(0)[2], crop_start(5)[2]]
    order = torch.from_numpy(tile_order(40).astype(np.int64))
    name = asset.rsplit("/", 1)[-1]
    for i, per_latent in zip((0, 5), _alive(asset, latents)):
        f = forward_shares([per_latent], order)
        print("KCTAIL %s start latent %d: forward K share at 16 / 8 / 2 / none: %.4f %.4f %.4f %.4f; ratios to 16: %.4f %.4f"
              % (name, i, f[16], f[8], f[2], f[1], f[8] / f[16], f[2] / f[16]))
        assert f[1] <= f[2] <= f[8] < f[16] < 1.0
        assert 0.975 <= f[8] / f[16] <= 0.995
    for i, lat in zip((0, 5), latents):
        j = jacobian_shares(asset, lat)
        print("KCTAIL %s start latent %d: %d band rows; Jacobian K share, mean / slowest tile: at 64 %.4f / %.4f, at 16 %.4f / %.4f"
              % (name, i, j["rows"], j[64][0], j[64][1], j[16][0], j[16][1]))
        assert j[16][0] < j[64][0] and j[16][1] <= j[64][1]
