"""The decoder kernels (csrc/mlp*.hip, mlp_kernel.h) against the float64 reference of tests/_decoder_ref.py, through the C ABI: every
output row of every forward path, every saved ReLU mask bit whose decision is certain, every entry of the mask-fed Jacobians (reference
evaluated with the kernel's OWN decoded masks, so nothing is forgiven) and of the recomputing ones (a row with k <= 3 undecidable units
must match one of the 2^k reference Jacobians), each within c u mass of that element's own terms.  The constants come from CPU
emulations (tests/test_decoder_refs_cpu.py), not from the kernels; profiles/decoder_tests_notes.md has the figures.  Every path prints a
line starting DECODERTEST with its largest ratio observed / allowed."""
import functools

import numpy as np
import pytest
import torch

from sdflabel_amd import _lib
from tests import _decoder_cases as C
from tests import _decoder_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MANY = 16                                   # SDFR_JAC_MANY_ROWS
T = lambda a, dt=torch.float32: torch.as_tensor(np.array(a), dtype=dt, device=DEV)
N = lambda t: t.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def handle(name):
    return C.decoders()[name].handle(torch.device(DEV))


@functools.lru_cache(maxsize=None)
def ref(name, arith):
    return R.evaluate(C.net(name), C.rows(name), arith)


def _sub(net, r, rows):
    """view of the reference result r on a subset of its rows (what the forward judges read)"""
    s = R.Result()
    for k in ("y", "y1", "out", "gy", "M_fwd", "M_half"):
        setattr(s, k, getattr(r, k)[rows])
    s.z, s.zmass = [z[rows] for z in r.z], [z[rows] for z in r.zmass]
    return s


def report(path, ratio, free=None, left=None):
    print("DECODERTEST %-44s max ratio %.4f%s%s" % (path, ratio, "" if free is None else "  free units %.2e" % free,
                                                    "" if left is None else "  rows left out %.2e" % left))


FWD = {"f32": "sdfr_mlp_forward", "f16": "sdfr_mlp_forward_f16", "split": "sdfr_mlp_forward_split"}


FILL = 0x5A5A5A5A                           # what the mask workspace holds before a launch


def fwd_tile(net, arith):
    """rows per workgroup of the forward that saves masks"""
    if arith == "f16":
        return 128
    return 64


def check_rows_beyond(ws, n, tile, n_layers, hp):
    """The workspace is sized in blocks of 128 rows and a workgroup stores the mask words of its whole tile: slots n .. end of the last
    tile repeat the tile's first row (the kernels evaluate that row in their idle slots), and nothing is written beyond that tile."""
    w = N(ws).view(np.uint32).reshape(-1, n_layers, 128, hp // 32)
    row = lambda r: w[r >> 7, :, r & 127, :]
    end = -(-n // tile) * tile
    for r in range(n, min(end, w.shape[0] * 128)):
        assert np.array_equal(row(r), row((n - 1) // tile * tile)), "mask words of idle slot %d" % r
    for r in range(end, w.shape[0] * 128):
        assert (row(r) == FILL).all(), "mask words written beyond the last tile (row %d, n = %d)" % (r, n)


def forward(name, arith, x, n, save_masks):
    """sdf (n + 64, sentinel beyond n), decoded masks (n, layers, hp) or None"""
    net, h, L = C.net(name), handle(name), _lib.lib()
    sdf = torch.full((n + 64,), C.SENTINEL, device=DEV)
    ws = None
    if save_masks:
        nw = int(L.sdfr_decoder_mask_words(h.h, n))
        assert nw == R.mask_words(n, net.n_lin - 1, net.hp)
        ws = torch.full((nw,), FILL, dtype=torch.int32, device=DEV)
    _lib.check(getattr(L, FWD[arith])(h.h, _lib.ptr(x), n, _lib.ptr(sdf), _lib.ptr(ws), _lib.stream_ptr()), FWD[arith])
    torch.cuda.synchronize()
    if ws is not None:
        check_rows_beyond(ws, n, fwd_tile(net, arith), net.n_lin - 1, net.hp)
    bits = None if ws is None else R.mask_decode(N(ws), np.arange(n), net.n_lin - 1, net.hp)
    return sdf, bits, ws


def check_masks(name, arith, r, bits):
    net = C.net(name)
    bad, free = R.judge_masks(net, r, bits, arith)
    assert bad == 0, "%d certain units with the wrong mask bit" % bad
    assert free <= (0.05 if arith == "f16" else 1e-3), free
    for l, od in enumerate(net.out_dims):
        pad = bits[:, l, od:]
        if arith != "f16":
            # the exact-f32, split and small-width epilogues store x > 0 of x = 0 + 0: padded features and the slots of re-injected columns are 0
            assert not pad.any(), (l, "padded mask bits set")
        else:
            # the half forward's fast epilogue stores "sign bit clear" (one v_alignbit per value) and x = +0 there: 1.  A wave (64
            # features) whose block touches the slots of the columns re-injected in front of the NEXT layer runs the generic epilogue
            # instead (x > 0: 0) -- unless the decoder has at most 8 input columns, whose re-injection is on the K side (kinj) and
            # leaves every wave on the fast path.  No consumer reads these bits (the Jacobian kernels stop at the layer's width).
            inj_n = net.inj[l + 1][0]
            wave0 = 64 * (np.arange(od, net.hp) // 64)
            generic = (inj_n > 0) & (net.n_inputs > 8) & (wave0 + 64 > od) & (wave0 < od + inj_n)
            assert np.array_equal(pad, np.broadcast_to(~generic, pad.shape)), (l, "padded mask bits of the half forward")
    return free


def _forward_sizes(name, arith, tag=""):
    net, x_all = C.net(name), T(C.rows(name))
    r = ref(name, arith)
    worst, free = 0.0, None
    # every launch size with the masks saved; 129 rows once more without a mask buffer (the half forward has a kernel of its own for that)
    for n, save in [(n, not net.has_ln) for n in C.LAUNCH_SIZES] + ([] if net.has_ln else [(129, False)]):
        x = x_all[:n].contiguous()
        sdf, bits, _ = forward(name, arith, x, n, save)
        out = N(sdf)
        assert (out[n:] == C.SENTINEL).all(), "rows beyond n written (n = %d)" % n
        rs = _sub(net, r, slice(0, n))
        ratio = R.judge_forward(net, rs, out[:n], arith)
        worst = max(worst, float(ratio.max()))
        assert ratio.max() <= 1, (n, int(ratio.argmax()), float(ratio.max()))
        if save:
            free = check_masks(name, arith, rs, bits)
    report("%s %s%s" % (FWD[arith], name, tag), worst, free)


@pytest.mark.parametrize("name", C.NAMES)
def test_forward_f32_every_row(name):
    _forward_sizes(name, "f32")


@pytest.mark.parametrize("tile,compact", [("64", "0")])
@pytest.mark.parametrize("name", C.NAMES_512)
def test_forward_f32_every_row_other_tiles(name, tile, compact, monkeypatch):
    """the exact-f32 grid forward with the full K chain instead of the per-tile K compaction"""
    monkeypatch.setenv("SDFR_FWD_COMPACT", compact)
    _forward_sizes(name, "f32", " tile=%s compact=%s" % (tile, compact))


@pytest.mark.parametrize("name", C.NAMES_512)
def test_forward_f16_every_row(name):
    _forward_sizes(name, "f16")


@pytest.mark.parametrize("name", C.NAMES_512)
def test_forward_split_every_row(name):
    _forward_sizes(name, "split")


# counts that select the 16-row tiles (below 4096 rows), the 64-row tiles and the 128-row tiles (half | 2: above 16384 rows)
COUNTED = [(0, 300, 17), (0, 300, 300), (0, 4300, 4200), (1, 300, 129), (1, 4300, 4200), (3, 300, 65), (3, 16600, 16500)]


@pytest.mark.parametrize("name", C.NAMES_512 + ("w200", "ln64"))
def test_forward_counted_every_row(name):
    net, h, L = C.net(name), handle(name), _lib.lib()
    x300 = C.rows(name)
    for half, n_max, n_dev in COUNTED:
        if half and name not in C.NAMES_512:
            continue
        arith = "f16" if half else "f32"
        r = ref(name, arith)
        src = np.arange(n_max) % C.N_ROWS
        x = T(x300[src])
        sdf = torch.full((n_max,), C.SENTINEL, device=DEV)
        cnt = T([n_dev], torch.int32)
        _lib.check(L.sdfr_mlp_forward_counted(h.h, _lib.ptr(x), n_max, _lib.ptr(cnt), _lib.ptr(sdf), half, _lib.stream_ptr()), "counted")
        torch.cuda.synchronize()
        out = N(sdf)
        assert (out[n_dev:] == C.SENTINEL).all(), "rows beyond *n_dev written"
        ratio = R.judge_forward(net, _sub(net, r, src[:n_dev]), out[:n_dev], arith)
        assert ratio.max() <= 1, (half, n_max, n_dev, int(ratio.argmax()), float(ratio.max()))
        report("sdfr_mlp_forward_counted half=%d n=%d %s" % (half, n_dev, name), float(ratio.max()))


@pytest.mark.parametrize("name", C.NAMES_512)
def test_forward_f16_counted_every_row_and_mask(name):
    net, h, L = C.net(name), handle(name), _lib.lib()
    r = ref(name, "f16")
    n_max, n_dev = 300, 129
    x = T(C.rows(name))
    sdf = torch.full((n_max,), C.SENTINEL, device=DEV)
    ws = torch.full((int(L.sdfr_decoder_mask_words(h.h, n_max)),), FILL, dtype=torch.int32, device=DEV)
    cnt = T([n_dev], torch.int32)
    _lib.check(L.sdfr_mlp_forward_f16_counted(h.h, _lib.ptr(x), n_max, _lib.ptr(cnt), _lib.ptr(sdf), _lib.ptr(ws), _lib.stream_ptr()), "f16_counted")
    torch.cuda.synchronize()
    out = N(sdf)
    assert (out[n_dev:] == C.SENTINEL).all()
    rs = _sub(net, r, slice(0, n_dev))
    ratio = R.judge_forward(net, rs, out[:n_dev], "f16")
    assert ratio.max() <= 1, (int(ratio.argmax()), float(ratio.max()))
    check_rows_beyond(ws, n_dev, 128, net.n_lin - 1, net.hp)
    free = check_masks(name, "f16", rs, R.mask_decode(N(ws), np.arange(n_dev), net.n_lin - 1, net.hp))
    report("sdfr_mlp_forward_f16_counted %s" % name, float(ratio.max()), free)


# ---- Jacobians --------------------------------------------------------------------------------------------------------------------

def _layouts():
    """name -> (B, rows_per_crop, cap, cnt, idx[B][cap]).  'batch': the layout of the issue; 'single': one crop (the 16-row half kernel);
    'crops8' / 'crops12': the 32-row float32 kernel and the pools over the crops' live tiles."""
    out = {"batch": (C.JAC_B, C.JAC_ROWS, C.JAC_CAP, np.array(C.JAC_CNT, np.int32), C.jac_layout())}
    rng = np.random.default_rng(3)
    out["single"] = (1, 300, 64, np.array([50], np.int32), np.concatenate([[299], rng.permutation(299)[:49], np.zeros(14)]).astype(np.int32)[None])
    for B in (8, 12):
        rpc, cap = 300 // B, 20
        cnt = rng.integers(0, cap + 1, B).astype(np.int32)
        cnt[0], cnt[1], cnt[2] = 0, 1, cap
        idx = np.zeros((B, cap), np.int32)
        for b in range(B):
            idx[b, :cnt[b]] = rng.permutation(rpc)[:cnt[b]]
        out["crops%d" % B] = (B, rpc, cap, cnt, idx)
    return out


LAYOUTS = _layouts()


def jacobian(name, layout, x, sdf_full, ws, mode):
    """J [B][cap][ni], sdf_sel [B][cap] (sentinel filled), the absolute rows of the live slots and their (b, s)"""
    net, h, L = C.net(name), handle(name), _lib.lib()
    B, rpc, cap, cnt, idx = LAYOUTS[layout]
    J = torch.full((B, cap, net.n_inputs), C.SENTINEL, device=DEV)
    sel = torch.full((B, cap), C.SENTINEL, device=DEV)
    d_idx, d_cnt = T(idx, torch.int32), T(cnt, torch.int32)
    _lib.check(L.sdfr_mlp_jacobian(h.h, _lib.ptr(x), rpc, B, _lib.ptr(d_idx), cap, _lib.ptr(d_cnt), _lib.ptr(J), _lib.ptr(sel),
                                   _lib.ptr(sdf_full), _lib.ptr(ws), mode, _lib.stream_ptr()), "sdfr_mlp_jacobian")
    torch.cuda.synchronize()
    J, sel = N(J), N(sel)
    live = np.arange(cap)[None, :] < cnt[:, None]
    assert (J[~live] == C.SENTINEL).all() and (sel[~live] == C.SENTINEL).all(), "slots beyond cnt[b] written"
    bs = np.argwhere(live)
    rows = bs[:, 0] * rpc + idx[bs[:, 0], bs[:, 1]]
    return J[live], sel[live], rows


MASK_FED = [("f32", 0, "f32"), ("split", 0, "f32"), ("f16", 1, "f32"), ("f16", 2, "f16"), ("f16", 2 | MANY, "f16")]


MASK_FED_CASES = [(n, *m) for n in ("asset", "w260", "w260_9", "dead") for m in MASK_FED] + [(n, *MASK_FED[0]) for n in ("w200", "w48", "w128")]


@pytest.mark.parametrize("name,fwd_arith,mode,bwd", MASK_FED_CASES)
def test_mask_fed_jacobian_every_entry(name, fwd_arith, mode, bwd):
    net = C.net(name)
    x = T(C.rows(name))
    sdf, bits, ws = forward(name, fwd_arith, x, C.N_ROWS, True)
    for layout in LAYOUTS:
        J, sel, rows = jacobian(name, layout, x, sdf, ws, mode)
        assert np.array_equal(sel, N(sdf)[rows]), "sdf_sel is not the forward's value"
        masks = [bits[rows, l, :od] for l, od in enumerate(net.out_dims)]
        ratio = R.judge_jac_masks(net, C.rows(name)[rows], masks, J, fwd_arith, bwd)
        assert ratio.max() <= 1, (layout, np.unravel_index(ratio.argmax(), ratio.shape), float(ratio.max()))
        report("jacobian masks=%s mode=%d %s %s" % (fwd_arith, mode, layout, name), float(ratio.max()))


@pytest.mark.parametrize("name", ("asset", "w260", "w260_9", "xyz_tanh", "dead", "w200", "w48", "w128", "ln64", "ln200", "ln512"))
def test_recomputing_jacobian_every_row(name):
    net = C.net(name)
    x = T(C.rows(name))
    modes = [0] + ([MANY] if net.hp == 512 and not net.has_ln else [])
    sdf = ws = None
    if net.use_tanh:                                    # masks supplied, but a use_tanh decoder needs the pre-tanh value: it recomputes
        sdf, _, ws = forward(name, "f32", x, C.N_ROWS, True)
    for mode in modes:
        for layout in LAYOUTS:
            J, sel, rows = jacobian(name, layout, x, sdf, ws, mode)
            xs = C.rows(name)[rows]
            r0 = R.evaluate(net, xs, "f32")
            rf = R.judge_forward(net, r0, sel, "f32")
            assert rf.max() <= 1, ("sdf_sel", mode, layout, float(rf.max()))
            ratio, left = R.judge_jac_recompute(net, xs, r0, J, "f32")
            assert np.isfinite(J).all() and np.isfinite(sel).all()
            assert left.mean() <= 0.02, left.mean()
            kept = np.where(left, 0.0, ratio)
            assert kept.max() <= 1, (mode, layout, int(kept.argmax()), float(kept.max()))
            free = float(np.mean(np.concatenate([f.ravel() for f in R.free_units(net, r0, "f32")])))
            report("jacobian recompute mode=%d %s %s" % (mode, layout, name), float(kept.max()), free, float(left.mean()))
