"""The decoder reference of tests/_decoder_ref.py without a GPU: it equals float64 autograd on a plain-torch restatement and the G2 golden,
the mask layout round-trips, the constants C_BOUND are 4 x what the CPU emulations of the working precisions reach (never calibrated on a
kernel), the caps of the GPU tests hold for the emulations, and the judges catch two planted defects (a dropped K tile, a neighbour's
mask word).  tests/test_gpu_decoder_ref.py holds the kernels to the same reference with the same judges."""
import functools

import numpy as np
import pytest
import torch

from tests import _decoder_cases as C
from tests import _decoder_ref as R
from tests._util import gold

CLASSES = [(n, "f32", None) for n in C.NAMES] + [(n, a, b) for n in C.NAMES_512 for a, b in (("split", None), ("f16", None), ("f16", "f32"))]


@functools.lru_cache(maxsize=None)
def ratios(name, arith, bwd):
    return R.emulation_ratios(C.net(name), C.rows(name), arith, bwd)


def _torch_forward(net, x):
    """Decoder.forward restated with torch ops, float64"""
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    cur = x
    for l in range(net.n_lin):
        n_inj, off = net.inj[l]
        if n_inj:
            cur = torch.cat([cur, x[:, off:off + n_inj]], 1)
        cur = torch.nn.functional.linear(cur, t(net.W[l]), t(net.b[l]))
        if l < net.n_lin - 1:
            if net.ln[l] is not None:
                cur = torch.nn.functional.layer_norm(cur, (cur.shape[1],), t(net.ln[l][0]), t(net.ln[l][1]), 1e-5)
            cur = torch.relu(cur)
        elif net.use_tanh:
            cur = torch.tanh(cur)
    return torch.tanh(cur)[:, 0]


@pytest.mark.parametrize("name", C.NAMES)
def test_reference_equals_float64_autograd(name):
    net = C.net(name)
    x = torch.from_numpy(C.rows(name).astype(np.float64)).requires_grad_(True)
    out = _torch_forward(net, x)
    out.sum().backward()                       # rows are independent: the gradient of the sum is every row's Jacobian
    r = R.evaluate(net, C.rows(name))
    assert np.abs(r.out - out.detach().numpy()).max() <= 1e-12
    J = x.grad.numpy()
    assert np.abs(r.J - J).max() <= 1e-12 * max(1.0, np.abs(J).max())
    # the forward-mode blocks A_l (the Jacobian's masses are built from them) give the same Jacobian as the reverse sweep
    w, od = net.W[-1][0].astype(np.float64), net.out_dims[-1]
    Jy = np.einsum("u,nuj->nj", w[:od], r.A[-1])
    n_inj, off = net.inj[-1]
    Jy[:, off:off + n_inj] += w[od:od + n_inj]
    assert np.abs(Jy - r.Jy).max() <= 1e-12 * max(1.0, np.abs(r.Jy).max())


def test_reference_reproduces_golden_g2_within_its_float32_error():
    z = gold("g2_decoder.npz")
    r = R.evaluate(C.net("asset"), z["fit_inputs"], want_masses=False)
    assert np.abs(r.out - z["fit_sdf"][:, 0]).max() < 2e-6
    assert np.abs(r.J - z["fit_grad_inputs"]).max() < 2e-5


@pytest.mark.parametrize("tag,kw", [
    ("ln", dict(latent_size=3, dims=[64] * 8, dropout=list(range(8)), dropout_prob=0.2, norm_layers=list(range(8)), latent_in=[4], weight_norm=False)),
    ("wn", dict(latent_size=3, dims=[64] * 8, dropout=list(range(8)), dropout_prob=0.2, norm_layers=list(range(8)), latent_in=[4], weight_norm=True)),
    ("x", dict(latent_size=5, dims=[48] * 5, dropout=None, norm_layers=(), latent_in=[2, 4], weight_norm=False, xyz_in_all=True, use_tanh=True)),
])
def test_reference_reproduces_golden_g2_small_specs(tag, kw):
    """LayerNorm, weight norm, xyz_in_all + use_tanh with two re-injections: the recorded float32 values of the original module"""
    from sdflabel_amd.deepsdf.networks.deep_sdf_decoder_scale import Decoder
    from tests._util import state_from_npz
    z = gold("g2_decoder.npz")
    d = Decoder(**kw)
    d.load_state_dict({k: torch.from_numpy(v) for k, v in state_from_npz(z, tag + "_state_").items()})
    r = R.evaluate(R.Net.from_decoder(d.eval()), z[tag + "_inputs"], want_masses=False)
    assert np.abs(r.out - z[tag + "_sdf"][:, 0]).max() < 2e-6
    g_out = z[tag + "_gout"] if (tag + "_gout") in z.files else np.ones_like(z[tag + "_sdf"])
    ref = z[tag + "_grad_inputs"]
    assert np.abs(r.J * g_out - ref).max() < 2e-5 * max(1.0, np.abs(ref).max())


def test_half_reference_holds_the_half_image():
    net = C.net("w260")
    Wh = net.weights("f16")
    assert all(np.array_equal(w, w.astype(np.float16).astype(np.float64)) for w in Wh[:-1])
    assert np.array_equal(Wh[-1], net.W[-1].astype(np.float64))          # w_last stays float32
    assert not np.array_equal(Wh[0], net.weights("f32")[0])


@pytest.mark.parametrize("hp,nl,n", [(512, 8, 300), (256, 4, 129), (128, 3, 1)])
def test_mask_layout_round_trip(hp, nl, n):
    rng = np.random.default_rng(hp + n)
    bits = rng.random((n, nl, hp)) < 0.5
    ws = R.mask_encode(bits)
    assert ws.size == R.mask_words(n, nl, hp)
    assert np.array_equal(R.mask_decode(ws, np.arange(n), nl, hp), bits)
    # the layout comment of mlp_kernel.h, element by element (sdfr_mask_dword, sdfr_mask_shift)
    for r, l, j in [(0, 0, 0), (n - 1, nl - 1, hp - 1), (n // 2, nl // 2, 37), (n - 1, 0, 4), (n // 3, nl - 1, 27)]:
        dword = (((r >> 7) * nl + l) * 128 + (r & 127)) * (hp // 32) + (j >> 5)
        shift = ((j >> 2) & 1) * 16 + ((j & 31) >> 3) * 4 + (j & 3)
        assert bool((int(ws[dword]) >> shift) & 1) == bool(bits[r, l, j])
    assert sorted(R.mask_shift(np.arange(32)).tolist()) == list(range(32))
    # rows are independent: decoding a subset in another order reads the same bits
    sel = rng.permutation(n)[:max(1, n // 2)]
    assert np.array_equal(R.mask_decode(ws, sel, nl, hp), bits[sel])


@pytest.mark.parametrize("name,arith,bwd", CLASSES)
def test_constants_are_four_times_the_emulation(name, arith, bwd):
    """emulation <= C_BOUND / 4, per arithmetic class"""
    rat = ratios(name, arith, bwd)[0]
    cls = "ln" if C.net(name).has_ln else arith
    assert rat["fwd"] <= R.C_BOUND[cls + "_fwd"] / 4, rat
    assert rat["cz"] <= R.C_BOUND[cls + "_cz"] / 4, rat
    jcls = "ln" if C.net(name).has_ln else (bwd or ("f16" if arith == "f16" else "f32"))
    assert rat["jac"] <= R.C_BOUND[jcls + "_jac"] / 4, rat
    assert 4 * rat["tanh"] + 4 <= R.C_BOUND["c_t"], rat          # + 2 ulp = 4 u for the device's tanhf


def test_constants_are_not_looser_than_the_rule():
    """each constant is 4 x the LARGEST ratio of its class (rounded up by at most 5 %)"""
    worst = {}
    for name, arith, bwd in CLASSES:
        rat = ratios(name, arith, bwd)[0]
        cls = "ln" if C.net(name).has_ln else arith
        jcls = "ln" if C.net(name).has_ln else (bwd or ("f16" if arith == "f16" else "f32"))
        for key, v in ((cls + "_fwd", rat["fwd"]), (cls + "_cz", rat["cz"]), (jcls + "_jac", rat["jac"]), ("c_t", rat["tanh"] + 1.0)):
            worst[key] = max(worst.get(key, 0.0), v)
    for key, v in worst.items():
        assert 4 * v <= R.C_BOUND[key] <= 4 * v * 1.05 + 0.05, (key, v, R.C_BOUND[key])


@pytest.mark.parametrize("name,arith,bwd", CLASSES)
def test_caps_and_judges_hold_for_the_emulation(name, arith, bwd):
    """what the GPU tests assert of a kernel, asserted of the emulation at a quarter of the bounds: the inputs stay within the caps by
    the reference alone"""
    net, x = C.net(name), C.rows(name)
    rat, e, r0, rm = ratios(name, arith, bwd)
    assert R.judge_forward(net, r0, e.out, arith, 0.25).max() <= 1
    hp = net.hp
    bits = np.zeros((x.shape[0], net.n_lin - 1, hp), bool)
    for l, m in enumerate(e.mask):
        bits[:, l, :m.shape[1]] = m
    bad, free = R.judge_masks(net, r0, bits, arith)
    assert bad == 0
    assert free <= (0.05 if arith == "f16" else 1e-3), free
    jb = bwd or ("f16" if arith == "f16" else "f32")
    assert R.judge_jac_masks(net, x, e.mask, e.J, arith, jb, 0.25).max() <= 1
    if arith == "f32":
        ratio, left = R.judge_jac_recompute(net, x, r0, e.J, "f32", 0.25)
        assert left.mean() <= 0.02, left.mean()
        assert ratio[~left].max() <= 1


@pytest.mark.parametrize("name", ["asset", "ln64"])
def test_a_non_finite_output_fails_every_judge(name):
    """a NaN or inf a kernel wrote is an error of infinite size, in a kept row of the recomputing judge too"""
    net, x = C.net(name), C.rows(name)
    r0 = ratios(name, "f32", None)[2]
    for bad in (np.nan, np.inf):
        J = r0.J.copy()
        J[7, 1] = bad
        ratio, left = R.judge_jac_recompute(net, x, r0, J, "f32")
        assert not left[7] and ratio[7] == np.inf and ratio[~left].max() == np.inf
        assert R.judge_jac_masks(net, x, r0.mask, J, "f32", "f32").max() == np.inf
        out = r0.out.copy()
        out[7] = bad
        assert R.judge_forward(net, r0, out, "f32").max() == np.inf


def test_the_last_row_saturates_tanh():
    """|y| > 9 on every reference the kernels are held to (LayerNorm decoders cannot be driven there): float32 tanh is 1, d out / d y is 0"""
    for name in C.NAMES:
        if C.net(name).has_ln:
            continue
        for arith in ("f32",) + (("f16",) if name in C.NAMES_512 else ()):
            assert abs(ratios(name, arith, None)[2].y[-1]) > 9, (name, arith)


# ---- planted defects: each must trip a judge -------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,arith", [("asset", "f32"), ("asset", "f16"), ("w260", "f32")])
def test_a_dropped_k_tile_of_one_row_is_caught(name, arith):
    net, x = C.net(name), C.rows(name)
    r0 = ratios(name, arith, None)[2]
    row, layer = 5, 2
    k0 = int(np.argmax(np.abs(r0.a[layer - 1][row]))) // 16 * 16           # a K tile that carries signal in that row
    e = R.emulate(net, x, arith, drop=(layer, row, k0))
    ratio = R.judge_forward(net, r0, e.out, arith)
    assert ratio[row] > 1 and np.delete(ratio, row).max() <= 1
    jb = "f16" if arith == "f16" else "f32"
    rj = R.judge_jac_masks(net, x, e.mask, e.J, arith, jb)
    # the masks of the defective run differ from the reference's in certain units of that row ...
    bits = np.zeros((x.shape[0], net.n_lin - 1, net.hp), bool)
    for l, m in enumerate(e.mask):
        bits[:, l, :m.shape[1]] = m
    assert R.judge_masks(net, r0, bits, arith)[0] > 0
    # ... while its Jacobian is the right one FOR those masks: only the value and the masks give the defect away
    assert np.delete(rj, row, 0).max() <= 1


@pytest.mark.parametrize("name,arith,bwd", [("asset", "f32", "f32"), ("asset", "f16", "f16"), ("w200", "f32", "f32")])
def test_a_neighbour_rows_mask_word_is_caught(name, arith, bwd):
    """the backward reads one mask dword of row r ^ 1: the Jacobian no longer belongs to the masks the forward saved"""
    net, x = C.net(name), C.rows(name)
    e = ratios(name, arith, None)[1]
    row, layer, word = 40, 1, 2
    wrong = [m.copy() for m in e.mask]
    wrong[layer][row, 32 * word:32 * word + 32] = e.mask[layer][row ^ 1, 32 * word:32 * word + 32]
    assert (wrong[layer][row] != e.mask[layer][row]).any()
    bad = R.emulate(net, x, arith, bwd, masks=e.mask, bwd_masks=wrong)
    ratio = R.judge_jac_masks(net, x, e.mask, bad.J, arith, bwd).max(1)
    assert ratio[row] > 1 and np.delete(ratio, row).max() <= 1
