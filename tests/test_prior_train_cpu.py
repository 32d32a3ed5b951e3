"""The float64 restatement of the decoder's training kernels (tests/_prior_train_ref.py) against torch float64 autograd and golden G23,
the dropout hash and the workspace layout against csrc/train_cells.h compiled for the host, the exported symbols, PriorTrainer's files,
and the calibration of the GPU tests' constants on the float32 emulation.  No GPU.
"""
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from sdflabel_amd import _lib
from tests import _decoder_ref as DR
from tests import _prior_train_cases as PC
from tests import _prior_train_ref as PR
from tests._util import build_host_program, gold

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G23_INJ = [(0, 0), (0, 0), (6, 0), (0, 0), (0, 0)]


# ---- plain torch ops, float64, under autograd --------------------------------------------------------------------------------------

def torch_run(vs, gs, bs, inj, use_tanh, x, target, keep=None, scale=None):
    """loss and the gradients of v, g (or the plain weights where g is None), b and x"""
    t = lambda a: torch.tensor(np.asarray(a, np.float64), requires_grad=True)  # noqa: E731
    V, G, B, X = [t(v) for v in vs], [None if g is None else t(g) for g in gs], [t(b) for b in bs], t(x)
    cur = X
    nh = len(V) - 1
    for l in range(nh + 1):
        W = V[l] if G[l] is None else V[l] * (G[l] / V[l].norm(2, dim=1, keepdim=True))
        if inj[l][0]:
            cur = torch.cat([cur, X[:, inj[l][1]:inj[l][1] + inj[l][0]]], 1)
        cur = cur @ W.t() + B[l]
        if l < nh:
            cur = torch.relu(cur)
            if keep is not None:
                cur = cur * torch.tensor(np.asarray(keep[l], np.float64) * scale[l])
    y = cur[:, 0]
    if use_tanh:
        y = torch.tanh(y)
    out = torch.tanh(y)
    tg = torch.tensor(np.asarray(target, np.float64))
    loss = (out.clamp(-0.1, 0.1) - tg.clamp(-0.1, 0.1)).abs().mean()
    loss.backward()
    return (float(loss), out.detach().numpy(), [v.grad.numpy() for v in V], [None if g is None else g.grad.numpy() for g in G],
            [b.grad.numpy() for b in B], X.grad.numpy())


def _close(a, b, tol=1e-12):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape
    assert np.abs(a - b).max() <= tol * max(1.0, np.abs(b).max()), float(np.abs(a - b).max())


def _small_target(net, x):
    """targets near the prediction so that most rows sit inside the clamp"""
    r = PR.forward(net, x)
    rng = np.random.default_rng(5)
    return 0.05 * np.tanh(r.out) + 0.02 * rng.standard_normal(len(x))


@pytest.mark.parametrize("name", ["w128", "xyz", "tanh", "lat8"])
def test_restatement_equals_torch_float64_autograd(name):
    net = PC.net(name)
    x, _ = PC.rows(name, 65)
    scale_out = 0.02                                                       # inside the clamp: |tanh(0.02 y)| stays small
    net = PR.Net64([(W, b) for W, b in zip(net.W[:-1], net.b[:-1])] + [(net.W[-1] * scale_out, net.b[-1] * scale_out)], net.inj, net.use_tanh)
    target = _small_target(net, x)
    loss, out, gv, _, gb, gx = torch_run(net.W, [None] * net.n_lin, net.b, net.inj, net.use_tanh, x, target)
    r = PR.forward(net, x)
    l_ref, g_sdf = PR.clamped_l1(r.out, target)
    assert np.count_nonzero(g_sdf) > 0.5 * len(x)
    b = PR.backward(net, r, g_sdf, want_masses=False)
    assert abs(loss - l_ref) <= 1e-12
    _close(r.out, out)
    _close(b.g_inputs, gx)
    for l in range(net.n_lin):
        _close(b.dW[l], gv[l])
        _close(b.db[l], gb[l])


def _g23():
    z = gold("g23_prior_train.npz")
    S, K = int(z["S"]), int(z["K"])
    vs = [z["state.lin%d.weight_v" % l].astype(np.float64) for l in range(5)]
    gs = [z["state.lin%d.weight_g" % l].astype(np.float64) for l in range(5)]
    bs = [z["state.lin%d.bias" % l].astype(np.float64) for l in range(5)]
    x = np.concatenate([np.repeat(z["latents"], K, 0), z["xyz"]], 1)
    return z, S, K, vs, gs, bs, x


def test_restatement_equals_golden_g23_of_the_reference_decoder():
    z, S, K, vs, gs, bs, x = _g23()
    net = PR.Net64([(PR.fold(v, g), b) for v, g, b in zip(vs, gs, bs)], G23_INJ)
    r = PR.forward(net, x)
    loss, g_sdf = PR.clamped_l1(r.out, z["target"])
    b = PR.backward(net, r, g_sdf, want_masses=False)
    _close(r.out, z["sdf"])
    assert abs(loss - float(z["loss"])) <= 1e-12
    _close(b.g_inputs, z["g_inputs"])
    _close(b.g_inputs[:, :3].reshape(S, K, 3).sum(1), z["g_latents"])
    for l in range(5):
        dv, dg = PR.fold_backward(vs[l], gs[l], b.dW[l])
        _close(dv, z["grad.lin%d.weight_v" % l])
        _close(dg, z["grad.lin%d.weight_g" % l])
        _close(b.db[l], z["grad.lin%d.bias" % l])
    # the golden holds data only: arrays of numbers
    assert all(z[k].dtype.kind in "fi" for k in z.files)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "g23_prior_train.npz")) < 1 << 20


def test_restatement_with_a_keep_mask_equals_torch_with_the_mask_multiplied():
    z, S, K, vs, gs, bs, x = _g23()
    net = PR.Net64([(PR.fold(v, g), b) for v, g, b in zip(vs, gs, bs)], G23_INJ)
    keep = [PR.keep_mask(77, l, len(x), net.out_dims[l], 0.2) for l in range(4)]
    scale = PR.scales(net, 0.2, 0b1111)
    loss, out, gv, gg, gb, gx = torch_run(vs, gs, bs, G23_INJ, False, x, z["target"], keep, scale)
    r = PR.forward(net, x, keep, scale)
    l_ref, g_sdf = PR.clamped_l1(r.out, z["target"])
    b = PR.backward(net, r, g_sdf, want_masses=False)
    assert abs(loss - l_ref) <= 1e-12
    _close(r.out, out)
    _close(b.g_inputs, gx)
    for l in range(5):
        dv, dg = PR.fold_backward(vs[l], gs[l], b.dW[l])
        _close(dv, gv[l])
        _close(dg, gg[l])
        _close(b.db[l], gb[l])


def test_forward_mass_is_the_decoder_tests_m_fwd_without_dropout():
    net = PC.net("w128")
    x, g = PC.rows("w128", 65)
    r = PR.forward(net, x)
    b = PR.backward(net, r, g)
    _close(b.M_fwd, DR.evaluate(net, x).M_fwd, 1e-12)


# ---- the dropout hash --------------------------------------------------------------------------------------------------------------

def test_hash_is_a_function_of_seed_layer_row_feature_only():
    a = PR.drop_word(9, 3, np.arange(100, 164), np.arange(50))
    b = PR.drop_word(9, 3, np.arange(120, 140), np.arange(10, 30))          # another block that overlaps: same units, same words
    assert np.array_equal(a[20:40, 10:30], b)
    assert (a < (1 << 24)).all()
    for other in (PR.drop_word(10, 3, np.arange(100, 164), np.arange(50)), PR.drop_word(9, 2, np.arange(100, 164), np.arange(50)),
                  PR.drop_word(9, 3, np.arange(101, 165), np.arange(50))):
        assert np.mean(a == other) < 0.01
    assert np.array_equal(PR.keep_mask(9, 3, 64, 50, 0.2, row0=100), a >= PR.drop_threshold(0.2))


@pytest.mark.parametrize("p", [0.2, 0.5, 0.03])
def test_kept_share_is_within_five_sigma(p):
    k = PR.keep_mask(PC.SEED, 1, 2048, 512, p)                               # 2^20 units
    n = k.size
    assert n == 1 << 20
    q = 1.0 - PR.drop_threshold(p) / 2.0 ** 24
    assert abs(k.mean() - q) <= 5.0 * np.sqrt(q * (1 - q) / n)
    assert abs(q - (1 - p)) < 2.0 ** -24


def test_p_zero_keeps_all_and_takes_no_hash(monkeypatch):
    monkeypatch.setattr(PR, "drop_word", lambda *a: (_ for _ in ()).throw(AssertionError("hash taken")))
    assert PR.keep_mask(1, 0, 10, 10, 0.0).all()
    assert PR.scales(PC.net("w128"), 0.0, 7) == [1.0, 1.0, 1.0]


# ---- train_cells.h on the host ----------------------------------------------------------------------------------------------------

def _host_checks(exe):
    thr = PR.drop_threshold(0.2)
    for seed, layer, row0, rows, width in ((PC.SEED, 0, 0, 40, 33), (2 ** 63 + 12345, 7, 2 ** 31 - 20, 24, 512), (0, 15, 1023, 3, 1000)):
        r = subprocess.run([exe, "hash", str(seed), str(layer), str(row0), str(rows), str(width), str(thr)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        got = np.array(r.stdout.split(), np.int64).reshape(rows, width, 2)
        want = PR.drop_word(seed, layer, np.arange(row0, row0 + rows), np.arange(width))
        assert np.array_equal(got[:, :, 0], want)
        assert np.array_equal(got[:, :, 1].astype(bool), want >= thr)
    for name, n in (("w128", 1), ("w128", 2 * PR.CHUNK + 76), ("asset", 1024), ("xyz", 1025)):
        net = PC.net(name)
        L = PR.layout(net, n)
        args = [str(n), str(net.n_lin)] + [str(v) for v in L.in_dim + L.out_dim + [i[0] for i in net.inj]]
        r = subprocess.run([exe, "layout"] + args, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        want = [L.chunks, L.x0] + L.act + [L.tail, L.delta[0], L.delta[1]] + L.ginj[1:] + [L.part, L.total]
        assert [int(v) for v in r.stdout.split()] == want


def test_train_cells_on_the_host_equal_the_numpy_restatement(tmp_path):
    _host_checks(build_host_program(tmp_path, "prior_train_host/prior_train_host.cpp", "prior_train_host"))


def test_train_cells_host_program_under_sanitizers(tmp_path):
    _host_checks(build_host_program(tmp_path, "prior_train_host/prior_train_host.cpp", "prior_train_host_san",
                                    ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]))


def test_chunk_sum_order_of_the_emulation():
    """_seq_rows sums rows in order inside chunks and the chunk sums in chunk order: values that show the order"""
    n = 2 * PR.CHUNK + 76
    d = np.ones((n, 1), np.float32)
    d[0, 0] = 2.0 ** 24                                                     # 1 is lost against 2^24 inside chunk 0, kept in chunks 1 and 2
    dw, db = PR._seq_rows(d, np.ones((n, 1), np.float32))
    want = np.float32(2.0 ** 24) + np.float32(PR.CHUNK) + np.float32(76)
    assert dw[0, 0] == want and db[0] == want and want != np.float32(2.0 ** 24 + n - 1)


# ---- exports ------------------------------------------------------------------------------------------------------------------------

def test_exports_and_abi_version():
    header = open(os.path.join(ROOT, "include", "sdfr.h")).read()
    assert _lib.ABI_VERSION >= 417 and int(re.search(r"#define SDFR_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION
    body = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(sdfr_[a-z0-9_]+)\s*\(", body))
    assert declared == set(_lib.EXPORTS)
    h = _lib.lib()
    for name in ("sdfr_decoder_train_bytes", "sdfr_decoder_train_forward", "sdfr_decoder_train_backward"):
        assert name in _lib.EXPORTS and hasattr(h, name) and re.search(r"\bint(64_t)? %s\(" % name, body), name


def test_argument_checks_need_no_gpu():
    import ctypes
    from sdflabel_amd.deepsdf.train import TrainDesc
    h = _lib.lib()
    d = TrainDesc.from_decoder(PC.decoders()["w128"])
    net = PC.net("w128")
    for n in (1, 1024, 2124):
        assert d.bytes(n) == 4 * PR.layout(net, n).total
        assert d.act_offset(1, n) == PR.layout(net, n).act[1]
    bad = TrainDesc([6, 64], [64, 2], [(0, 0), (0, 0)], 6)
    assert h.sdfr_decoder_train_bytes(*bad.args(), 10) == -1 and b"out_dim 1" in h.sdfr_last_error()
    wide = TrainDesc([6, 600], [600, 1], [(0, 0), (0, 0)], 6)
    assert h.sdfr_decoder_train_bytes(*wide.args(), 10) == -1
    W = (ctypes.c_void_p * 4)(1, 1, 1, 1)
    # a workspace that is too small is an error before any launch
    assert h.sdfr_decoder_train_forward(*d.args(), 0, W, W, 1, 10, 0.0, 0, 0, 1, 1, d.bytes(10) - 4, None) == -1
    assert b"workspace" in h.sdfr_last_error()
    assert h.sdfr_decoder_train_backward(*d.args(), 0, W, 1, 10, 1, d.bytes(10) - 4, W, W, 1, None) == -1
    assert b"workspace" in h.sdfr_last_error()
    assert h.sdfr_decoder_train_forward(*d.args(), 0, W, W, 1, 10, 1.0, 0, 0, 1, 1, d.bytes(10), None) == -1
    assert b"drop_p" in h.sdfr_last_error()


def test_layer_norm_decoders_are_refused():
    from sdflabel_amd.deepsdf.networks.deep_sdf_decoder_scale import Decoder
    from sdflabel_amd.deepsdf.train import TrainDesc
    ln = Decoder(3, [64] * 3, norm_layers=[0, 1, 2], latent_in=[2], weight_norm=False)
    with pytest.raises(_lib.SdfrError, match="LayerNorm"):
        TrainDesc.from_decoder(ln)


# ---- save / load --------------------------------------------------------------------------------------------------------------------

def test_prior_trainer_files_load_strictly_through_setup_dsdf(tmp_path):
    from sdflabel_amd.deepsdf.workspace import setup_dsdf
    from sdflabel_amd.pipelines.train_prior import PriorTrainer, default_specs
    specs = default_specs(3, (128,) * 3, (2,))
    tr = PriorTrainer(specs, 5, "cpu", seed=3)
    assert tr.decoder.training and tr.desc.drop_layers == 0b111 and tr.drop_p == 0.2
    before = {k: v.clone() for k, v in tr.decoder.scale_net.state_dict().items()}
    path = tr.save(str(tmp_path / "prior"))
    assert sorted(os.listdir(tmp_path)) == ["prior.json", "prior.pt", "prior_latents.pt"]
    assert json.load(open(tmp_path / "prior.json")) == specs
    saved = torch.load(path)
    assert set(saved) == {"epoch", "model_state_dict"} and all(k.startswith("module.") for k in saved["model_state_dict"])
    dec, L = setup_dsdf(path, precision=torch.float32)                       # load_state_dict is strict there
    assert L == 3 and not dec.training
    for (W0, b0), (W1, b1) in zip(tr.decoder.effective_layers(), dec.effective_layers()):
        assert np.array_equal(W0, W1) and np.array_equal(b0, b1)
    assert all(torch.equal(v, dec.scale_net.state_dict()[k]) for k, v in before.items())
    lat = torch.load(str(tmp_path / "prior_latents.pt"))
    assert lat["latents"].shape == (5, 3) and torch.allclose(lat["latents"].norm(dim=1), torch.ones(5), atol=1e-6) and lat["unit_latents"]
    assert torch.equal(lat["raw_latents"], tr.latents.detach())
    # Decoder.forward keeps refusing train() mode with dropout
    with pytest.raises(_lib.SdfrError):
        tr.decoder(torch.zeros(2, 6))


def test_segmented_sum_is_the_latent_expansions_backward():
    from sdflabel_amd.deepsdf.train import expand_latents
    z = torch.randn(3, 4, dtype=torch.float64, requires_grad=True)
    w = torch.randn(15, 4, dtype=torch.float64)
    (expand_latents(z, 5) * w).sum().backward()
    assert torch.allclose(z.grad, w.view(3, 5, 4).sum(1), atol=0, rtol=1e-15)


# ---- calibration of the GPU tests' constants on the float32 emulation ---------------------------------------------------------------

@pytest.fixture(scope="module")
def emulation_ratios():
    """per case: the judges' ratios of the emulation at the full tolerance, and raw = error / (u mass) with the constants divided out"""
    out = {}
    for name, n, p in PC.cases():
        net = PC.net(name)
        x, g = PC.rows(name, n)
        dl = PC.drop_layers(name)
        keep, scale = PR.keep_masks(net, PC.SEED, n, p, dl), PR.scales(net, p, dl)
        e = PR.emulate(net, x, g, keep if p > 0 else None, scale)
        j, r, _ = PR.judge(net, x, g, keep, scale, e.sdf, e.y1, e.a, e.g_inputs, e.dW, e.db)
        b0 = PR.backward(net, r, g)
        j["raw"] = {"c_fwd": float((np.abs(e.y.astype(np.float64) - r.y) / (PR.U32 * b0.M_fwd)).max()), "c_dx": j["dx"] * PR.C["c_dx"],
                    "c_dw": max(j["dw"], j["db"]) * PR.C["c_dw"], "c_z": j["cz"]}
        out[(name, n, p)] = j
    return out


def test_emulation_passes_every_judge_at_a_quarter_of_the_tolerance(emulation_ratios):
    for case, j in emulation_ratios.items():
        assert 4 * j["fwd"] <= 1 and 4 * j["dx"] <= 1 and 4 * j["dw"] <= 1 and 4 * j["db"] <= 1, (case, j)
        assert 4 * j["cz"] <= PR.C["c_z"], (case, j)
        assert j["bad_units"] == 0 and j["wrong_drop"] == 0, (case, j)
        assert j["free_share"] <= PR.FREE_CAP, (case, j)             # the cap is a condition on the inputs: the emulation alone stays under it


def test_constants_are_four_times_the_emulations_worst_ratio(emulation_ratios):
    """each constant is 4 x the largest error / (u mass) of the emulation over the cases, rounded up in the third digit: not looser"""
    worst = {k: max(j["raw"][k] for j in emulation_ratios.values()) for k in ("c_fwd", "c_dx", "c_dw", "c_z")}
    print("largest error / (u mass) of the float32 emulation:", worst)
    for k, w in worst.items():
        assert 4 * w <= PR.C[k] <= 4 * w * 1.01, (k, w, PR.C[k])
