"""The shape encoder without a GPU: the numpy restatement (tests/_encode_ref.py) against torch float64 autograd + torch.optim.Adam, the row hash,
csrc/encode_cells.h compiled into a host program (tests/encode_host/encode_host.cpp) against the restatement bit for bit -- also under
ASan/UBSan with exact-size buffers and broken tables --, exports / header / binding, argument checks, encode_folder's files and the calibration of
the trajectory bound of tests/test_gpu_encode.py on the float32 emulation.
"""
import copy
import os
import re
import struct
import subprocess

import numpy as np
import pytest
import torch

from sdflabel_amd import _lib
from sdflabel_amd import encode as E
from sdflabel_amd.sdf_samples import SdfSamples
from tests import _decoder_ref as DR
from tests import _encode_cases as EC
from tests import _encode_ref as ER
from tests import _encode_traj as ET
from tests import _prior_train_cases as PC
from tests._prior_train_loop import plain_forward
from tests._util import build_host_program

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement's loop against torch ------------------------------------------------------------------------------------------------

def _torch_fit(dec, samples, soff, z0, iters, k, lr, lr_step, lr_factor, clamp, code_reg, unit):
    """float64 autograd + torch.optim.Adam on the first k rows of every shape; the loss is the SUM over shapes of each shape's mean, so a shape's
    gradient is its own"""
    dec = copy.deepcopy(dec).double()
    for p in dec.parameters():
        p.requires_grad_(False)
    z = torch.tensor(np.asarray(z0, np.float64), requires_grad=True)
    opt = torch.optim.Adam([z], lr=lr)
    B = z.shape[0]
    rows = torch.tensor(np.stack([np.asarray(samples, np.float64)[int(soff[b]):int(soff[b]) + k] for b in range(B)]))      # [B][k][4]
    losses = []
    for it in range(iters):
        opt.param_groups[0]["lr"] = lr * lr_factor ** (it // lr_step)
        zn = z / z.norm(dim=1, keepdim=True) if unit else z
        inputs = torch.cat([zn.repeat_interleave(k, 0), rows[:, :, :3].reshape(-1, 3)], 1)
        pred = plain_forward(dec, inputs)[:, 0].reshape(B, k)
        per = (pred.clamp(-clamp, clamp) - rows[:, :, 3].clamp(-clamp, clamp)).abs().mean(1)
        loss = per.sum() if unit else (per + code_reg * z.norm(dim=1)).sum()
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        losses.append(per.detach().numpy().copy())
    return z.detach().numpy(), np.array(losses)


@pytest.mark.parametrize("name", ["w128", "lat8"])
@pytest.mark.parametrize("unit", [True, False])
def test_restatement_loop_equals_torch_float64_autograd_and_adam(name, unit):
    dec, net = PC.decoders()[name], PC.net(name)
    samples, soff, z0, k = ET.fit_case(name, seed=3, B=3, k=65)
    kw = dict(lr=5e-3, lr_step=5, lr_factor=0.1, clamp=ET.CLAMPS[name], code_reg=1e-4)
    ref = ER.loop(ET.decoder64(net), samples, soff, z0, 10, k, False, unit=unit, ft=np.float64, **kw)
    z_t, losses = _torch_fit(dec, samples, soff, z0, 10, k, unit=unit, **kw)
    assert np.abs(ref["z"] - z_t).max() <= 1e-12, float(np.abs(ref["z"] - z_t).max())
    assert np.abs(ref["history"] - losses).max() <= 1e-12
    assert np.abs(ref["z"] - z0).max() > 1e-3                                   # ten steps moved the latents


# ---- the hash ----------------------------------------------------------------------------------------------------------------------------

def test_hash_indices_are_in_range_and_uniform_within_five_sigma():
    n = 1 << 16
    for count in (1, 2, 7, 1000, (1 << 40) + 12345):
        idx = ER.draw(EC.SEED, 5, 2, np.arange(n), count)
        assert idx.min() >= 0 and idx.max() < count
    bins = 64
    for it, b in ((0, 0), (799, 63)):
        h = np.bincount(ER.draw(EC.SEED, it, b, np.arange(n), bins), minlength=bins)
        sigma = np.sqrt(n * (1.0 / bins) * (1 - 1.0 / bins))
        assert np.abs(h - n / bins).max() <= 5 * sigma, h
    # a function of (seed, iteration, shape, row) alone, and each of them matters
    a = ER.draw(EC.SEED, 3, 1, np.arange(1000), 1 << 30)
    assert np.array_equal(a, ER.draw(EC.SEED, 3, 1, np.arange(1000), 1 << 30))
    for other in (ER.draw(EC.SEED + 1, 3, 1, np.arange(1000), 1 << 30), ER.draw(EC.SEED, 4, 1, np.arange(1000), 1 << 30),
                  ER.draw(EC.SEED, 3, 2, np.arange(1000), 1 << 30)):
        assert (a != other).mean() > 0.99
    assert int(ER.mulhi64(np.uint64(0xFFFFFFFFFFFFFFFF), np.uint64(0xFFFFFFFFFFFFFFFF))) == 0xFFFFFFFFFFFFFFFE
    assert int(ER.mix64(np.uint64(1))) == 0x5692161D100B05E5                    # splitmix64's finaliser of 1


# ---- the header on the host -----------------------------------------------------------------------------------------------------------------

def _f32_bits(x):
    return struct.unpack("<I", struct.pack("<f", float(x)))[0]


def _run(exe, mode, tmp, head, arrays, expect=0):
    src, dst = os.path.join(str(tmp), "in.bin"), os.path.join(str(tmp), "out.bin")
    with open(src, "wb") as f:
        f.write(np.asarray(list(head) + [0] * (9 - len(head)), np.int64).tobytes())
        for a in arrays:
            f.write(np.ascontiguousarray(a).tobytes())
    r = subprocess.run([exe, mode, src, dst], capture_output=True, text=True)
    assert r.returncode == expect, (r.returncode, r.stderr[-3000:])
    return open(dst, "rb").read()


def _split(blob, specs):
    out, at = [], 0
    for dtype, shape in specs:
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        out.append(np.frombuffer(blob, dtype=dtype, count=int(np.prod(shape)), offset=at).reshape(shape))
        at += n
    assert at == len(blob)
    return out


def host_rows(exe, tmp, samples, soff, B, k, draw, seed, it, z, unit, S=None, shape0=0):
    L = z.shape[1]
    S = len(samples) if S is None else S
    blob = _run(exe, "rows", tmp, [S, B, k, draw, seed, it, L, unit, shape0], [np.asarray(soff, np.int64), np.asarray(samples, np.float32)[:S], z])
    return _split(blob, [(np.float32, (B * k, L + 3)), (np.float32, (B * k,)), (np.float32, (B, L)), (np.int32, (B,))])


def host_reduce(exe, tmp, pred, target, J, L, B, k, clamp, flags):
    blob = _run(exe, "reduce", tmp, [B, k, L, J.shape[1], _f32_bits(clamp)], [pred, target, J, flags])
    ch = (k + ER.CHUNK - 1) // ER.CHUNK
    loss, g, part, fl = _split(blob, [(np.float64, (B,)), (np.float64, (B, L)), (np.float64, (B, ch, L + 2)), (np.int32, (B,))])
    return loss, g, fl, part


def host_step(exe, tmp, z, m, v, g, flags, unit, code_reg, lr, t):
    B, L = z.shape
    blob = _run(exe, "step", tmp, [B, L, unit, t, _f32_bits(code_reg), _f32_bits(lr)], [z, m, v, np.asarray(g, np.float64), flags])
    return _split(blob, [(np.float32, (B, L))] * 3 + [(np.int32, (B,))])


def same_bits(a, b, what=""):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    assert np.array_equal(a.view(u), b.view(u)), (what, int((a.view(u) != b.view(u)).sum()))


def _host_checks(exe, tmp):
    for case in EC.rows_cases():
        B, counts, k, draw, L, unit = case
        samples, soff, z = EC.rows_case(*case)
        for shape0 in (0, 9):
            got = host_rows(exe, tmp, samples, soff, B, k, draw, EC.SEED, 17, z, unit, shape0=shape0)
            want = ER.rows(samples, soff, B, k, draw, EC.SEED, 17, z, unit, shape0=shape0)
            for g, w, n in zip(got, want, ("inputs", "target", "zn", "flags")):
                same_bits(g, w, (case, n))
        assert got[3][counts.index(0)] == ER.EMPTY if 0 in counts else True
    for case in EC.reduce_cases():
        B, k, L, Js = case
        pred, target, J, flags = EC.reduce_case(*case)
        got = host_reduce(exe, tmp, pred, target, J, L, B, k, EC.CLAMP, flags)
        want = ER.reduce(pred, target, J, L, B, k, EC.CLAMP, flags)
        for g, w, n in zip(got, want, ("loss", "g_zn", "flags", "part")):
            same_bits(g, w, (case, n))
        assert np.isfinite(want[0]).all() and np.isfinite(want[1][0]).all()        # the NaN Jacobian row under a zero factor added nothing
        if B >= 2:
            assert want[2][1] & ER.NO_ROWS and want[0][1] == 0 and not want[1][1].any()
        if B >= 3:
            assert not np.isfinite(want[1][B - 1, 0])
    for case in EC.step_cases():
        B, L, unit, t = case[:4]
        z, m, v, g, flags, code_reg, lr = EC.step_case(*case)
        got = host_step(exe, tmp, z, m, v, g, flags, unit, code_reg, lr, t)
        want = ER.step(z, m, v, g, flags, unit, code_reg, lr, t)
        for a, w, n in zip(got, want, ("z", "m", "v", "flags")):
            same_bits(a, w, (case, n))
        assert not want[3][0]                                                      # shape 0 stepped, every element
        if lr:
            assert (want[0][0] != z[0]).all()
        else:                                                                      # at lr = 0 Adam still runs: z stays, m and v move
            same_bits(want[0][0], z[0])
            assert (want[1][0] != m[0]).all() and (want[2][0] != v[0]).all()
        for b in range(2, B):                                                      # flagged, NaN and overflowing gradients: untouched
            assert want[3][b] & ER.SKIPPED
            same_bits(want[0][b], z[b]); same_bits(want[1][b], m[b]); same_bits(want[2][b], v[b])
    # broken tables and draw = 0 with k > count: flagged, zero rows, nothing read through them (the sanitizer build watches the reads)
    samples, soff, z = EC.rows_case(3, (70, 5, 40), 64, 0, 3, 1)
    for broken, S in (([0, -4, 75, 115], None), ([0, 80, 75, 115], None), ([0, 70, 75, 999], None), ([0, 70, 75, 115], 100), ([5, 3, 1, 0], None)):
        got = host_rows(exe, tmp, samples, broken, 3, 64, 0, EC.SEED, 0, z, 1, S=S)
        want = ER.rows(samples[:S], broken, 3, 64, 0, EC.SEED, 0, z, 1, S=S)
        for g, w in zip(got, want):
            same_bits(g, w, broken)
        assert (want[3] & ER.BAD_TABLE).any()
        for b in np.nonzero(want[3])[0]:
            assert not got[0][b * 64:(b + 1) * 64].any() and not got[1][b * 64:(b + 1) * 64].any()
    assert ER.rows(samples, soff, 3, 64, 0, EC.SEED, 0, z, 1)[3].tolist() == [0, ER.BAD_TABLE, ER.BAD_TABLE]      # k = 64 > 5 and > 40


def test_encode_cells_on_the_host_equal_the_restatement_bit_for_bit(tmp_path):
    _host_checks(build_host_program(tmp_path, "encode_host/encode_host.cpp", "encode_host"), tmp_path)


def test_encode_cells_host_program_under_sanitizers(tmp_path):
    _host_checks(build_host_program(tmp_path, "encode_host/encode_host.cpp", "encode_host_san",
                                    ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]), tmp_path)


def test_chunk_order_is_a_function_of_the_chunk_length_alone():
    rng = np.random.default_rng(4)
    v = rng.standard_normal((ER.CHUNK, 2)) * 10.0 ** rng.integers(-8, 8, (ER.CHUNK, 2))
    for n in (1, 63, 64, 65, 130, ER.CHUNK):
        want = np.zeros(2)
        slots = [v[j:n:ER.SLOTS] for j in range(ER.SLOTS)]
        acc = []
        for s in slots:
            a = np.zeros(2)
            for r in s:
                a = a + r
            acc.append(a)
        o = 32
        while o:
            for j in range(o):
                acc[j] = acc[j] + acc[j + o]
            o //= 2
        want = acc[0]
        assert np.array_equal(ER.chunk_sum(v[:n]), want)
    assert abs(ER.chunk_sum(v)[0] - float(np.sum(v[:, 0].astype(np.longdouble)))) <= 1e-12 * np.abs(v[:, 0]).sum()


# ---- exports, header, binding -------------------------------------------------------------------------------------------------------------

NAMES = ("sdfr_encode_ws_bytes", "sdfr_encode_rows", "sdfr_encode_reduce", "sdfr_encode_step")


def test_exports_header_and_binding_agree():
    header = open(os.path.join(ROOT, "include", "sdfr.h")).read()
    assert _lib.ABI_VERSION >= 418 and int(re.search(r"#define SDFR_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION
    assert "418: encoding shapes" in header
    body = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    h = _lib.lib()
    assert h.sdfr_version() == _lib.ABI_VERSION
    for name in NAMES:
        assert name in _lib.EXPORTS and hasattr(h, name) and re.search(r"\bint(64_t)? %s\(" % name, body), name
    cells = open(os.path.join(ROOT, "sdflabel_amd", "csrc", "encode_cells.h")).read()
    for name, val in (("ENC_CHUNK", ER.CHUNK), ("ENC_SLOTS", ER.SLOTS), ("ENC_MAX_L", ER.MAX_L), ("ENC_EMPTY", ER.EMPTY), ("ENC_NO_ROWS", ER.NO_ROWS),
                      ("ENC_SKIPPED", ER.SKIPPED), ("ENC_BAD_TABLE", ER.BAD_TABLE)):
        assert int(re.search(r"#define %s (\d+)" % name, cells).group(1)) == val, name
    assert (E.EMPTY, E.NO_ROWS, E.SKIPPED, E.BAD_TABLE) == (ER.EMPTY, ER.NO_ROWS, ER.SKIPPED, ER.BAD_TABLE)
    assert "train_mix64" in cells and "0xBF58476D1CE4E5B9" not in cells          # the finaliser is shared with train_cells.h, not copied


def test_c_argument_checks_need_no_gpu():
    h = _lib.lib()
    assert h.sdfr_encode_ws_bytes(3, 2124, 3) == 3 * 3 * 5 * 8
    assert h.sdfr_encode_ws_bytes(1, 1 << 20, 256) == 1024 * 258 * 8
    for bad in ((1, 0, 3), (1, (1 << 20) + 1, 3), (1, 10, 0), (1, 10, 257), (-1, 10, 3), (65536, 10, 3)):
        assert h.sdfr_encode_ws_bytes(*bad) == -1, bad
    d = 4096            # never dereferenced: every call below is refused before a launch
    inv = -1                                    # SDFR_E_INVALID
    assert h.sdfr_encode_rows(d, 10, None, 1, 0, 5, 0, 0, 0, d, 3, 1, d, d, d, d, None) == inv and b"NULL" in h.sdfr_last_error()
    assert h.sdfr_encode_rows(d, 10, d, 1, 0, 5, 0, 0, 0, d, 257, 1, d, d, d, d, None) == inv and b"latent size" in h.sdfr_last_error()
    assert h.sdfr_encode_rows(d, 10, d, 1, 0, 0, 0, 0, 0, d, 3, 1, d, d, d, d, None) == inv and b"k = 0" in h.sdfr_last_error()
    assert h.sdfr_encode_rows(d, 10, d, 1, 0, (1 << 20) + 1, 0, 0, 0, d, 3, 1, d, d, d, d, None) == inv
    assert h.sdfr_encode_rows(d, 10, d, 1, 0, 5, 0, 0, 1 << 24, d, 3, 1, d, d, d, d, None) == inv and b"iter" in h.sdfr_last_error()
    assert h.sdfr_encode_rows(d, 10, d, 2, 65534, 5, 0, 0, 0, d, 3, 1, d, d, d, d, None) == inv and b"shape0" in h.sdfr_last_error()
    assert h.sdfr_encode_reduce(d, d, d, 2, 3, 1, 5, 0.1, d, 1 << 20, d, d, d, None) == inv and b"stride" in h.sdfr_last_error()
    assert h.sdfr_encode_reduce(d, d, d, 6, 3, 1, 5, 0.1, d, 39, d, d, d, None) == inv and b"workspace" in h.sdfr_last_error()
    assert h.sdfr_encode_reduce(d, d, d, 6, 3, 1, 5, 0.0, d, 40, d, d, d, None) == inv and b"clamp" in h.sdfr_last_error()
    assert h.sdfr_encode_reduce(d, d, None, 6, 3, 1, 5, 0.1, d, 40, d, d, d, None) == inv
    assert h.sdfr_encode_step(d, d, d, 3, 1, 1, d, d, d, 1e-4, 5e-3, 0, None, 0, None) == inv and b"starts at 1" in h.sdfr_last_error()
    assert h.sdfr_encode_step(d, d, d, 3, 2, 1, d, d, d, 1e-4, 5e-3, 1, d, 1, None) == inv and b"history_stride" in h.sdfr_last_error()
    assert h.sdfr_encode_step(d, d, d, 3, 2, 1, d, d, d, 1e-4, float("nan"), 1, None, 0, None) == inv
    assert h.sdfr_encode_step(d, None, d, 3, 2, 1, d, d, d, 1e-4, 5e-3, 1, None, 0, None) == inv
    # B = 0 is a no-op
    assert h.sdfr_encode_rows(d, 10, d, 0, 0, 5, 0, 0, 0, d, 3, 1, d, d, d, d, None) == 0
    assert h.sdfr_encode_reduce(d, d, d, 6, 3, 0, 5, 0.1, d, 0, d, d, d, None) == 0
    assert h.sdfr_encode_step(d, d, d, 3, 0, 1, d, d, d, 1e-4, 5e-3, 1, None, 0, None) == 0


def test_encode_many_argument_checks_come_before_any_launch():
    dec = PC.decoders()["w128"]                                                    # on the CPU
    s = SdfSamples(torch.zeros((10, 4)))
    with pytest.raises(ValueError):
        E.encode_many(dec, [s], iters=-1)
    with pytest.raises(ValueError):
        E.encode_many(dec, [s], rows_per_iter=0)
    with pytest.raises(ValueError):
        E.encode_many(dec, [s], init=torch.zeros((1, 8)))                          # a latent size that is not the decoder's
    with pytest.raises(ValueError):
        E.encode_many(dec, [s, s], init=torch.zeros((1, 3)))
    with pytest.raises(ValueError):
        E.encode_many(dec, [SdfSamples(torch.zeros((10, 3)))])
    with pytest.raises(ValueError):
        E.encode_many(dec, [s], clamp=0.0)
    with pytest.raises(_lib.SdfrError):
        E.encode_many(dec, [s])                                                    # a CPU decoder, CPU rows
    with pytest.raises(_lib.SdfrError):
        E.encode_many(dec, s, iters=0)


def test_encode_folder_round_trip_with_the_device_call_stubbed(tmp_path, monkeypatch):
    from sdflabel_amd.pipelines import encode_shapes as ES
    rng = np.random.default_rng(2)
    sdir = tmp_path / "samples"
    sdir.mkdir()
    for name, n in (("b_chair", 12), ("a_car", 7)):
        SdfSamples(torch.from_numpy(rng.uniform(-1, 1, (n, 4)).astype(np.float32))).save(str(sdir / (name + ".npz")))
    seen = {}

    class FakeDecoder:
        def to(self, device):
            seen["device"] = device
            return self

        def eval(self):
            return self

    def fake_setup(path, precision=torch.float32):
        seen["prior"] = path
        return (FakeDecoder(), 3)

    def fake_encode(dsdf, samples, **kw):
        seen["dsdf"], seen["counts"], seen["kw"] = dsdf, [len(s) for s in samples], kw
        B = len(samples)
        raw = torch.arange(B * 3, dtype=torch.float32).reshape(B, 3) + 1
        return E.Encoded(raw / raw.norm(dim=1, keepdim=True), raw, torch.tensor([0.25, 0.5], dtype=torch.float64), torch.tensor([0, 4], dtype=torch.int32),
                         None, True)

    monkeypatch.setattr(ES, "setup_dsdf", fake_setup)
    monkeypatch.setattr(ES, "encode_many", fake_encode)
    out = ES.encode_folder("prior.pt", str(sdir), str(tmp_path / "held_out.pt"), device="cpu", iters=5)
    assert out == str(tmp_path / "held_out_latents.pt") and os.path.isfile(out)
    assert seen["prior"] == "prior.pt" and isinstance(seen["dsdf"], FakeDecoder) and seen["device"] == "cpu" and seen["counts"] == [7, 12] and seen["kw"] == {"iters": 5}
    d = torch.load(out)
    assert set(d) == {"latents", "raw_latents", "unit_latents", "files", "loss", "flags"}
    assert [os.path.basename(f) for f in d["files"]] == ["a_car.npz", "b_chair.npz"]
    assert d["unit_latents"] is True and d["latents"].shape == (2, 3) and d["raw_latents"][1].tolist() == [4.0, 5.0, 6.0]
    assert d["loss"].tolist() == [0.25, 0.5] and d["flags"].tolist() == [0, 4]
    with pytest.raises(FileNotFoundError):
        ES.encode_folder("prior.pt", str(tmp_path), str(tmp_path / "x.pt"), device="cpu")


# ---- the trajectory cases and their bound -----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def trajectories():
    """name -> (float64 run with its kink margins, float32 emulation run); computed once"""
    return {name: ET.cpu_runs(name) for name in ET.NAMES}


@pytest.mark.parametrize("name", ET.NAMES)
def test_float64_run_admits_every_row_of_the_trajectory_cases(trajectories, name):
    ref, _ = trajectories[name]
    assert ref["margin"].shape == (ET.STEPS, ET.B * ET.K)
    assert ref["margin"].min() > 1.0, float(ref["margin"].min())                 # no row within m = 100 fwd_tol of a kink on any step
    assert not ref["flags"].any() and np.abs(ref["z"] - ref["z0"]).max() > 1e-3


@pytest.mark.parametrize("name", ET.NAMES)
def test_trajectory_bound_is_four_times_the_emulations_worst_deviation(trajectories, name):
    ref, emu = trajectories[name]
    worst = max(float(np.abs(a - b).max()) for a, b in zip(emu["zs"], ref["zs"]))
    print("%s: emulation deviates %.3e from float64 over %d steps; bound %.3e" % (name, worst, ET.STEPS, EC.TRAJECTORY_BOUND[name]))
    assert worst > 0
    assert 4 * worst <= EC.TRAJECTORY_BOUND[name] <= 4 * worst * 1.05, (worst, EC.TRAJECTORY_BOUND[name])


def test_recovery_case_reference_reaches_a_tenth_of_its_initial_loss():
    ref = ET.recovery_reference()
    h = ref["history"][:, 0]
    print("recovery: float64 loss %.4e -> %.4e" % (h[0], h[-1]))
    assert h[-1] <= 0.1 * h[0], (h[0], h[-1])
