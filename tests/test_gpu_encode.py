"""The shape encoder on the device (csrc/encode.hip, sdflabel_amd/encode.py): each kernel against the numpy restatement bit for bit between
guard words, batch independence, broken tables, one whole iteration of encode_many against the restatement fed with the device's own decoder
values, a ten-step trajectory against the float64 loop within the bound calibrated on the CPU (tests/test_encode_cpu.py), the recovery of a known
latent, no host traffic in the loop, and meshes / folders end to end.
"""
import copy
import warnings

import numpy as np
import pytest
import torch

from sdflabel_amd import _lib
from sdflabel_amd import encode as E
from sdflabel_amd import mesh as M
from sdflabel_amd.deepsdf.workspace import setup_dsdf
from sdflabel_amd.fixtures import ASSET, ASSET_ELLIPSOID_LN
from sdflabel_amd.sdf_samples import SdfSamples, prior_residuals
from tests import _encode_cases as EC
from tests import _encode_ref as ER
from tests import _encode_traj as ET
from tests import _prior_train_cases as PC

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64
SENT = {torch.float32: -777.25, torch.float64: -777.25, torch.int32: -77725, torch.int64: -77725}


class Guarded:
    """a device buffer with sentinel words before and behind it; `.t` is the part the kernels get"""

    def __init__(self, init, dtype=None):
        a = torch.from_numpy(np.array(init)) if isinstance(init, np.ndarray) else None
        dtype = a.dtype if a is not None else dtype
        size = a.numel() if a is not None else int(init)
        self.sent = SENT[dtype]
        self.buf = torch.full((size + 2 * GUARD,), self.sent, dtype=dtype, device=DEV)
        self.t = self.buf[GUARD:GUARD + size]
        if a is not None:
            self.t.copy_(a.reshape(-1).to(DEV))

    def intact(self):
        return bool((self.buf[:GUARD] == self.sent).all()) and bool((self.buf[-GUARD:] == self.sent).all())

    def numpy(self, shape=None):
        a = self.t.cpu().numpy()
        return a if shape is None else a.reshape(shape)


def same_bits(a, b, what=""):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    assert np.array_equal(a.view(u), b.view(u)), (what, int((a.view(u) != b.view(u)).sum()))


def count_syncs(fn):
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            out = fn()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    return sum("synchroniz" in str(x.message).lower() for x in w), out


def st():
    return _lib.stream_ptr()


# ---- the kernels through the C ABI -----------------------------------------------------------------------------------------------------------

def dev_rows(samples, soff, B, k, draw, seed, it, z, unit, S=None, shape0=0):
    L = z.shape[1]
    S = len(samples) if S is None else S
    sm = Guarded(np.asarray(samples, np.float32)[:S] if S else np.zeros((1, 4), np.float32))
    so, zz = Guarded(np.asarray(soff, np.int64)), Guarded(np.asarray(z, np.float32))
    inputs, target, zn, flags = Guarded(B * k * (L + 3), torch.float32), Guarded(B * k, torch.float32), Guarded(B * L, torch.float32), \
        Guarded(B, torch.int32)
    _lib.check(_lib.lib().sdfr_encode_rows(sm.t.data_ptr(), S, so.t.data_ptr(), B, shape0, k, draw, seed, it, zz.t.data_ptr(), L, unit,
                                           inputs.t.data_ptr(), target.t.data_ptr(), zn.t.data_ptr(), flags.t.data_ptr(), st()), "sdfr_encode_rows")
    torch.cuda.synchronize()
    for g in (sm, so, zz, inputs, target, zn, flags):
        assert g.intact()
    return inputs.numpy((B * k, L + 3)), target.numpy(), zn.numpy((B, L)), flags.numpy()


def dev_reduce(pred, target, J, L, B, k, clamp, flags):
    h = _lib.lib()
    nbytes = int(h.sdfr_encode_ws_bytes(B, k, L))
    ch = (k + ER.CHUNK - 1) // ER.CHUNK
    assert nbytes == B * ch * (L + 2) * 8
    p, t, j, fl = Guarded(np.asarray(pred)), Guarded(np.asarray(target)), Guarded(np.asarray(J)), Guarded(np.asarray(flags, np.int32).copy())
    ws, loss, g = Guarded(nbytes // 8, torch.float64), Guarded(B, torch.float64), Guarded(B * L, torch.float64)
    _lib.check(h.sdfr_encode_reduce(p.t.data_ptr(), t.t.data_ptr(), j.t.data_ptr(), J.shape[1], L, B, k, float(clamp), ws.t.data_ptr(), nbytes,
                                    loss.t.data_ptr(), g.t.data_ptr(), fl.t.data_ptr(), st()), "sdfr_encode_reduce")
    torch.cuda.synchronize()
    for x in (p, t, j, fl, ws, loss, g):
        assert x.intact()
    return loss.numpy(), g.numpy((B, L)), fl.numpy(), ws.numpy((B, ch, L + 2))


def dev_step(z, m, v, g, flags, unit, code_reg, lr, t, loss=None, history_rows=0):
    B, L = z.shape
    zz, mm, vv = Guarded(np.array(z, np.float32)), Guarded(np.array(m, np.float32)), Guarded(np.array(v, np.float32))
    gg, fl = Guarded(np.asarray(g, np.float64)), Guarded(np.asarray(flags, np.int32).copy())
    ls = Guarded(np.zeros((B,), np.float64) if loss is None else np.asarray(loss, np.float64))
    hist = Guarded(history_rows * (B + 2), torch.float32) if history_rows else None
    _lib.check(_lib.lib().sdfr_encode_step(zz.t.data_ptr(), mm.t.data_ptr(), vv.t.data_ptr(), L, B, unit, gg.t.data_ptr(), ls.t.data_ptr(),
                                           fl.t.data_ptr(), float(code_reg), float(lr), t, hist.t.data_ptr() if hist else None, B + 2, st()),
               "sdfr_encode_step")
    torch.cuda.synchronize()
    for x in (zz, mm, vv, gg, fl, ls) + ((hist,) if hist else ()):
        assert x.intact()
    return zz.numpy((B, L)), mm.numpy((B, L)), vv.numpy((B, L)), fl.numpy(), (hist.numpy((history_rows, B + 2)) if hist else None)


@pytest.mark.parametrize("case", EC.rows_cases(), ids=lambda c: "B%d_k%d_d%d_L%d_u%d" % (c[0], c[2], c[3], c[4], c[5]))
def test_rows_kernel_equals_the_restatement(case):
    B, counts, k, draw, L, unit = case
    samples, soff, z = EC.rows_case(*case)
    for shape0 in (0, 9):
        got = dev_rows(samples, soff, B, k, draw, EC.SEED, 17, z, unit, shape0=shape0)
        want = ER.rows(samples, soff, B, k, draw, EC.SEED, 17, z, unit, shape0=shape0)
        for g, w, n in zip(got, want, ("inputs", "target", "zn", "flags")):
            same_bits(g, w, (case, n))


@pytest.mark.parametrize("case", EC.reduce_cases(), ids=lambda c: "B%d_k%d_L%d_s%d" % c)
def test_reduce_kernel_equals_the_restatement(case):
    B, k, L, Js = case
    pred, target, J, flags = EC.reduce_case(*case)
    got = dev_reduce(pred, target, J, L, B, k, EC.CLAMP, flags)
    want = ER.reduce(pred, target, J, L, B, k, EC.CLAMP, flags)
    for g, w, n in zip(got, want, ("loss", "g_zn", "flags", "part")):
        same_bits(g, w, (case, n))


@pytest.mark.parametrize("case", EC.step_cases(), ids=lambda c: "B%d_L%d_u%d_t%d" % c[:4] + ("_lr0" if len(c) > 4 else ""))
def test_step_kernel_equals_the_restatement(case):
    B, L, unit, t = case[:4]
    z, m, v, g, flags, code_reg, lr = EC.step_case(*case)
    loss = np.linspace(0.01, 0.09, B)
    got = dev_step(z, m, v, g, flags, unit, code_reg, lr, t, loss=loss, history_rows=t if t < 10 else 0)
    want = ER.step(z, m, v, g, flags, unit, code_reg, lr, t)
    for a, w, n in zip(got, want, ("z", "m", "v", "flags")):
        same_bits(a, w, (case, n))
    if got[4] is not None:                                                  # history[t - 1][b] = float32(loss[b]), nothing else written
        same_bits(got[4][t - 1, :B], loss.astype(np.float32))
        rest = np.delete(got[4].reshape(-1), np.arange((t - 1) * (B + 2), (t - 1) * (B + 2) + B))
        assert (rest == SENT[torch.float32]).all()


def test_a_shapes_results_do_not_depend_on_the_batch_and_repeat():
    B, k, L, Js = 5, 2 * ER.CHUNK + 76, 8, 16
    pred, target, J, flags = EC.reduce_case(B, k, L, Js)
    whole = dev_reduce(pred, target, J, L, B, k, EC.CLAMP, flags)
    again = dev_reduce(pred, target, J, L, B, k, EC.CLAMP, flags)
    for a, b in zip(whole, again):
        same_bits(a, b, "run twice")
    order = [3, 0, 4, 2, 1]
    idx = np.concatenate([np.arange(b * k, (b + 1) * k) for b in order])
    moved = dev_reduce(pred[idx], target[idx], J[idx], L, B, k, EC.CLAMP, flags[order])
    for i, b in enumerate(order):
        alone = dev_reduce(pred[b * k:(b + 1) * k], target[b * k:(b + 1) * k], J[b * k:(b + 1) * k], L, 1, k, EC.CLAMP, flags[b:b + 1])
        for x in range(4):
            same_bits(whole[x][b], moved[x][i], ("moved", b, x))
            same_bits(whole[x][b], alone[x][0], ("alone", b, x))
    z, m, v, g, fl, code_reg, lr = EC.step_case(5, 8, 1, 400)
    whole = dev_step(z, m, v, g, fl, 1, code_reg, lr, 400)
    moved = dev_step(z[order], m[order], v[order], g[order], fl[order], 1, code_reg, lr, 400)
    for i, b in enumerate(order):
        alone = dev_step(z[b:b + 1], m[b:b + 1], v[b:b + 1], g[b:b + 1], fl[b:b + 1], 1, code_reg, lr, 400)
        for x in range(4):
            same_bits(whole[x][b], moved[x][i], ("step moved", b, x))
            same_bits(whole[x][b], alone[x][0], ("step alone", b, x))
    # draw = 0: a shape's rows do not depend on the batch either
    samples, soff, zz = EC.rows_case(5, (70, 0, 300, 65, 64), 64, 0, 8, 1)
    whole = dev_rows(samples, soff, 5, 64, 0, EC.SEED, 3, zz, 1)
    alone = dev_rows(samples[soff[2]:soff[3]], [0, 300], 1, 64, 0, EC.SEED, 3, zz[2:3], 1)
    same_bits(whole[0][2 * 64:3 * 64], alone[0]); same_bits(whole[1][2 * 64:3 * 64], alone[1]); same_bits(whole[2][2], alone[2][0])


def test_broken_tables_are_flagged_not_faults():
    samples, soff, z = EC.rows_case(3, (70, 5, 40), 64, 0, 3, 1)
    for broken, S in (([0, -4, 75, 115], None), ([0, 80, 75, 115], None), ([0, 70, 75, 999], None), ([0, 70, 75, 115], 100), ([5, 3, 1, 0], None),
                      ([0, 1 << 40, 1 << 41, 1 << 42], None)):
        for draw in (0, 1):
            got = dev_rows(samples, broken, 3, 64, draw, EC.SEED, 0, z, 1, S=S)                    # guard words checked inside
            want = ER.rows(samples[:S], broken, 3, 64, draw, EC.SEED, 0, z, 1, S=S)
            for g, w in zip(got, want):
                same_bits(g, w, (broken, draw))
            assert (got[3] & ER.BAD_TABLE).any()
            for b in np.nonzero(got[3])[0]:
                assert not got[0][b * 64:(b + 1) * 64].any() and not got[1][b * 64:(b + 1) * 64].any()
    # draw = 0 with k > count
    got = dev_rows(samples, soff, 3, 64, 0, EC.SEED, 0, z, 1)
    assert got[3].tolist() == [0, ER.BAD_TABLE, ER.BAD_TABLE] and got[0][:64].any() and not got[0][64:].any()
    # a flagged shape is never stepped
    zs, m, v, fl = dev_step(z, np.zeros_like(z), np.zeros_like(z), np.full((3, 3), 0.01), got[3], 1, 1e-4, 5e-3, 1)[:4]
    assert fl.tolist() == [0, ER.BAD_TABLE | ER.SKIPPED, ER.BAD_TABLE | ER.SKIPPED]
    same_bits(zs[1:], z[1:]); assert not m[1:].any() and not v[1:].any() and (zs[0] != z[0]).all()
    # what the host can see is an error code with a message
    h = _lib.lib()
    d = torch.zeros((64,), device=DEV).data_ptr()
    assert h.sdfr_encode_rows(d, 10, d, 1, 0, 0, 0, 0, 0, d, 3, 1, d, d, d, d, st()) == -1 and b"k = 0" in h.sdfr_last_error()
    assert h.sdfr_encode_reduce(d, d, d, 6, 3, 1, 5, 0.1, d, 39, d, d, d, st()) == -1 and b"workspace" in h.sdfr_last_error()


# ---- encode_many -------------------------------------------------------------------------------------------------------------------------------

def gpu_decoder(name):
    if name == "ln":
        return setup_dsdf(ASSET_ELLIPSOID_LN + ".pt", precision=torch.float32)[0].to(DEV).eval()
    if name in ("f16", "asset"):                   # (loaded afresh: a weight-norm module has no deepcopy)
        return setup_dsdf(ASSET + ".pt", precision=torch.float16 if name == "f16" else torch.float32)[0].to(DEV).eval()
    return copy.deepcopy(PC.decoders()[name]).to(DEV).eval()


def device_pred_and_J(dec, inputs):
    """the decoder entry points on staged rows, called here: the forward of the decoder's mode with its masks saved, then the mask-fed Jacobian"""
    h = _lib.lib()
    handle = dec.handle(torch.device(DEV, torch.cuda.current_device()))
    f16 = dec.mlp_precision == torch.float16 and not handle.has_ln
    x = torch.from_numpy(np.array(inputs)).to(DEV)
    n, ni = x.shape
    pred, sel, J = torch.empty((n,), device=DEV), torch.empty((n,), device=DEV), torch.empty((n, ni), device=DEV)
    idx, cnt = torch.arange(n, dtype=torch.int32, device=DEV), torch.full((1,), n, dtype=torch.int32, device=DEV)
    masks = None if handle.has_ln else torch.empty((int(h.sdfr_decoder_mask_words(handle.h, n)),), dtype=torch.int32, device=DEV)
    fwd = h.sdfr_mlp_forward_f16 if f16 else h.sdfr_mlp_forward
    P = _lib.ptr
    _lib.check(fwd(handle.h, P(x), n, P(pred), P(masks), st()), "forward")
    _lib.check(h.sdfr_mlp_jacobian(handle.h, P(x), n, 1, P(idx), n, P(cnt), P(J), P(sel), P(pred) if masks is not None else None, P(masks),
                                   2 if f16 else 0, st()), "sdfr_mlp_jacobian")
    torch.cuda.synchronize()
    return pred.cpu().numpy(), J.cpu().numpy()


ONE_CLAMP = 0.5          # the one-iteration tests: wide enough that every case decoder has rows inside it (lat8's values all lie below -0.12)


def shapes_of(L, B=3, n=200, seed=0):
    rng = np.random.default_rng(500 + seed + L)
    rows = np.concatenate([rng.uniform(-1, 1, (B * n, 3)), rng.uniform(-0.12, 0.12, (B * n, 1))], 1).astype(np.float32)
    z0 = (0.5 * rng.standard_normal((B, L))).astype(np.float32)
    return rows, np.arange(B + 1, dtype=np.int64) * n, z0


@pytest.mark.parametrize("draw", [False, True])
@pytest.mark.parametrize("name", ["w128", "lat8", "tanh", "xyz", "asset", "ln", "f16"])
def test_one_iteration_equals_the_restatement_on_the_devices_own_decoder_values(name, draw):
    dec = gpu_decoder(name)
    L, B, n = int(dec.latent_size), 3, 200
    rows, soff, z0 = shapes_of(L, B, n)
    k = 128 if draw else n
    samples = [SdfSamples(torch.from_numpy(rows[soff[b]:soff[b + 1]]).to(DEV)) for b in range(B)]
    kw = dict(iters=1, rows_per_iter=k, lr=5e-3, clamp=ONE_CLAMP, init=torch.from_numpy(z0), seed=11, history=True, draw=draw)
    enc = E.encode_many(dec, samples, **kw)
    inputs, target, zn0, flags = ER.rows(rows, soff, B, k, draw, 11, 0, z0, True)
    pred, J = device_pred_and_J(dec, inputs)
    loss, g, flags, _ = ER.reduce(pred, target, J, L, B, k, ONE_CLAMP, flags)
    z1, _, _, flags = ER.step(z0, np.zeros_like(z0), np.zeros_like(z0), g, flags, True, 1e-4, 5e-3, 1)
    assert not flags.any() and (np.abs(g).max(1) > 0).all()                  # every shape has rows inside the clamp
    same_bits(enc.raw_latents.cpu().numpy(), z1, name)
    same_bits(enc.latents.cpu().numpy(), ER.normalised(z1, True), name)
    same_bits(enc.loss.cpu().numpy(), loss, name)
    same_bits(enc.history.cpu().numpy(), loss.astype(np.float32)[None], name)
    assert enc.flags.cpu().numpy().tolist() == [0] * B
    # staged one shape at a time: the same bits (the hash takes the shape's index in the call, not in its group)
    one = E.encode_many(dec, samples, staging_bytes=1, **kw)
    same_bits(one.raw_latents.cpu().numpy(), z1, "staged")
    same_bits(one.loss.cpu().numpy(), loss, "staged")


def test_raw_latents_take_the_regulariser_and_empty_shapes_are_left_alone():
    dec = gpu_decoder("w128")
    rows, soff, z0 = shapes_of(3, 3, 200, seed=1)
    z0[2] = 0.0
    samples = [SdfSamples(torch.from_numpy(rows[:200]).to(DEV)), SdfSamples(torch.zeros((0, 4), device=DEV)), SdfSamples(torch.from_numpy(rows[400:]).to(DEV))]
    enc = E.encode_many(dec, samples, iters=1, rows_per_iter=200, init=torch.from_numpy(z0), unit_latents=False, code_reg=1e-2)
    soff = np.array([0, 200, 200, 400], np.int64)
    rr = np.concatenate([rows[:200], rows[400:]])
    inputs, target, _, flags = ER.rows(rr, soff, 3, 200, False, 0, 0, z0, False)
    pred, J = device_pred_and_J(dec, inputs)
    loss, g, flags, _ = ER.reduce(pred, target, J, 3, 3, 200, 0.1, flags)
    z1, _, _, flags = ER.step(z0, np.zeros_like(z0), np.zeros_like(z0), g, flags, False, 1e-2, 5e-3, 1)
    assert flags.tolist() == [0, ER.EMPTY | ER.SKIPPED, 0]
    same_bits(enc.raw_latents.cpu().numpy(), z1); same_bits(enc.latents.cpu().numpy(), z1)
    assert enc.flags.cpu().numpy().tolist() == flags.tolist()
    same_bits(enc.raw_latents.cpu().numpy()[1], z0[1])
    start = E.encode_many(dec, samples, iters=0, init=torch.from_numpy(z0))                       # iters = 0 returns the start
    same_bits(start.raw_latents.cpu().numpy(), z0); same_bits(start.latents.cpu().numpy(), ER.normalised(z0, True))
    assert start.flags.cpu().numpy().tolist() == [0, ER.EMPTY, 0] and torch.isnan(start.loss).all()


@pytest.mark.parametrize("name", ET.NAMES)
def test_ten_step_trajectory_stays_within_the_calibrated_bound_of_the_float64_loop(name):
    """Measured on an MI355X, max |z - z_float64| over the raw latents after ten steps: w128 2.45e-7 (bound 6.1e-5), lat8 6.44e-8 (3.6e-7), asset
    1.46e-7 (3.9e-7); profiles/encode_notes.md."""
    dec = gpu_decoder(name)
    samples, soff, z0, k = ET.fit_case(name, EC.TRAJECTORY_SEED[name], ET.B, ET.K)
    ref = ET.run(name, ET.decoder64(PC.net(name)), np.float64, samples, soff, z0, k, ET.STEPS, watch_margin=True, clamp=ET.CLAMPS[name], **ET.FIT)
    assert ref["margin"].min() > 1.0                                          # every row admitted: none within 100 fwd_tol of a kink
    sam = [SdfSamples(torch.from_numpy(np.array(samples[soff[b]:soff[b + 1]])).to(DEV)) for b in range(ET.B)]
    enc = E.encode_many(dec, sam, iters=ET.STEPS, rows_per_iter=k, init=torch.from_numpy(np.array(z0)), clamp=ET.CLAMPS[name], history=True, **ET.FIT)
    dev = float(np.abs(enc.raw_latents.cpu().numpy().astype(np.float64) - ref["z"]).max())
    dl = float(np.abs(enc.history.cpu().numpy().astype(np.float64) - ref["history"]).max())
    print("%s: device deviates %.3e from float64 after %d steps (bound %.3e); loss history %.3e" % (name, dev, ET.STEPS, EC.TRAJECTORY_BOUND[name], dl))
    assert not enc.flags.any()
    assert dev <= EC.TRAJECTORY_BOUND[name], (dev, EC.TRAJECTORY_BOUND[name])


def test_recovery_of_a_known_latent():
    dec = gpu_decoder("w128")
    samples, soff, z_true, z0 = ET.recovery_case()
    ref = ET.recovery_reference()["history"][:, 0]
    assert ref[-1] <= 0.1 * ref[0]
    sam = SdfSamples(torch.from_numpy(np.array(samples)).to(DEV))
    r = ET.RECOVERY
    enc = E.encode_many(dec, sam, iters=r["iters"], rows_per_iter=r["n"], lr=r["lr"], lr_step=r["lr_step"], lr_factor=r["lr_factor"], clamp=r["clamp"],
                        init=torch.from_numpy(z0), history=True)
    h = enc.history.cpu().numpy()[:, 0]
    print("recovery: device loss %.4e -> %.4e, float64 %.4e -> %.4e; latent %s for %s" % (h[0], h[-1], ref[0], ref[-1], enc.latents.cpu().numpy(), z_true))
    assert 0.5 * ref[-1] <= h[-1] <= 2.0 * ref[-1], (h[-1], ref[-1])
    after, _ = prior_residuals(dec, enc.latents, sam)
    before, _ = prior_residuals(dec, torch.from_numpy(z0).to(DEV), sam)
    assert float(after[0]) < float(before[0])


def test_no_host_traffic_in_the_loop():
    dec = gpu_decoder("w128")
    rows, soff, z0 = shapes_of(3, 3, 200, seed=2)
    samples = [SdfSamples(torch.from_numpy(rows[soff[b]:soff[b + 1]]).to(DEV)) for b in range(3)]
    init = torch.from_numpy(z0).to(DEV)
    E.encode_many(dec, samples, iters=2, rows_per_iter=64, init=init)                                # the handle and the library are loaded
    syncs, enc = count_syncs(lambda: E.encode_many(dec, samples, iters=20, rows_per_iter=64, init=init, history=True))
    assert syncs == 0, syncs
    assert enc.loss.is_cuda and enc.flags.is_cuda and enc.history.is_cuda and enc.latents.is_cuda and tuple(enc.history.shape) == (20, 3)


def test_meshes_and_folders_end_to_end(tmp_path):
    dec = gpu_decoder("asset")
    z_true = torch.nn.functional.normalize(torch.tensor([[0.3, -0.5, 0.8]]), dim=1).to(DEV)
    (mesh,) = M.meshes_many(dec, z_true, resolution=24)
    assert mesh.is_closed()
    gen = torch.Generator().manual_seed(5)
    enc = E.encode_meshes(dec, [mesh], n=6000, generator=gen, iters=120, rows_per_iter=2000, lr=2e-2, lr_step=80, init=-z_true.cpu())
    samples = enc.samples
    got, _ = prior_residuals(dec, enc.latents, samples)
    far, _ = prior_residuals(dec, -z_true, samples)
    print("end to end: residual %.4e at the encoded latent %s, %.4e at the antipode of %s" % (float(got[0]), enc.latents.cpu().numpy(), float(far[0]),
                                                                                              z_true.cpu().numpy()))
    assert float(got[0]) < float(far[0]) and int(enc.flags[0]) == 0
    (again,) = M.meshes_many(dec, enc.latents, resolution=24)
    assert again.is_closed() and len(again) > 0
    enc2 = mesh.encode(dec, n=2000, generator=torch.Generator().manual_seed(5), iters=2, rows_per_iter=500)
    assert tuple(enc2.latents.shape) == (1, 3) and len(enc2.samples[0]) == 2000
    # a folder of two .npz files as SdfSamples.save writes them
    from sdflabel_amd.pipelines.encode_shapes import encode_folder
    sdir = tmp_path / "samples"
    sdir.mkdir()
    samples[0].save(str(sdir / "b.npz"))
    SdfSamples(samples[0].rows[:3000]).save(str(sdir / "a.npz"))
    out = encode_folder(ASSET + ".pt", str(sdir), str(tmp_path / "held_out.pt"), device=DEV, iters=5, rows_per_iter=1000)
    d = torch.load(out)
    assert set(d) == {"latents", "raw_latents", "unit_latents", "files", "loss", "flags"} and d["unit_latents"] is True
    assert [f[-5:] for f in d["files"]] == ["a.npz", "b.npz"] and tuple(d["latents"].shape) == (2, 3) and d["flags"].tolist() == [0, 0]
    assert torch.isfinite(d["loss"]).all() and torch.allclose(d["latents"].norm(dim=1), torch.ones(2), atol=1e-6)
