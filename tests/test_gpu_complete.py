"""Shape completion from one view on the device (csrc/complete.hip, sdflabel_amd/complete.py): each kernel against the numpy restatement bit
for bit between guard words, batch independence, broken tables, fit_many on exact rows = encode_many in every bit, a ten-step trajectory on
mixed rows against the float64 loop within the bound calibrated on the CPU (tests/test_complete_cpu.py), no host traffic, the completion of
a meshed shape from its camera-facing side, and the stage of refine_frame.
"""
import numpy as np
import pytest
import torch

from sdflabel_amd import _lib
from sdflabel_amd import complete as C
from sdflabel_amd import encode as E
from sdflabel_amd.fixtures import ASSET
from sdflabel_amd.sdf_samples import SdfSamples, prior_residuals
from tests import _complete_cases as CC
from tests import _complete_ref as CR
from tests import _complete_traj as CT
from tests import _encode_ref as ER
from tests import _encode_traj as ET
from tests import _prior_train_cases as PC
from tests.test_gpu_encode import DEV, Guarded, count_syncs, gpu_decoder, same_bits, shapes_of, st

pytestmark = pytest.mark.gpu


# ---- the kernels through the C ABI -----------------------------------------------------------------------------------------------------------

def dev_view(pts, nrm, ptoff, pose, origin, F, eta, s_max, seed, shape0=0, N=None):
    N = len(pts) if N is None else N
    B, P = len(pose), 3 + F
    pp = Guarded(np.asarray(pts, np.float32)[:N] if N else np.zeros((1, 3), np.float32))
    nn = None if nrm is None else Guarded(np.asarray(nrm, np.float64)[:N] if N else np.zeros((1, 3), np.float64))
    po, ps, og = Guarded(np.asarray(ptoff, np.int64)), Guarded(np.asarray(pose, np.float32)), Guarded(np.asarray(origin, np.float32))
    rows, flags = Guarded(max(N * P * 5, 1), torch.float32), Guarded(B, torch.int32)
    _lib.check(_lib.lib().sdfr_view_samples(pp.t.data_ptr(), nn.t.data_ptr() if nn else None, N, po.t.data_ptr(), B, ps.t.data_ptr(), og.t.data_ptr(),
                                            shape0, F, float(eta), float(s_max), seed, rows.t.data_ptr(), flags.t.data_ptr(), st()), "sdfr_view_samples")
    torch.cuda.synchronize()
    for g in (pp, po, ps, og, rows, flags) + ((nn,) if nn else ()):
        assert g.intact()
    got = rows.numpy()
    if N == 0:
        assert got[0] == rows.sent                                               # nothing written
    return got[:N * P * 5].reshape(N * P, 5), flags.numpy()


def dev_rows(samples, soff, B, k, draw, seed, it, z, unit, S=None, shape0=0):
    L = z.shape[1]
    S = len(samples) if S is None else S
    sm = Guarded(np.asarray(samples, np.float32)[:S] if S else np.zeros((1, 5), np.float32))
    so, zz = Guarded(np.asarray(soff, np.int64)), Guarded(np.asarray(z, np.float32))
    inputs, lo, hi, zn, flags = Guarded(B * k * (L + 3), torch.float32), Guarded(B * k, torch.float32), Guarded(B * k, torch.float32), \
        Guarded(B * L, torch.float32), Guarded(B, torch.int32)
    _lib.check(_lib.lib().sdfr_bound_rows(sm.t.data_ptr(), S, so.t.data_ptr(), B, shape0, k, draw, seed, it, zz.t.data_ptr(), L, unit, inputs.t.data_ptr(),
                                          lo.t.data_ptr(), hi.t.data_ptr(), zn.t.data_ptr(), flags.t.data_ptr(), st()), "sdfr_bound_rows")
    torch.cuda.synchronize()
    for g in (sm, so, zz, inputs, lo, hi, zn, flags):
        assert g.intact()
    return inputs.numpy((B * k, L + 3)), lo.numpy(), hi.numpy(), zn.numpy((B, L)), flags.numpy()


def dev_reduce(pred, lo, hi, J, L, B, k, clamp, flags):
    h = _lib.lib()
    nbytes = int(h.sdfr_encode_ws_bytes(B, k, L))
    ch = (k + ER.CHUNK - 1) // ER.CHUNK
    p, a, e, j, fl = (Guarded(np.asarray(x)) for x in (pred, lo, hi, J, np.asarray(flags, np.int32).copy()))
    ws, loss, g = Guarded(nbytes // 8, torch.float64), Guarded(B, torch.float64), Guarded(B * L, torch.float64)
    _lib.check(h.sdfr_bound_reduce(p.t.data_ptr(), a.t.data_ptr(), e.t.data_ptr(), j.t.data_ptr(), J.shape[1], L, B, k, float(clamp), ws.t.data_ptr(), nbytes,
                                   loss.t.data_ptr(), g.t.data_ptr(), fl.t.data_ptr(), st()), "sdfr_bound_reduce")
    torch.cuda.synchronize()
    for x in (p, a, e, j, fl, ws, loss, g):
        assert x.intact()
    return loss.numpy(), g.numpy((B, L)), fl.numpy(), ws.numpy((B, ch, L + 2))


@pytest.mark.parametrize("case", CC.view_cases(), ids=lambda c: "B%d_n%s_F%d_%s_%s" % (c[0], "-".join(map(str, c[1])), c[2], c[3], c[4]))
def test_view_kernel_equals_the_restatement(case):
    B, counts, F, normals, special = case
    pts, ptoff, pose, origin, nrm = CC.view_case(*case)
    for shape0 in (0, 9):
        got = dev_view(pts, nrm, ptoff, pose, origin, F, CC.ETA, CC.S_MAX, CC.SEED, shape0)
        want = CR.view_rows(pts, nrm, ptoff, pose, origin, F, CC.ETA, CC.S_MAX, CC.SEED, shape0)
        same_bits(got[0], want[0], (case, "rows")); same_bits(got[1], want[1], (case, "flags"))


def test_broken_point_tables_are_flagged_not_faults():
    pts, ptoff, pose, origin, nrm = CC.view_case(3, (65, 65, 65), 4, "all", None)
    for broken in CC.BROKEN_PTOFF:
        for N in (195, 100):
            got = dev_view(pts, nrm, broken, pose, origin, 4, CC.ETA, CC.S_MAX, CC.SEED, N=N)              # guard words checked inside
            want = CR.view_rows(pts[:N], nrm[:N], broken, pose, origin, 4, CC.ETA, CC.S_MAX, CC.SEED, N=N)
            same_bits(got[0], want[0], (broken, N)); same_bits(got[1], want[1], (broken, N))
            bad = [a < 0 or e < a or e > N for a, e in zip(broken[:-1], broken[1:])]
            assert [bool(f & CR.BAD_TABLE) for f in got[1]] == bad
    h = _lib.lib()
    d = torch.zeros((64,), device=DEV).data_ptr()
    assert h.sdfr_view_samples(d, d, 4, d, 1, d, d, 0, 65, 0.01, 0.5, 0, d, d, st()) == -1 and b"free-space" in h.sdfr_last_error()


@pytest.mark.parametrize("case", CC.rows_cases(), ids=lambda c: "B%d_k%d_d%d_L%d_u%d" % (c[0], c[2], c[3], c[4], c[5]))
def test_bound_rows_kernel_equals_the_restatement(case):
    B, counts, k, draw, L, unit = case
    samples, soff, z = CC.rows_case(*case)
    got = dev_rows(samples, soff, B, k, draw, CC.SEED, 17, z, unit, shape0=2)
    want = CR.rows(samples, soff, B, k, draw, CC.SEED, 17, z, unit, shape0=2)
    for g, w, n in zip(got, want, ("inputs", "lo", "hi", "zn", "flags")):
        same_bits(g, w, (case, n))


def test_broken_sample_tables_are_flagged_not_faults():
    samples, soff, z = CC.rows_case(3, (65, 0, 72), 65, 0, 3, 1)
    for broken, S in (([0, -4, 75, 115], None), ([0, 80, 75, 115], None), ([0, 65, 65, 999], None), ([0, 65, 65, 137], 100),
                      ([0, 1 << 40, 1 << 41, 1 << 42], None)):
        for draw in (0, 1):
            got = dev_rows(samples, broken, 3, 64, draw, CC.SEED, 0, z, 1, S=S)
            want = CR.rows(samples[:S], broken, 3, 64, draw, CC.SEED, 0, z, 1, S=S)
            for g, w in zip(got, want):
                same_bits(g, w, (broken, draw))
            assert (got[4] & ER.BAD_TABLE).any()
            for b in np.nonzero(got[4])[0]:
                assert not got[0][b * 64:(b + 1) * 64].any() and not got[1][b * 64:(b + 1) * 64].any() and not got[2][b * 64:(b + 1) * 64].any()


@pytest.mark.parametrize("case", CC.reduce_cases(), ids=lambda c: "B%d_k%d_L%d_s%d" % c)
def test_bound_reduce_kernel_equals_the_restatement(case):
    B, k, L, Js = case
    pred, lo, hi, J, flags = CC.reduce_case(*case)
    got = dev_reduce(pred, lo, hi, J, L, B, k, CC.CLAMP, flags)
    want = CR.reduce(pred, lo, hi, J, L, B, k, CC.CLAMP, flags)
    for g, w, n in zip(got, want, ("loss", "g_zn", "flags", "part")):
        same_bits(g, w, (case, n))
    exact = dev_reduce(pred, lo, lo, J, L, B, k, CC.CLAMP, flags)                    # lo == hi: the encoder's reduce, in every bit
    want = ER.reduce(pred, lo, J, L, B, k, CC.CLAMP, flags)
    for g, w, n in zip(exact, want, ("loss", "g_zn", "flags", "part")):
        same_bits(g, w, (case, "lo == hi", n))


def test_a_shapes_results_do_not_depend_on_the_batch_and_repeat():
    # the reduce
    B, k, L, Js = 5, 2049, 33, 40
    pred, lo, hi, J, flags = CC.reduce_case(B, k, L, Js)
    whole = dev_reduce(pred, lo, hi, J, L, B, k, CC.CLAMP, flags)
    again = dev_reduce(pred, lo, hi, J, L, B, k, CC.CLAMP, flags)
    for a, b in zip(whole, again):
        same_bits(a, b, "run twice")
    order = [3, 0, 4, 2, 1]
    idx = np.concatenate([np.arange(b * k, (b + 1) * k) for b in order])
    moved = dev_reduce(pred[idx], lo[idx], hi[idx], J[idx], L, B, k, CC.CLAMP, flags[order])
    for i, b in enumerate(order):
        sl = slice(b * k, (b + 1) * k)
        alone = dev_reduce(pred[sl], lo[sl], hi[sl], J[sl], L, 1, k, CC.CLAMP, flags[b:b + 1])
        for x in range(4):
            same_bits(whole[x][b], moved[x][i], ("moved", b, x))
            same_bits(whole[x][b], alone[x][0], ("alone", b, x))
    # the view: twice, shape 1 of three alone (its index given as shape0), and the shapes in another order (with their indices' hashes:
    # a shape's draws follow shape0 + b, so the moved run is compared slot by slot only where the index is kept -- shape 1 stays second)
    case = (3, (1, 257, 65), 64, "none", None)
    pts, ptoff, pose, origin, nrm = CC.view_case(*case)
    nrm = np.random.default_rng(0).standard_normal((len(pts), 3))
    P = 67
    whole = dev_view(pts, nrm, ptoff, pose, origin, 64, CC.ETA, CC.S_MAX, CC.SEED)
    again = dev_view(pts, nrm, ptoff, pose, origin, 64, CC.ETA, CC.S_MAX, CC.SEED)
    same_bits(whole[0], again[0], "view twice")
    alone = dev_view(pts[1:258], nrm[1:258], [0, 257], pose[1:2], origin, 64, CC.ETA, CC.S_MAX, CC.SEED, shape0=1)
    same_bits(whole[0][P:258 * P], alone[0], "view alone")
    idx = np.concatenate([np.arange(258, 323), np.arange(1, 258), np.arange(0, 1)])                       # shapes 2, 1, 0
    moved = dev_view(pts[idx], nrm[idx], [0, 65, 322, 323], pose[[2, 1, 0]], origin, 64, CC.ETA, CC.S_MAX, CC.SEED)
    same_bits(moved[0][65 * P:322 * P], whole[0][P:258 * P], "view moved, index kept")
    for b, lo_w, lo_m, n in ((0, 0, 322, 1), (2, 258, 0, 65)):                                              # shapes 0 and 2: at the other index
        there = dev_view(pts[lo_w:lo_w + n], nrm[lo_w:lo_w + n], [0, n], pose[b:b + 1], origin, 64, CC.ETA, CC.S_MAX, CC.SEED, shape0=2 - b)
        same_bits(moved[0][lo_m * P:(lo_m + n) * P], there[0], ("view moved", b))
    # the rows: alone, at another position (the shape's index passed as shape0) and twice, taking rows in order and drawing them
    samples, soff, z = CC.rows_case(5, (70, 0, 300, 65, 64), 64, 0, 33, 1)
    for draw in (0, 1):
        whole = dev_rows(samples, soff, 5, 64, draw, CC.SEED, 3, z, 1, shape0=4)
        alone = dev_rows(samples[soff[2]:soff[3]], [0, 300], 1, 64, draw, CC.SEED, 3, z[2:3], 1, shape0=6)
        for x in range(3):
            same_bits(whole[x][2 * 64:3 * 64], alone[x], ("rows alone", draw, x))
        moved = dev_rows(np.concatenate([samples[soff[3]:soff[4]], samples[soff[2]:soff[3]]]), [0, 65, 365], 2, 64, draw, CC.SEED, 3, z[[3, 2]], 1, shape0=5)
        for x in range(3):
            same_bits(whole[x][2 * 64:3 * 64], moved[x][64:], ("rows moved", draw, x))
        same_bits(dev_rows(samples, soff, 5, 64, draw, CC.SEED, 3, z, 1, shape0=4)[0], whole[0], ("rows twice", draw))


# ---- fit_many --------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("draw", [False, True])
@pytest.mark.parametrize("name", ["w128", "lat8", "asset", "ln", "f16"])
def test_fit_many_on_exact_rows_is_encode_many_in_every_bit(name, draw):
    dec = gpu_decoder(name)
    L, B, n = int(dec.latent_size), 3, 200
    rows, soff, z0 = shapes_of(L, B, n)
    samples = [SdfSamples(torch.from_numpy(rows[soff[b]:soff[b + 1]]).to(DEV)) for b in range(B)]
    kw = dict(iters=5, rows_per_iter=128 if draw else n, lr=5e-3, lr_step=3, clamp=0.5, init=torch.from_numpy(z0), seed=11, history=True, draw=draw)
    enc = E.encode_many(dec, samples, **kw)
    fit = C.fit_many(dec, [C.BoundSamples.from_sdf(s) for s in samples], **kw)
    for what in ("latents", "raw_latents", "loss", "flags", "history"):
        same_bits(getattr(fit, what).cpu().numpy(), getattr(enc, what).cpu().numpy(), (name, what))
    assert not enc.flags.any() and (enc.raw_latents.cpu().numpy() != z0).any()
    one = C.fit_many(dec, [C.BoundSamples.from_sdf(s) for s in samples], staging_bytes=1, **kw)       # staged one shape at a time
    same_bits(one.raw_latents.cpu().numpy(), enc.raw_latents.cpu().numpy(), "staged")


@pytest.mark.parametrize("name", ET.NAMES)
def test_ten_step_trajectory_on_mixed_rows_stays_within_the_calibrated_bound_of_the_float64_loop(name):
    """Measured values: profiles/complete_notes.md."""
    dec = gpu_decoder(name)
    samples, soff, z0, k = CC.fit_case(name, CC.TRAJECTORY_SEED[name], ET.B, ET.K)
    ref = CC.run(name, ET.decoder64(PC.net(name)), np.float64, samples, soff, z0, k, ET.STEPS, watch_margin=True, clamp=ET.CLAMPS[name], **ET.FIT)
    assert ref["margin"].min() > 1.0                                          # every row admitted: none within 100 fwd_tol of a kink
    sam = [C.BoundSamples(torch.from_numpy(np.array(samples[soff[b]:soff[b + 1]])).to(DEV)) for b in range(ET.B)]
    enc = C.fit_many(dec, sam, iters=ET.STEPS, rows_per_iter=k, init=torch.from_numpy(np.array(z0)), clamp=ET.CLAMPS[name], history=True, **ET.FIT)
    dev = float(np.abs(enc.raw_latents.cpu().numpy().astype(np.float64) - ref["z"]).max())
    dl = float(np.abs(enc.history.cpu().numpy().astype(np.float64) - ref["history"]).max())
    print("%s: device deviates %.3e from float64 after %d steps (bound %.3e); loss history %.3e" % (name, dev, ET.STEPS, CC.TRAJECTORY_BOUND[name], dl))
    assert not enc.flags.any()
    assert dev <= CC.TRAJECTORY_BOUND[name], (dev, CC.TRAJECTORY_BOUND[name])


def _params(yaw, trans, scale, latent):
    return {"yaw": torch.tensor([yaw], dtype=torch.float32), "trans": torch.tensor(trans, dtype=torch.float32),
            "scale": torch.tensor([scale], dtype=torch.float32), "latent": torch.as_tensor(latent, dtype=torch.float32).reshape(-1)}


def test_view_samples_many_equals_the_restatement_and_nothing_waits_for_the_host():
    case = (3, (65, 0, 1), 1, "holes", None)
    pts, ptoff, pose, origin, nrm = CC.view_case(*case)
    rng = np.random.default_rng(5)
    yaw = rng.uniform(-3, 3, 3).astype(np.float32)
    params = [_params(float(yaw[b]), pose[b, 2:5], float(pose[b, 5]), np.zeros(3)) for b in range(3)]
    pose = np.array(pose)
    pose[:, 0], pose[:, 1] = torch.cos(torch.from_numpy(yaw)).numpy(), torch.sin(torch.from_numpy(yaw)).numpy()      # as verify._pose_rows forms them
    clouds = [torch.from_numpy(np.array(pts[ptoff[b]:ptoff[b + 1]])).to(DEV) for b in range(3)]
    normals = [torch.from_numpy(np.array(nrm[ptoff[b]:ptoff[b + 1]])).to(DEV) for b in range(3)]
    kw = dict(origin=(0.5, -0.25, 0.125), free_rows=4, eta=0.02, s_max=0.4, seed=77)
    C.view_samples_many(params, clouds, normals, **kw)
    syncs, out = count_syncs(lambda: C.view_samples_many(params, clouds, normals, **kw))
    assert syncs == 0, syncs
    want, flags = CR.view_rows(pts, nrm, ptoff, pose, np.array(kw["origin"], np.float32), 4, 0.02, 0.4, 77)
    assert [len(s) for s in out] == [65 * 7, 0, 7] and all(s.rows.is_cuda for s in out)
    same_bits(np.concatenate([s.numpy() for s in out]), want)
    assert [int(s.flags) for s in out] == flags.tolist()
    none = C.view_samples_many(params, clouds, None, **kw)
    same_bits(np.concatenate([s.numpy() for s in none]), CR.view_rows(pts, None, ptoff, pose, np.array(kw["origin"], np.float32), 4, 0.02, 0.4, 77)[0])


def test_no_host_traffic_in_the_loop():
    dec = gpu_decoder("w128")
    rows, soff, z0 = shapes_of(3, 3, 200, seed=2)
    rng = np.random.default_rng(8)
    samples = [C.BoundSamples(torch.from_numpy(np.concatenate([rows[soff[b]:soff[b + 1]], rows[soff[b]:soff[b + 1], 3:] + rng.uniform(0, 0.1, (200, 1)).astype(np.float32)], 1)).to(DEV))
               for b in range(3)]
    init = torch.from_numpy(z0).to(DEV)
    C.fit_many(dec, samples, iters=2, rows_per_iter=64, init=init)                                   # the handle and the library are loaded
    syncs, enc = count_syncs(lambda: C.fit_many(dec, samples, iters=20, rows_per_iter=64, init=init, history=True))
    assert syncs == 0, syncs
    assert enc.loss.is_cuda and enc.flags.is_cuda and enc.history.is_cuda and enc.latents.is_cuda and tuple(enc.history.shape) == (20, 3)


# ---- end to end ----------------------------------------------------------------------------------------------------------------------------------

def test_completion_of_a_meshed_shape_from_its_camera_facing_side():
    """The case of tests/_complete_traj.py (built on the CPU: the asset decoder's shape meshed at R = 24, its camera-facing vertices, the
    start at the antipode of the true latent, the seed chosen with the float64 loop).  The loss falls, the completed latent explains the
    WHOLE shape's samples better than the start, and the last loss lies within a factor of two of the float64 run's.
    profiles/complete_notes.md has the measured values, and those of the same run without free-space rows."""
    dec = gpu_decoder("asset")
    c, case = CT.COMPLETION, CT.completion_case()
    ref = CT.completion_reference()
    assert ref["history"][-1] < ref["history"][0] and ref["residual_end"] < ref["residual_start"]
    z_true = torch.from_numpy(np.array(case["z_true"])).to(DEV)
    cloud, normals = np.array(case["cloud"]), np.array(case["normals"])
    params = _params(c["yaw"], c["trans"], c["scale"], -case["z_true"][0])            # the start: the antipodal latent
    full = SdfSamples(torch.from_numpy(np.array(case["full"])).to(DEV))
    start, _ = prior_residuals(dec, -z_true, full)
    fit = dict(iters=c["iters"], rows_per_iter=c["rows"], lr=c["lr"], lr_step=c["lr_step"], lr_factor=c["lr_factor"], clamp=c["clamp"], history=True)
    for free_rows in (c["free_rows"], 0):
        enc = C.complete_many(dec, [params], [cloud], normals=[normals], free_rows=free_rows, eta=c["eta"], s_max=c["s_max"], seed=c["seed"], **fit)
        h = enc.history.cpu().numpy()[:, 0]
        end, _ = prior_residuals(dec, enc.latents, full)
        cos = float((torch.nn.functional.normalize(enc.latents.double(), dim=1) * z_true.double()).sum())
        print("completion (free_rows = %d, %d points, %d rows): loss %.4e -> %.4e; residual on the whole shape %.4e -> %.4e; cosine to the true latent %.4f"
              % (free_rows, len(cloud), len(enc.samples[0]), h[0], h[-1], float(start[0]), float(end[0]), cos))
        if free_rows:                                                              # (the run without free-space rows is recorded, not asserted)
            print("            float64: loss %.4e -> %.4e; residual %.4e -> %.4e; cosine %.4f"
                  % (ref["history"][0], ref["history"][-1], ref["residual_start"], ref["residual_end"], ref["cosine"]))
            assert int(enc.flags[0]) == 0 and int(enc.samples[0].flags) == 0
            assert len(enc.samples[0]) == len(case["rows%d" % free_rows])
            assert h[-1] < h[0], (h[0], h[-1])
            assert float(end[0]) < float(start[0]), (float(end[0]), float(start[0]))
            assert 0.5 * ref["history"][-1] <= h[-1] <= 2.0 * ref["history"][-1], (h[-1], ref["history"][-1])
    # normals=None: estimated on the cloud; a point with fewer than 3 neighbours gets a NaN normal and loses its two normal rows
    lone = np.concatenate([cloud[:50], [[40.0, 40.0, 40.0]]]).astype(np.float32)
    enc = C.complete_many(dec, [params], [lone], iters=2, rows_per_iter=64, free_rows=1)
    r = enc.samples[0].numpy().reshape(51, 4, 5)
    assert not np.isfinite(r[-1, :, 3]).any() and np.isfinite(r[:50, 1, 3]).all() == np.isfinite(r[:50, 0, 3]).all() and np.isfinite(r[:50, 1, 3]).any()
    assert tuple(enc.latents.shape) == (1, 3)


def _same(a, b, where):
    """a and b hold the same bits: tensors, arrays, scalars, None, and lists / tuples / dicts / plain objects of them, recursively"""
    assert type(a) is type(b), (where, type(a), type(b))
    if torch.is_tensor(a):
        assert a.dtype == b.dtype and a.shape == b.shape and a.device == b.device, where
        assert a.detach().cpu().contiguous().numpy().tobytes() == b.detach().cpu().contiguous().numpy().tobytes(), where
    elif isinstance(a, np.ndarray):
        assert a.dtype == b.dtype and a.shape == b.shape and (a.tobytes() == b.tobytes() if a.dtype != object else list(a) == list(b)), where
    elif isinstance(a, dict):
        assert list(a) == list(b), where
        for k in a:
            _same(a[k], b[k], where + (k,))
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), where
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, where + (i,))
    elif a is None or isinstance(a, (bool, int, str, bytes)):
        assert a == b, where
    elif isinstance(a, (float, np.floating)):
        assert np.float64(a).tobytes() == np.float64(b).tobytes(), where
    elif hasattr(a, "__dict__"):
        _same(vars(a), vars(b), where + (type(a).__name__,))
    else:
        assert a == b, where


def test_refine_frame_complete():
    import sdflabel_amd
    from sdflabel_amd.pipelines import optimizer as OP
    from sdflabel_amd.pipelines.frame import refine_frame
    from tests.test_gpu_frame import _synthetic_frame
    dec32 = sdflabel_amd.setup_dsdf(ASSET + ".pt", precision=torch.float32)[0].to(DEV)
    dec16 = sdflabel_amd.setup_dsdf(ASSET + ".pt", precision=torch.float16)[0].to(DEV)
    annos, K_orig, latents = _synthetic_frame(dec32, n=4)
    grid = sdflabel_amd.Grid3D(40, DEV)
    p_WC = np.eye(4)
    p_WC[:3, 3] = [0.1, -0.2, 0.3]
    W8 = {"2d": 0.3, "3d": 0.5}
    with pytest.raises(ValueError):
        refine_frame(annos, dec16, grid, latents, K_orig, p_WC, 3, W8, seed=7, complete=True)
    OP.clear_refiner_cache()
    est0, kept0, st0 = refine_frame(annos, dec16, grid, latents, K_orig, p_WC, 3, W8, seed=7, return_stages=True)
    OP.clear_refiner_cache()
    est, kept, st1 = refine_frame(annos, dec16, grid, latents, K_orig, p_WC, 3, W8, seed=7, return_stages=True,
                                  complete=dict(iters=10, rows_per_iter=256, history=True))
    assert kept == kept0 and len(kept) >= 2 and set(st1) == set(st0) | {"complete"}
    for k in est0:
        assert (est[k] == est0[k]) if k == "name" else (est[k].dtype == est0[k].dtype and est[k].tobytes() == est0[k].tobytes()), k
    for k in st0:                                                                 # every other stage, every label: the same bits
        _same(st0[k], st1[k], (k,))
    done = st1["complete"]
    assert set(done) == {"encoded", "cosine"}
    enc, cos = done["encoded"], done["cosine"]
    n = len(st1["params"])
    assert cos.is_cuda and cos.dtype == torch.float64 and tuple(cos.shape) == (n,) and tuple(enc.latents.shape) == (n, 3)
    assert tuple(enc.history.shape) == (10, n) and len(enc.samples) == n
    c = cos.cpu().numpy()
    print("refine_frame complete: cosines %s, flags %s, loss %s" % (c, enc.flags.cpu().numpy(), enc.loss.cpu().numpy()))
    assert np.isfinite(c).all() and (np.abs(c) <= 1 + 1e-12).all()
    assert n == len(kept0)                                                        # no label was dropped, so params follow kept
    assert [len(s) for s in enc.samples] == [7 * int(st1["lidar"][i][0].shape[0]) for i in kept0]
