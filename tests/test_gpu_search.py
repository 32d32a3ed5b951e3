"""The search for a fit's start on the device (csrc/search.hip, sdflabel_amd/search.py): each kernel against the numpy restatement bit for
bit between guard words; with identity owners against the completion's and the alignment's own entry points, device against device; the
draws shared by the starts of a shape; batch independence; score_many staged start by start; no host traffic; search_many against the
restatement's ranking of the device's own decoder values; fit_many / complete_many with search= against the hand-written chain; and the
end-to-end case of tests/_search_traj.py.  Measured values: profiles/search_notes.md.
"""
import numpy as np
import pytest
import torch

from sdflabel_amd import _lib
from sdflabel_amd import complete as C
from sdflabel_amd import search as S
from sdflabel_amd.sdf_samples import SdfSamples, prior_residuals
from tests import _align_cases as AC
from tests import _align_ref as AR
from tests import _complete_ref as CR
from tests import _complete_traj as CT
from tests import _encode_ref as ER
from tests import _search_cases as SC
from tests import _search_ref as SR
from tests import _search_traj as ST
from tests.test_gpu_align import dev_reduce as dev_align_reduce, dev_rows as dev_align_rows
from tests.test_gpu_complete import _params, _same, dev_reduce as dev_bound_reduce, dev_rows as dev_bound_rows
from tests.test_gpu_encode import DEV, Guarded, count_syncs, gpu_decoder, same_bits, st

pytestmark = pytest.mark.gpu

ROWS_NAMES = ("inputs", "cam", "lo", "hi", "zn", "flags")


# ---- the kernels through the C ABI -----------------------------------------------------------------------------------------------------------

def dev_rows(samples, soff, B, own, k, draw, seed, it, z, unit, pose=None, want_cam=True, S=None, shape0=0):
    N, L = z.shape
    S = len(samples) if S is None else S
    sm = Guarded(np.asarray(samples, np.float32)[:S] if S else np.zeros((1, 5), np.float32))
    so, ow, zz = Guarded(np.asarray(soff, np.int64)), Guarded(np.asarray(own, np.int32)), Guarded(np.asarray(z, np.float32))
    ps = None if pose is None else Guarded(np.asarray(pose, np.float32))
    cam = Guarded(N * k * 3, torch.float32) if (pose is not None and want_cam) else None
    inputs, lo, hi, zn, flags = Guarded(N * k * (L + 3), torch.float32), Guarded(N * k, torch.float32), Guarded(N * k, torch.float32), \
        Guarded(N * L, torch.float32), Guarded(N, torch.int32)
    _lib.check(_lib.lib().sdfr_search_rows(sm.t.data_ptr(), S, so.t.data_ptr(), B, ow.t.data_ptr(), N, shape0, k, draw, seed, it, zz.t.data_ptr(), L, unit,
                                           ps.t.data_ptr() if ps else None, inputs.t.data_ptr(), cam.t.data_ptr() if cam else None, lo.t.data_ptr(),
                                           hi.t.data_ptr(), zn.t.data_ptr(), flags.t.data_ptr(), st()), "sdfr_search_rows")
    torch.cuda.synchronize()
    for g in (sm, so, ow, zz, inputs, lo, hi, zn, flags) + ((ps,) if ps else ()) + ((cam,) if cam else ()):
        assert g.intact()
    return inputs.numpy((N * k, L + 3)), (cam.numpy((N * k, 3)) if cam else np.zeros((N * k, 3), np.float32)), lo.numpy(), hi.numpy(), zn.numpy((N, L)), \
        flags.numpy()


def dev_reduce(pred, lo, hi, pose, N, k, clamp, flags):
    h = _lib.lib()
    nbytes = int(h.sdfr_search_ws_bytes(N, k))
    ch = (k + ER.CHUNK - 1) // ER.CHUNK
    assert nbytes == N * ch * 2 * 8
    p, a, e, fl = (Guarded(np.asarray(x)) for x in (pred, lo, hi, np.asarray(flags, np.int32).copy()))
    ps = None if pose is None else Guarded(np.asarray(pose, np.float32))
    ws, loss = Guarded(nbytes // 8, torch.float64), Guarded(N, torch.float64)
    _lib.check(h.sdfr_search_reduce(p.t.data_ptr(), a.t.data_ptr(), e.t.data_ptr(), ps.t.data_ptr() if ps else None, N, k, float(clamp), ws.t.data_ptr(),
                                    nbytes, loss.t.data_ptr(), fl.t.data_ptr(), st()), "sdfr_search_reduce")
    torch.cuda.synchronize()
    for x in (p, a, e, fl, ws, loss) + ((ps,) if ps else ()):
        assert x.intact()
    return loss.numpy(), fl.numpy(), ws.numpy((N, ch, 2))


def dev_select(loss, flags, coff, N, keep):
    """loss and flags hold exactly the words a correct walk may read, between guard words"""
    B = len(coff) - 1
    ls = Guarded(np.asarray(loss, np.float64) if len(loss) else np.zeros(1, np.float64))
    fl = Guarded(np.asarray(flags, np.int32) if len(flags) else np.zeros(1, np.int32))
    co = Guarded(np.asarray(coff, np.int64))
    order, count = Guarded(B * keep, torch.int32), Guarded(B, torch.int32)
    _lib.check(_lib.lib().sdfr_search_select(ls.t.data_ptr(), fl.t.data_ptr(), co.t.data_ptr(), B, N, keep, order.t.data_ptr(), count.t.data_ptr(), st()),
               "sdfr_search_select")
    torch.cuda.synchronize()
    for g in (ls, fl, co, order, count):
        assert g.intact()
    return order.numpy((B, keep)), count.numpy()


def _case_id(c):
    return "B%d_s%s_k%d_d%d_L%d_u%d_p%d_o%d" % (c[0], "-".join(map(str, c[2])), c[3], c[4], c[5], c[6], c[7], c[8])


@pytest.mark.parametrize("case", SC.rows_cases(), ids=_case_id)
def test_rows_kernel_equals_the_restatement(case):
    B, counts, starts, k, draw, L, unit, posed, bad = case
    samples, soff, own, z, pose = SC.rows_case(*case)
    want = SR.rows(samples, soff, B, own, k, draw, SC.SEED, 17, z, unit, pose, shape0=2)
    for want_cam in ((True, False) if posed else (True,)):
        got = dev_rows(samples, soff, B, own, k, draw, SC.SEED, 17, z, unit, pose, want_cam, shape0=2)
        for g, w, n in zip(got, want, ROWS_NAMES):
            if n != "cam" or (posed and want_cam):
                same_bits(g, w, (case, want_cam, n))
    if bad:
        for s in np.nonzero((own < 0) | (own >= B))[0]:
            assert got[5][s] == ER.BAD_TABLE and not got[0][s * k:(s + 1) * k].any()
    if posed:
        assert (got[5] == AR.BAD_POSE).sum() == 1 and np.isnan(got[2]).any()


@pytest.mark.parametrize("case", AC.rows_cases(), ids=lambda c: "B%d_k%d_d%d_L%d_u%d_bad%d" % (c[0], c[2], c[3], c[4], c[5], c[6]))
def test_rows_with_identity_owners_are_the_fits_rows_device_against_device(case):
    B, counts, k, draw, L, unit, bad_pose = case
    samples, soff, z, pose = AC.rows_case(*case)
    own = np.arange(B, dtype=np.int32)
    got = dev_rows(samples, soff, B, own, k, draw, SC.SEED, 17, z, unit, pose, shape0=2)
    want = dev_align_rows(samples, soff, B, k, draw, SC.SEED, 17, z, unit, pose, shape0=2)
    for g, w, n in zip(got, want, ROWS_NAMES):
        same_bits(g, w, (case, "posed", n))
    got = dev_rows(samples, soff, B, own, k, draw, SC.SEED, 17, z, unit, None, shape0=2)
    i, lo, hi, zn, fl = dev_bound_rows(samples, soff, B, k, draw, SC.SEED, 17, z, unit, shape0=2)
    for g, w, n in zip((got[0],) + got[2:], (i, lo, hi, zn, fl), ("inputs", "lo", "hi", "zn", "flags")):
        same_bits(g, w, (case, "unposed", n))


def test_broken_sample_tables_are_flagged_not_faults():
    samples, soff, own, z, pose = SC.rows_case(3, (65, 0, 72), (3, 1, 2), 65, 0, 8, 0, False, False)
    for broken, Sn in AC.BROKEN_SOFF:
        for draw in (0, 1):
            got = dev_rows(samples, broken, 3, own, 64, draw, SC.SEED, 0, z, 1, None, S=Sn)            # guard words checked inside
            want = SR.rows(samples[:Sn], broken, 3, own, 64, draw, SC.SEED, 0, z, 1, None, S=Sn)
            for g, w in zip(got, want):
                same_bits(g, w, (broken, draw))
            assert (got[5] & ER.BAD_TABLE).any()


@pytest.mark.parametrize("case", SC.reduce_cases(), ids=lambda c: "N%d_k%d_p%d_bad%d" % c)
def test_reduce_kernel_equals_the_restatement_and_the_fits_loss_word(case):
    N, k, posed, bad_pose = case
    pred, lo, hi, pose, flags, J, cam = SC.reduce_case(*case)
    got = dev_reduce(pred, lo, hi, pose, N, k, SC.CLAMP[posed], flags)
    want = SR.reduce(pred, lo, hi, pose, N, k, SC.CLAMP[posed], flags)
    for g, w, n in zip(got, want, ("loss", "flags", "part")):
        same_bits(g, w, (case, n))
    if posed:
        fit = dev_align_reduce(pred, lo, hi, J, cam, pose, 3, N, k, SC.CLAMP[posed], flags)
    else:
        fit = dev_bound_reduce(pred, lo, hi, J, 3, N, k, SC.CLAMP[posed], flags)
    same_bits(got[0], fit[0], (case, "the loss word of the fit's reduce")); same_bits(got[1], fit[2], (case, "flags"))
    same_bits(got[2], fit[3][:, :, -2:], (case, "the partial sums of loss and count"))


@pytest.mark.parametrize("name", ["asset", "f16"])
@pytest.mark.parametrize("k", [1025, 2049])
def test_loss_on_the_decoders_own_values_is_the_fits_loss_word(name, k):
    """two and three chunks, float32 and float16 decoders: rows -> the decoder -> both reduces, device against device"""
    from tests.test_gpu_encode import device_pred_and_J
    dec = gpu_decoder(name)
    B, L = 3, 3
    samples, soff, z, pose = AC.rows_case(B, (2 * k + 3, 0, 70), k, 1, L, 1, -1)
    own = np.arange(B, dtype=np.int32)
    for ps in (None, pose):
        inputs, cam, lo, hi, zn, flags = dev_rows(samples, soff, B, own, k, 1, SC.SEED, 0, z, 1, ps)
        pred, J = device_pred_and_J(dec, inputs)
        clamp = SC.CLAMP[ps is not None]
        got = dev_reduce(pred, lo, hi, ps, B, k, clamp, flags)
        fit = dev_bound_reduce(pred, lo, hi, J, L, B, k, clamp, flags) if ps is None else dev_align_reduce(pred, lo, hi, J, cam, ps, L, B, k, clamp, flags)
        same_bits(got[0], fit[0], (name, k, "loss")); same_bits(got[1], fit[2], (name, k, "flags"))
        assert got[0][0] > 0 and got[1].tolist() == [0, ER.EMPTY, 0]          # (the zero rows of an empty shape count: p finite, lo == hi == 0)


def test_starts_of_one_shape_share_their_draw_and_shapes_do_not():
    B, counts, starts, k, draw, L, unit, posed, bad = case = (3, (133, 0, 70), (2, 1, 3), 65, 1, 3, 1, True, True)
    samples, soff, own, z, pose = SC.rows_case(*case)
    inputs, cam, lo, hi, zn, flags = dev_rows(samples, soff, B, own, k, draw, SC.SEED, 0, z, unit, pose)
    a, b = [s for s in range(len(own)) if own[s] == 0][:2]
    A, Bs = slice(a * k, (a + 1) * k), slice(b * k, (b + 1) * k)
    assert np.array_equal(pose[a], pose[b]) and not flags[a] and not flags[b]
    same_bits(cam[A], cam[Bs]); same_bits(lo[A], lo[Bs]); same_bits(hi[A], hi[Bs]); same_bits(inputs[A, L:], inputs[Bs, L:], "equal poses: equal xyz")
    assert not np.array_equal(inputs[A, :L], inputs[Bs, :L])
    two = np.concatenate([samples[:70], samples[:70]])
    i2, _, lo2, hi2, _, _ = dev_rows(two, [0, 70, 140], 2, [0, 0, 1], k, 1, SC.SEED, 0, z[:3], unit)
    same_bits(lo2[:k], lo2[k:2 * k]); same_bits(hi2[:k], hi2[k:2 * k]); same_bits(i2[:k, L:], i2[k:2 * k, L:])
    assert not np.array_equal(i2[:k, L:], i2[2 * k:, L:])                              # two shapes with equal samples draw differently


# ---- the select --------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(SC.select_cases()))
def test_select_kernel_equals_the_restatement_and_a_stable_sort(name):
    loss, flags, coff, N, keep = SC.select_cases()[name]
    got = dev_select(loss, flags, coff, N, keep)
    for want in (SR.select(loss, flags, coff, N, keep), SR.select_lexsort(loss, flags, coff, N, keep)):
        same_bits(got[0], want[0], (name, "order")); same_bits(got[1], want[1], (name, "count"))
    again = dev_select(loss, flags, coff, N, keep)
    same_bits(got[0], again[0], "twice")


def test_broken_start_tables_are_flagged_not_faults():
    for loss, flags, coff, N, keep in SC.broken_select_cases():
        got = dev_select(loss, flags, coff, N, keep)                                  # guard words checked inside
        want = SR.select(loss, flags, coff, N, keep)
        same_bits(got[0], want[0], (coff.tolist(), "order")); same_bits(got[1], want[1], (coff.tolist(), "count"))


# ---- batch independence ------------------------------------------------------------------------------------------------------------------------

def test_a_starts_results_do_not_depend_on_the_batch_and_repeat():
    B, counts, starts, k, draw, L, unit, posed, bad = case = (3, (2 * 1025 + 3, 0, 70), (2, 1, 3), 1025, 1, 3, 1, True, True)
    samples, soff, own, z, pose = SC.rows_case(*case)
    whole = dev_rows(samples, soff, B, own, k, draw, SC.SEED, 3, z, unit, pose, shape0=4)
    again = dev_rows(samples, soff, B, own, k, draw, SC.SEED, 3, z, unit, pose, shape0=4)
    for a, b in zip(whole, again):
        same_bits(a, b, "rows twice")
    perm = np.arange(len(own))[::-1].copy()
    moved = dev_rows(samples, soff, B, own[perm], k, draw, SC.SEED, 3, z[perm], unit, pose[perm], shape0=4)
    per_start = {"inputs": k, "cam": k, "lo": k, "hi": k, "zn": 1, "flags": 1}
    for i, s in enumerate(perm):
        alone = dev_rows(samples, soff, B, own[s:s + 1], k, draw, SC.SEED, 3, z[s:s + 1], unit, pose[s:s + 1], shape0=4)
        for x, n in enumerate(ROWS_NAMES):
            m = per_start[n]
            same_bits(whole[x][s * m:(s + 1) * m], moved[x][i * m:(i + 1) * m], ("moved", s, n))
            same_bits(whole[x][s * m:(s + 1) * m], alone[x], ("alone", s, n))
    N, kk = 5, 2049
    pred, lo, hi, _, flags, _, _ = SC.reduce_case(N, kk, False, -1)
    whole = dev_reduce(pred, lo, hi, None, N, kk, 0.1, flags)
    for a, b in zip(whole, dev_reduce(pred, lo, hi, None, N, kk, 0.1, flags)):
        same_bits(a, b, "reduce twice")
    order = [3, 0, 4, 2, 1]
    idx = np.concatenate([np.arange(b * kk, (b + 1) * kk) for b in order])
    moved = dev_reduce(pred[idx], lo[idx], hi[idx], None, N, kk, 0.1, flags[order])
    for i, b in enumerate(order):
        sl = slice(b * kk, (b + 1) * kk)
        alone = dev_reduce(pred[sl], lo[sl], hi[sl], None, 1, kk, 0.1, flags[b:b + 1])
        for x in range(3):
            same_bits(whole[x][b], moved[x][i], ("reduce moved", b, x)); same_bits(whole[x][b], alone[x][0], ("reduce alone", b, x))
    # the select: a shape alone, and elsewhere in the batch (its indices move with its first start)
    loss, fl, coff, Nn, keep = SC.select_cases()["uneven"]
    whole = dev_select(loss, fl, coff, Nn, keep)
    for b in range(len(coff) - 1):
        a, e = int(coff[b]), int(coff[b + 1])
        alone = dev_select(loss[a:e], fl[a:e], [0, e - a], e - a, keep)
        same_bits(np.where(whole[0][b] >= 0, whole[0][b] - a, -1).astype(np.int32), alone[0][0], ("select alone", b))
        assert whole[1][b] == alone[1][0]


# ---- score_many, search_many, choose -------------------------------------------------------------------------------------------------------------

def _view_samples(B, n, seed=3):
    """B shapes of n lattice-frame interval rows on the device, and the same as one array"""
    rng = np.random.default_rng(900 + seed)
    rows = np.concatenate([rng.uniform(-1, 1, (B * n, 3)), rng.uniform(-0.12, 0.12, (B * n, 1))], 1).astype(np.float32)
    rows = np.concatenate([rows, rows[:, 3:] + np.where(np.arange(B * n) % 3 == 0, 0, rng.uniform(0, 0.1, B * n)).astype(np.float32)[:, None]], 1)
    rows[5::17, 3:] = np.nan
    return [C.BoundSamples(torch.from_numpy(rows[b * n:(b + 1) * n]).to(DEV)) for b in range(B)], rows, np.arange(B + 1, dtype=np.int64) * n


def _device_pred(dec, inputs):
    handle, fwd, _ = S._decoder_mode(dec, torch.device(DEV, torch.cuda.current_device()))
    x = torch.from_numpy(np.array(inputs)).to(DEV)
    pred = torch.empty((x.shape[0],), device=DEV)
    _lib.check(fwd(handle.h, x.data_ptr(), x.shape[0], pred.data_ptr(), None, st()), "forward")
    return pred.cpu().numpy()


@pytest.mark.parametrize("name", ["asset", "lat8", "f16", "ln"])
def test_search_many_ranks_as_the_restatement_ranks_the_devices_own_values(name):
    dec = gpu_decoder(name)
    L, B, n, Cn, k, keep = int(dec.latent_size), 3, 300, 7, 128, 3
    samples, rows, soff = _view_samples(B, n)
    samples[1] = C.BoundSamples(samples[1].rows[:0])                                   # an empty shape: no usable start
    soff = np.array([0, n, n, 2 * n], np.int64)
    rows = np.concatenate([rows[:n], rows[2 * n:]])
    codes = S.sphere_codes(L, Cn, seed=5)
    found = S.search_many(dec, samples, codes, keep=keep, rows=k, clamp=0.1, seed=11)
    own = np.repeat(np.arange(B, dtype=np.int32), Cn)
    z = np.tile(codes.numpy(), (B, 1))
    inputs, _, lo, hi, zn, flags = SR.rows(rows, soff, B, own, k, True, 11, 0, z, True)
    loss, flags, _ = SR.reduce(_device_pred(dec, inputs), lo, hi, None, B * Cn, k, 0.1, flags)
    same_bits(found.scores.loss.cpu().numpy(), loss, (name, "loss")); same_bits(found.scores.flags.cpu().numpy(), flags, (name, "flags"))
    same_bits(found.scores.zn.cpu().numpy(), zn, (name, "zn"))
    order, count = SR.select(loss, flags, np.arange(B + 1, dtype=np.int64) * Cn, B * Cn, keep)
    same_bits(found.order.cpu().numpy(), order, (name, "order")); same_bits(found.count.cpu().numpy(), count, (name, "count"))
    assert count.tolist() == [keep, 0, keep]
    got_loss, got_lat = found.loss.cpu().numpy(), found.latents.cpu().numpy()
    for b in (0, 2):
        same_bits(got_loss[b], loss[order[b]], (name, b)); same_bits(got_lat[b], z[order[b]], (name, b))
    assert np.isnan(got_loss[1]).all() and not found.valid[1].any() and found.valid[0].all()


def test_score_many_staged_one_start_at_a_time_posed_and_unposed_and_nothing_waits_for_the_host():
    dec = gpu_decoder("asset")
    B, n, k = 2, 200, 96
    samples, rows, soff = _view_samples(B, n, seed=4)
    rng = np.random.default_rng(1)
    own = torch.tensor([1, 0, 0, 1, 1], dtype=torch.int32)
    z = torch.from_numpy(rng.standard_normal((5, 3)).astype(np.float32)).to(DEV)
    theta = torch.tensor([[0.1 * i, 0.01 * i, 0.0, 0.02, 1.0 + 0.05 * i] for i in range(5)])
    poses = S.pose_rows(theta).to(DEV)
    for ps, clamp in ((None, 0.1), (poses, 0.2)):
        kw = dict(poses=ps, rows=k, clamp=clamp, seed=5, draw=True)
        S.score_many(dec, samples, z, own, **kw)
        syncs, one = count_syncs(lambda: S.score_many(dec, samples, z, own, **kw))
        assert syncs == 0, syncs
        each = S.score_many(dec, samples, z, own, staging_bytes=1, **kw)
        again = S.score_many(dec, samples, z, own, **kw)
        for what in ("loss", "flags", "zn"):
            same_bits(getattr(one, what).cpu().numpy(), getattr(each, what).cpu().numpy(), ("staged", what))
            same_bits(getattr(one, what).cpu().numpy(), getattr(again, what).cpu().numpy(), ("twice", what))
        inputs, _, lo, hi, zn, flags = SR.rows(rows, soff, B, own.numpy(), k, True, 5, 0, z.cpu().numpy(), True, None if ps is None else ps.cpu().numpy())
        loss, flags, _ = SR.reduce(_device_pred(dec, inputs), lo, hi, None if ps is None else ps.cpu().numpy(), 5, k, clamp, flags)
        same_bits(one.loss.cpu().numpy(), loss, "loss"); same_bits(one.flags.cpu().numpy(), flags, "flags")
        assert one.loss.is_cuda and one.flags.is_cuda and not flags.any() and (loss > 0).all()
    codes = S.sphere_codes(3, 6).to(DEV)
    S.search_many(dec, samples, codes, keep=2, rows=k)
    syncs, found = count_syncs(lambda: S.search_many(dec, samples, codes, keep=2, rows=k))
    assert syncs == 0 and found.order.is_cuda and found.latents.is_cuda and tuple(found.latents.shape) == (2, 2, 3)
    loss = torch.tensor([[0.5, np.nan, 0.25], [0.25, 0.25, 0.1], [np.nan, np.inf, 0.3], [0.1, 0.2, 0.3]], dtype=torch.float64, device=DEV)
    flags = torch.tensor([[0, 0, 0], [0, 4, 2], [0, 0, 16], [1, 8, 2]], dtype=torch.int32, device=DEV)
    S.choose(loss, flags)
    syncs, pick = count_syncs(lambda: S.choose(loss, flags))
    assert syncs == 0 and pick.dtype == torch.int64 and pick.cpu().tolist() == [2, 0, -1, -1]


# ---- fit_many and complete_many with search= ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["asset", "f16"])
def test_fit_many_with_a_search_is_the_hand_written_chain_and_without_one_unchanged(name):
    dec = gpu_decoder(name)
    B, n, keep = 2, 300, 3
    samples, _, _ = _view_samples(B, n, seed=6)
    codes = S.sphere_codes(3, 8)
    kw = dict(iters=6, rows_per_iter=128, lr=5e-3, lr_step=4, clamp=0.1, seed=9, history=True)
    enc = C.fit_many(dec, samples, search=dict(codes=codes, keep=keep, rows=96), **kw)
    found = S.search_many(dec, samples, codes, keep=keep, rows=96, clamp=0.1, unit_latents=True, seed=9)
    fits = C.fit_many(dec, [samples[b] for b in range(B) for _ in range(keep)], init=found.latents.reshape(B * keep, 3), **kw)
    chosen = S.choose(fits.loss.reshape(B, keep), fits.flags.reshape(B, keep))
    at = (torch.arange(B, device=DEV) * keep + chosen).cpu().numpy()
    assert found.valid.all() and (chosen >= 0).all()
    _same(enc.chosen, chosen, ("chosen",)); _same(enc.found.order, found.order, ("order",)); _same(enc.found.loss, found.loss, ("found loss",))
    for what in ("latents", "raw_latents", "loss", "flags"):
        same_bits(getattr(enc, what).cpu().numpy(), getattr(fits, what).cpu().numpy()[at], (name, what))
        same_bits(getattr(enc.fits, what).cpu().numpy(), getattr(fits, what).cpu().numpy(), (name, "fits", what))
    same_bits(enc.history.cpu().numpy(), fits.history.cpu().numpy()[:, at], (name, "history"))
    assert (enc.loss.cpu().numpy() == fits.loss.cpu().numpy().reshape(B, keep).min(1)).all()
    # search=None: the unchanged call, in every bit
    init = torch.from_numpy(np.random.default_rng(2).standard_normal((B, 3)).astype(np.float32))
    a, b = C.fit_many(dec, samples, init=init, search=None, **kw), C.fit_many(dec, samples, init=init, **kw)
    for what in ("latents", "raw_latents", "loss", "flags", "history"):
        same_bits(getattr(a, what).cpu().numpy(), getattr(b, what).cpu().numpy(), (name, "search=None", what))
    assert a.found is None and a.chosen is None
    C.fit_many(dec, samples, search=dict(codes=codes, keep=keep, rows=96), **kw)
    on_dev = codes.to(DEV)                                                           # (a codebook on the host is uploaded through pinned memory)
    syncs, _ = count_syncs(lambda: C.fit_many(dec, samples, search=dict(codes=on_dev, keep=keep, rows=96), **kw))
    assert syncs == 0, syncs


def test_complete_many_with_a_search_is_the_hand_written_chain_and_without_one_unchanged():
    dec = gpu_decoder("asset")
    c, case = CT.COMPLETION, CT.completion_case()
    cloud, normals = np.array(case["cloud"][:400]), np.array(case["normals"][:400])
    params = [_params(c["yaw"], c["trans"], c["scale"], -case["z_true"][0])]
    codes = S.sphere_codes(3, 8)
    kw = dict(free_rows=2, eta=c["eta"], s_max=c["s_max"], seed=4, iters=5, rows_per_iter=256, lr=c["lr"], clamp=c["clamp"])
    enc = C.complete_many(dec, params, [cloud], normals=[normals], search=dict(codes=codes, keep=2), **kw)
    samples = C.view_samples_many(params, [cloud], [normals], free_rows=2, eta=c["eta"], s_max=c["s_max"], seed=4)
    hand = C.fit_many(dec, samples, iters=5, rows_per_iter=256, lr=c["lr"], clamp=c["clamp"], seed=4, search=dict(codes=codes, keep=2))
    for what in ("latents", "raw_latents", "loss", "flags", "chosen"):
        _same(getattr(enc, what), getattr(hand, what), (what,))
    same_bits(enc.samples[0].numpy(), samples[0].numpy(), "samples")
    assert tuple(enc.found.latents.shape) == (1, 2, 3) and int(enc.found.count[0]) == 2
    a = C.complete_many(dec, params, [cloud], normals=[normals], search=None, **kw)
    b = C.complete_many(dec, params, [cloud], normals=[normals], **kw)
    for what in ("latents", "raw_latents", "loss", "flags"):
        _same(getattr(a, what), getattr(b, what), ("search=None", what))


# ---- search_poses, align_many and label_scan with search= ------------------------------------------------------------------------------------

def _align_scene(B=2, n=250):
    """B clouds of the completion fixture's camera-facing points (strided subsets), their normals, and rough boxes off in yaw and trans"""
    from tests.test_gpu_align import _params as align_params
    c, case = CT.COMPLETION, CT.completion_case()
    cloud, normals = np.array(case["cloud"]), np.array(case["normals"])
    clouds = [cloud[b::7][:n].copy() for b in range(B)]
    nrms = [normals[b::7][:n].copy() for b in range(B)]
    params = [align_params([c["yaw"] + 0.2 - 0.3 * b, c["trans"][0] + 0.02, c["trans"][1], c["trans"][2] - 0.03 * b, c["scale"]], np.zeros(3)) for b in range(B)]
    return params, clouds, nrms, case


def test_search_poses_scores_codes_times_yaws_on_the_rows_of_align_samples_many():
    """posed scoring through the public path on align_samples_many's rows: every start's loss is the restatement's on the device's own
    decoder values, and -- device against device -- the loss word sdfr_align_reduce gives for the same start in align_many's first iteration"""
    from sdflabel_amd import align as A
    from tests.test_gpu_encode import device_pred_and_J
    dec = gpu_decoder("asset")
    params, clouds, nrms, case = _align_scene()
    B, k, keep = 2, 256, 3
    codes = torch.cat([torch.from_numpy(np.array(case["z_true"])), S.sphere_codes(3, 3)])            # C = 4
    yaws = S.yaw_offsets(4)
    kw = dict(normals=nrms, free_rows=2, eta=0.02, s_max=1.0, seed=6)
    S.search_poses(dec, params, clouds, codes, yaws=yaws, keep=keep, rows=k, clamp=0.2, **kw)
    syncs, found = count_syncs(lambda: S.search_poses(dec, params, clouds, codes, yaws=yaws, keep=keep, rows=k, clamp=0.2, **kw))
    assert syncs == 0, syncs
    samples = A.align_samples_many(clouds, nrms, free_rows=2, eta=0.02, s_max=1.0, seed=6)
    for a, b in zip(found.samples, samples):
        same_bits(a.numpy(), b.numpy(), "samples")
    Cn, H = 4, 4
    N = B * Cn * H
    base = np.stack([np.concatenate([p["yaw"].cpu().numpy(), p["trans"].cpu().numpy(), p["scale"].cpu().numpy()]) for p in params]).astype(np.float32)
    theta = np.repeat(base, Cn * H, 0)
    theta[:, 0] = (theta[:, 0] + np.tile(yaws.numpy(), B * Cn)).astype(np.float32)
    z = np.tile(np.repeat(codes.numpy(), H, 0), (B, 1))
    own = np.repeat(np.arange(B, dtype=np.int32), Cn * H)
    pose = AR.pose_row(theta)
    rows = np.concatenate([s.numpy() for s in samples])
    soff = np.concatenate([[0], np.cumsum([len(s) for s in samples])]).astype(np.int64)
    inputs, cam, lo, hi, zn, flags = SR.rows(rows, soff, B, own, k, True, 6, 0, z, True, pose)
    pred, J = device_pred_and_J(dec, inputs)
    loss, flags, _ = SR.reduce(pred, lo, hi, pose, N, k, 0.2, flags)
    same_bits(found.scores.loss.cpu().numpy(), loss, "loss"); same_bits(found.scores.flags.cpu().numpy(), flags, "flags")
    fit = dev_align_reduce(pred, lo, hi, J, cam, pose, 3, N, k, 0.2, np.zeros(N, np.int32))
    same_bits(found.scores.loss.cpu().numpy(), fit[0], "the loss word of sdfr_align_reduce")
    order, count = SR.select(loss, flags, np.arange(B + 1, dtype=np.int64) * Cn * H, N, keep)
    same_bits(found.order.cpu().numpy(), order, "order"); assert count.tolist() == [keep] * B and not flags.any()
    same_bits(found.theta.cpu().numpy(), theta[order], "theta"); same_bits(found.latents.cpu().numpy(), z[order], "latents")
    assert len(found.params) == B and len(found.params[0]) == keep
    for b in range(B):
        for r in range(keep):
            p = found.params[b][r]
            same_bits(np.concatenate([p["yaw"].cpu().numpy(), p["trans"].cpu().numpy(), p["scale"].cpu().numpy()]), theta[order[b, r]], (b, r))
            same_bits(p["latent"].cpu().numpy(), z[order[b, r]], (b, r))


@pytest.mark.parametrize("name", ["asset", "f16"])
def test_align_many_with_a_search_is_the_hand_written_chain_and_without_one_unchanged(name):
    from sdflabel_amd import align as A
    dec = gpu_decoder(name)
    params, clouds, nrms, case = _align_scene()
    B, keep = 2, 2
    codes = torch.cat([torch.from_numpy(np.array(case["z_true"])), -torch.from_numpy(np.array(case["z_true"]))])
    view = dict(normals=nrms, free_rows=2, eta=0.02, s_max=1.0, seed=6)
    kw = dict(iters=6, rows_per_iter=256, lr_step=4, clamp=0.2, history=True)
    srch = dict(codes=codes, yaws=S.yaw_offsets(4), keep=keep, rows=128)
    out = A.align_many(dec, params, clouds, search=srch, **view, **kw)
    found = S.search_poses(dec, params, clouds, codes, yaws=S.yaw_offsets(4), keep=keep, rows=128, clamp=0.2, unit_latents=True, **view)
    fits = A.align_many(dec, [found.params[b][r] for b in range(B) for r in range(keep)], None, seed=6,
                        samples=[found.samples[b] for b in range(B) for _ in range(keep)], **kw)
    chosen = S.choose(fits.loss.reshape(B, keep), fits.flags.reshape(B, keep))
    at = (torch.arange(B, device=DEV) * keep + chosen).cpu().numpy()
    assert found.valid.all() and (chosen >= 0).all()
    _same(out.chosen, chosen, ("chosen",)); _same(out.found.order, found.order, ("order",)); _same(out.found.theta, found.theta, ("theta",))
    for what in ("latents", "raw_latents", "theta", "loss", "flags"):
        same_bits(getattr(out, what).cpu().numpy(), getattr(fits, what).cpu().numpy()[at], (name, what))
        same_bits(getattr(out.fits, what).cpu().numpy(), getattr(fits, what).cpu().numpy(), (name, "fits", what))
    same_bits(out.history.cpu().numpy(), fits.history.cpu().numpy()[:, at], (name, "history"))
    assert len(out.params) == B and (out.loss.cpu().numpy() == fits.loss.cpu().numpy().reshape(B, keep).min(1)).all()
    a, b = A.align_many(dec, params, clouds, search=None, **view, **kw), A.align_many(dec, params, clouds, **view, **kw)
    for what in ("latents", "raw_latents", "theta", "loss", "flags", "history"):
        same_bits(getattr(a, what).cpu().numpy(), getattr(b, what).cpu().numpy(), (name, "search=None", what))
    assert a.found is None and a.chosen is None
    dsrch = dict(srch, codes=codes.to(DEV), yaws=S.yaw_offsets(4).to(DEV))
    A.align_many(dec, params, clouds, search=dsrch, **view, **kw)
    syncs, _ = count_syncs(lambda: A.align_many(dec, params, clouds, search=dsrch, **view, **kw))
    assert syncs == 0, syncs


def _scan_scene():
    import sdflabel_amd
    from tests import _cluster_ref as CLR
    from tests import _normals_ref as NR
    sc, s = CLR.planted_scene(), CLR.SCENE
    P = sc["points"][sc["mask"] != 0]
    p_WC = np.eye(4)
    p_WC[:3, 3] = [0.1, -0.2, 0.3]
    ckw = dict(eps=s["eps"], min_points=s["min_points"], max_clusters=64, n_angles=s["n_angles"], scale=s["scale"], gates=s["gates"])
    return sc, torch.from_numpy(np.array(P)).to(DEV), NR.KITTI_K, NR.KITTI_WH, p_WC, ckw, sdflabel_amd.Grid3D(40, DEV)


def test_label_scan_with_a_search_is_the_hand_written_chain_and_tells_front_from_back():
    """The planted scene (three objects of the asset shape): with the true latent and its antipode as the codebook, four yaw offsets and
    keep = 2, label_scan equals align_many(search=) + labels_many written out by hand in every bit, makes the synchronisations its docstring
    states, and every object's chosen yaw lies within a quarter turn of the truth: front is told from back three times out of three.
    search=None is the unchanged call in every bit."""
    from sdflabel_amd import align as A
    from sdflabel_amd import cluster as CL
    from sdflabel_amd import frame as FR
    from sdflabel_amd.pipelines import scan
    sc, pts, K, (w, h), p_WC, ckw, grid = _scan_scene()
    dec = gpu_decoder("asset")
    z = torch.from_numpy(np.array(sc["z_true"])).reshape(1, -1)
    lat = z[0].to(DEV)
    akw = dict(iters=60, rows_per_iter=512, lr_step=40, seed=3)
    srch = dict(codes=torch.cat([z, -z]), yaws=S.yaw_offsets(4), keep=2, rows=512)
    props = CL.proposals(pts, None, latent=lat, **ckw)
    fits = A.align_many(dec, props.params, props.clouds, search=srch, **akw)              # (the chain first: it also creates the decoder's handle)
    syncs, (est, st) = count_syncs(lambda: scan.label_scan(dec, grid, pts, K, w, h, p_WC, lat, remove_road=False, cluster_kw=ckw, align_kw=akw, search=srch))
    A_ = len(st["proposals"])
    assert A_ == 3 and syncs == 2 + (A_ + 15) // 16, (A_, syncs)
    for what in ("theta", "latents", "loss", "flags", "chosen"):
        _same(getattr(st["fits"], what), getattr(fits, what), (what,))
    uv = scan.pinhole_extents(props, K).cpu().numpy()
    bboxes = [np.array([np.clip(r[0], 0, w), np.clip(r[2], 0, h), np.clip(r[1], 0, w), np.clip(r[3], 0, h)], np.float32) for r in uv]
    want = FR.frame_dict(FR.labels_many(dec, grid, fits.params, p_WC, bboxes))
    assert set(est) == set(want)
    for k in want:
        assert (list(est[k]) == list(want[k])) if k == "name" else (est[k].dtype == want[k].dtype and est[k].tobytes() == want[k].tobytes()), k
    assert st["chosen"].tolist() == fits.chosen.cpu().tolist() and len(st["second"]) == 0
    theta = fits.theta.cpu().numpy().astype(np.float64)
    label = st["proposals"].clusters.label.cpu().numpy()
    right = 0
    for a, info in enumerate(st["proposals"].info):
        who = int(np.unique(sc["owner"][sc["mask"] != 0][np.nonzero(label == info["cluster"])[0]])[0])
        y_true = sc["truth"][who][0]
        err = abs((theta[a, 0] - y_true + np.pi) % (2 * np.pi) - np.pi)
        print("object %d: yaw %.3f, truth %.3f, |error| %.3f rad, chosen rank %d, kept scores %s, final losses %s, cosine of the latent %.4f"
              % (who, theta[a, 0], y_true, err, int(fits.chosen[a]), fits.found.loss[a].cpu().numpy(), fits.fits.loss.cpu().numpy()[2 * a:2 * a + 2],
                 float((fits.latents[a].cpu() * z[0]).sum())))
        right += err < np.pi / 2
    assert right == 3, right
    a = scan.label_scan(dec, grid, pts, K, w, h, p_WC, lat, remove_road=False, cluster_kw=ckw, align_kw=akw, search=None)
    b = scan.label_scan(dec, grid, pts, K, w, h, p_WC, lat, remove_road=False, cluster_kw=ckw, align_kw=akw)
    for k in b[0]:
        assert (list(a[0][k]) == list(b[0][k])) if k == "name" else a[0][k].tobytes() == b[0][k].tobytes(), k
    assert torch.equal(a[1]["fits"].theta, b[1]["fits"].theta) and a[1]["second"].tolist() == b[1]["second"].tolist() and "chosen" not in a[1]


# ---- end to end ----------------------------------------------------------------------------------------------------------------------------------

def test_search_recovers_the_shape_the_antipodal_start_loses():
    """The case of tests/_search_traj.py: the completion fixture, 32 Fibonacci codes, keep = 3, the fixture's fit settings, against the recorded
    float64 run (tests/golden/search_traj.json, which tests/test_search_cpu.py recomputes).  The device keeps the three starts the float64
    run keeps, in its order, and chooses the start the float64 run chooses (seed 0, which the admission rule refuses for that choice as it
    refuses seeds 1 to 4: see _search_traj); the chosen fit's residual on the WHOLE shape lies below the antipodal run's and its cosine above the
    one-start run's.  profiles/search_notes.md has the measured values."""
    dec = gpu_decoder("asset")
    c, s, case, ref = CT.COMPLETION, ST.SEARCH, CT.completion_case(), ST.golden()
    assert ref["seed"] == s["seed"] and ref["gap34"] > ST.ADMIT * ref["tol_score"]
    z_true = torch.from_numpy(np.array(case["z_true"])).to(DEV)
    params = _params(c["yaw"], c["trans"], c["scale"], -case["z_true"][0])
    full = SdfSamples(torch.from_numpy(np.array(case["full"])).to(DEV))
    enc = C.complete_many(dec, [params], [np.array(case["cloud"])], normals=[np.array(case["normals"])], free_rows=c["free_rows"], eta=c["eta"],
                          s_max=c["s_max"], seed=s["seed"], iters=c["iters"], rows_per_iter=c["rows"], lr=c["lr"], lr_step=c["lr_step"],
                          lr_factor=c["lr_factor"], clamp=c["clamp"], search=dict(codes=S.sphere_codes(3, s["C"]), keep=s["keep"], rows=c["rows"]))
    end, _ = prior_residuals(dec, enc.latents, full)
    cos = float((torch.nn.functional.normalize(enc.latents.double(), dim=1) * z_true.double()).sum())
    order, chosen = enc.found.order.cpu().numpy()[0], int(enc.chosen[0])
    print("search: device kept %s (float64 %s), scores %s (float64 %s); final losses %s (float64 %s); chose rank %d (float64 %d, tie %s); "
          "residual %.4e (float64 %.4e, antipodal %.4e); cosine %.8f (float64 %.8f)"
          % (order.tolist(), ref["order"], enc.found.loss.cpu().numpy()[0].tolist(), ref["score_kept"], enc.fits.loss.cpu().numpy().tolist(), ref["final"],
             chosen, ref["chosen"], ref["tie"], float(end[0]), ref["residual"][ref["chosen"]], ref["antipodal_residual_end"], cos,
             ref["cosine"][ref["chosen"]]))
    assert order.tolist() == ref["order"]
    assert chosen == ref["chosen"], (chosen, ref["chosen"])
    assert float(end[0]) < ref["antipodal_residual_end"], (float(end[0]), ref["antipodal_residual_end"])
    assert cos > ST.BEST_ONE_START_COSINE, cos
