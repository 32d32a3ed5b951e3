"""The float64 references of tests/_loss_ref.py against the reference project's recorded losses (golden G12), against the float32 oracle and
against torch.optim in float64; and the admission conditions of the inputs of tests/test_gpu_losses.py, asserted on the references alone, so
that no GPU test can hide a failure behind an ambiguous input.  Runs without a GPU."""
import numpy as np
import pytest
import torch

from oracle import sdf_oracle as O
from tests import _loss_cases as C
from tests._loss_ref import DELTA, loss_2d_ref, loss_3d_ref, match_rows, solver_ref
from tests._util import gold


@pytest.mark.parametrize("tag", ["a", "b"])
def test_references_reproduce_the_recorded_losses_G12(tag):
    """tolerances of test_gpu_configs.py::test_losses_vs_reference_G12"""
    z = gold("g12_losses.npz")
    for suffix, thr in (("", 1.0), ("_t03", 0.3)):
        r = loss_2d_ref(z[tag + "_color"], z[tag + "_target"], 5.0, thr)
        assert abs(r.loss - float(z[tag + "_l2d" + suffix])) < 2e-6, suffix
        assert np.abs(r.grad - z[tag + "_g_color" + suffix]).max() < 2e-6, suffix
    s = float(z[tag + "_scale"][0])
    r = loss_3d_ref(z[tag + "_xyzf"], z[tag + "_lidar"], s, 0.2)
    assert r.npairs == int(z[tag + "_n_pairs"])
    assert abs(r.loss - float(z[tag + "_l3d"])) < 1e-6
    assert np.abs(r.g_est - z[tag + "_g_xyzf"]).max() < 1e-6
    gs = float(z[tag + "_g_scale"][0])
    assert abs(r.g_scale - gs) < 1e-5 * max(1.0, abs(gs))


@pytest.mark.parametrize("diam", C.DIAMS)
def test_2d_reference_agrees_with_the_oracle_and_inputs_are_admissible(diam):
    """on every generated 2-D input of this diam (the 6x6 and 12x12 dense crops among them): reference and oracle give the same loss and, by
    the candidate rule, the same gradient; <= 1 % of the rendered pixels have more than one candidate; no minimum lies within DELTA of a
    threshold the input is used with."""
    for name, rend, tgt, dm, thresholds, one_sided in C.all_2d_inputs():
        if dm != diam:
            continue
        for thr in thresholds:
            r = loss_2d_ref(rend, tgt, diam, thr)
            lo, go = O.loss_2d(rend, tgt, diam=diam, threshold_nocs=thr, want_grad=True)
            assert (np.isnan(lo) and np.isnan(r.loss)) or abs(float(lo) - r.loss) <= 1e-5 * max(1.0, diam), (name, thr, float(lo), r.loss)
            err, _ = match_rows(go[:, r.ys, r.xs].T, r.rows)
            assert err.size == 0 or err.max() <= 1e-5, (name, thr, err.max())
            go[:, r.ys, r.xs] = 0
            assert not go.any(), name
            assert not (np.abs(r.mins - thr) <= DELTA).any(), (name, thr, "a minimum at the threshold")
        amb = sum(c.shape[0] > 1 for c in r.cands)
        assert amb <= 0.01 * len(r.cands), (name, amb, len(r.cands))
        if not one_sided and r.ys.size >= 200:
            assert 0.0 < (r.mins < 0.3).mean() < 1.0, (name, (r.mins < 0.3).mean())            # the 0.3 threshold cuts both ways


def test_3d_reference_agrees_with_the_oracle_and_inputs_are_admissible():
    """every generated cloud: reference and oracle agree; <= 1 % ambiguous rows; no nearest distance within DELTA of threshold / scale; 20 to
    80 % of the estimated points of the clouds of 1 000 points and more are paired."""
    for name, est, lid, scale in C.all_3d_inputs():
        r = loss_3d_ref(est, lid, scale, C.THRESHOLD_3D)
        lo, ge, gs, idx, close = O.loss_3d(est, lid, scale, threshold=C.THRESHOLD_3D, want_grad=True)
        assert abs(float(lo) - r.loss) <= 1e-5, (name, float(lo), r.loss)
        if est.shape[0] == 0 or lid.shape[0] == 0:
            assert r.npairs == -1
            continue
        assert int(close.sum()) == r.npairs, name
        err, pick = match_rows(ge, r.rows)
        assert err.max() <= 1e-5, (name, err.max())
        gs_ref = sum(g[p] for g, p in zip(r.gs_rows, pick))
        assert abs(float(gs) - gs_ref) <= 1e-5 * max(1.0, abs(gs_ref)), (name, float(gs), gs_ref)
        amb = sum(c.size > 1 for c in r.cand_idx)
        assert amb <= 0.01 * est.shape[0], (name, amb)
        assert not (np.abs(r.mins - r.thr) <= DELTA).any(), (name, "a nearest distance at the pairing threshold")
        if est.shape[0] >= 1000:
            assert 0.2 <= r.paired.mean() <= 0.8, (name, r.paired.mean())


@pytest.mark.parametrize("scale", C.TIE_SCALES)
def test_tie_lattice_spreads_its_ties_over_waves_and_tiles(scale):
    """the lattice input of the tie rule: 2, 4 or 8 lidar points tie exactly for every estimated point, and the shuffle puts tied points into
    different waves of one tile, into different tiles, and -- the case an index-blind merge gets wrong -- the lowest index into a HIGHER
    wave than another tied point's."""
    est, lidar, winner, tied = C.lattice_3d(scale)
    nl = lidar.shape[0]
    assert nl == 2197 and est.shape[0] == 3 * C.TIE_PER_KIND
    n = np.array([t.size for t in tied])
    assert sorted(set(n)) == [2, 4, 8] and all(int(w) == int(t.min()) for w, t in zip(winner, tied))
    slots = [[C.scan_slot(i, nl) for i in t] for t in tied]
    cross_tile = sum(len({s[0] for s in sl}) > 1 for sl in slots)
    cross_wave = sum(len({s[1] for s in sl}) > 1 for sl in slots)
    low_in_higher_wave = sum(C.scan_slot(t.min(), nl)[1] > min(s[1] for s in sl) for t, sl in zip(tied, slots))
    assert cross_tile > 1000 and cross_wave > 1000 and low_in_higher_wave > 300, (cross_tile, cross_wave, low_in_higher_wave)


def test_solver_reference_is_torch_optim_in_float64():
    """solver_ref against torch.optim.Adam (yaw, trans) + torch.optim.SGD (scale, latent) on float64 CPU tensors, one pair of optimizers per
    crop (a skipped crop takes no step), 200 steps, to 1e-12."""
    B, L = 6, 3
    p0, mag, seq = C.solver_inputs(B, L)
    p = p0.astype(np.float64)
    m, v, t = np.zeros((B, 4)), np.zeros((B, 4)), np.zeros(B, np.int64)
    tp, opts = [], []
    for b in range(B):
        q = [torch.tensor(p[b:b + 1]), torch.tensor(p[B + 3 * b:B + 3 * b + 3]), torch.tensor(p[4 * B + b:4 * B + b + 1]),
             torch.tensor(p[5 * B + b * L:5 * B + (b + 1) * L])]
        tp.append(q)
        opts.append((torch.optim.Adam([{"params": q[0], "lr": C.LR_ADAM}, {"params": q[1], "lr": C.LR_ADAM}], lr=0.03),
                     torch.optim.SGD([{"params": q[2], "lr": C.LR_SCALE}, {"params": q[3], "lr": C.LR_LATENT}], lr=0.01, momentum=0.0)))
    nskip = 0
    for g, l2, l3, npairs in seq:
        g = g.astype(np.float64)
        total, stepped = solver_ref(p, g, L, l2, l3, npairs, C.W2, C.W3, m, v, t, C.LR_ADAM, C.LR_SCALE, C.LR_LATENT)
        for b in range(B):
            tot = np.float32(C.W3) * l3[b] + np.float32(C.W2) * l2[b]
            skip = npairs[b] < 0 or np.isnan(tot) or tot == 0
            assert stepped[b] == (0 if skip else 1)
            nskip += int(skip)
            if skip:
                continue
            q = tp[b]
            q[0].grad = torch.tensor(g[b:b + 1]); q[1].grad = torch.tensor(g[B + 3 * b:B + 3 * b + 3])
            q[2].grad = torch.tensor(g[4 * B + b:4 * B + b + 1]); q[3].grad = torch.tensor(g[5 * B + b * L:5 * B + (b + 1) * L])
            opts[b][0].step(); opts[b][1].step()
        got = np.concatenate([np.concatenate([tp[b][k].numpy().reshape(-1) for b in range(B)]) for k in range(4)])
        assert np.abs(got - p).max() <= 1e-12 * max(1.0, np.abs(p).max())
    assert 0.1 * B * len(seq) < nskip < 0.4 * B * len(seq)
    for b in range(B):
        st = opts[b][0].state
        assert int(st[tp[b][0]]["step"]) == t[b]
        tm = np.concatenate([st[tp[b][0]]["exp_avg"].numpy(), st[tp[b][1]]["exp_avg"].numpy()])
        tv = np.concatenate([st[tp[b][0]]["exp_avg_sq"].numpy(), st[tp[b][1]]["exp_avg_sq"].numpy()])
        assert np.abs(tm - m[b]).max() <= 1e-12 * max(1.0, np.abs(m[b]).max()) and np.abs(tv - v[b]).max() <= 1e-12 * max(1.0, np.abs(v[b]).max())
