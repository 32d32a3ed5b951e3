"""tests/_surface_ref.py against independent sources, on the CPU: the oracle's band list and torch.nonzero, torch float64 autograd of
F.normalize and of the pose matrix, float64 autograd of the whole backward tail, and hand-written sequences of the plan and guard state
machines."""
import numpy as np
import torch
import torch.nn.functional as TF

from oracle import sdf_oracle as O
from tests import _surface_ref as R

F = np.float32


def _prev(B, G, cap, slot=True, over=True):
    return dict(idx=np.full((B, cap), -7, np.int32), cnt=np.full(B, -7, np.int32), slot=np.full((B, G), -7, np.int32) if slot else None,
                over=np.zeros(B, np.int32) if over else None)


def test_band_ref_is_the_oracles_and_torchs_index_list():
    rng = np.random.default_rng(0)
    for G, dens in ((1, 1.0), (257, 0.05), (3000, 0.3), (3000, 0.0)):
        sdf = rng.uniform(-0.03, 0.03, (2, G)).astype(F) / F(max(dens, 1e-3))
        r = R.band_ref(sdf, 0.03, None, None, _prev(2, G, G), G, 1)
        for b in range(2):
            _, _, _, idx, _ = O.get_surface_points(np.zeros((G, 3), F), sdf[b][:, None], np.ones((G, 3), F), 0.03)
            n = int(r["cnt"][b])
            assert n == idx.size and np.array_equal(r["idx"][b, :n], idx) and (r["idx"][b, n:] == -7).all()
            tn = torch.nonzero(torch.from_numpy(sdf[b]).abs() < 0.03)[:, 0].numpy()
            assert np.array_equal(r["idx"][b, :n], tn)
            inv = np.full(G, -1); inv[idx] = np.arange(n)
            assert np.array_equal(r["slot"][b], inv) and r["over"][b] == 0


def test_band_ref_cap_skip_extra_and_the_sticky_flag():
    sdf = np.array([[0.01, 0.5, -0.02, 0.029, np.nan, np.inf, 0.03, -0.0]] * 3, F)
    prev = _prev(3, 8, 2); prev["over"][:] = 4
    r = R.band_ref(sdf, 0.03, np.array([0.0, 0.0, -0.04], F), np.array([0, 1, 0]), prev, 2, 2)
    assert r["cnt"].tolist() == [4, -7, 0] and r["idx"].tolist() == [[0, 2], [-7, -7], [-7, -7]]
    assert r["slot"][0].tolist() == [0, -1, 1, -1, -1, -1, -1, -1] and (r["slot"][1] == -7).all() and (r["slot"][2] == -1).all()
    assert r["over"].tolist() == [6, 4, 4]
    r2 = R.band_ref(sdf, 0.03, None, None, r, 2, 1)                    # still overflowing, the other bit
    assert r2["over"].tolist() == [7, 5, 5]
    r3 = R.band_ref(sdf * F(100), 0.03, None, None, r2, 2, 1)          # fits again (only the zero row): nothing is cleared
    assert r3["cnt"].tolist() == [1, 1, 1] and r3["over"].tolist() == [7, 5, 5]


def test_candidate_band_ref_is_scatter_select_map():
    rng = np.random.default_rng(1)
    B, G, stride, cap = 2, 500, 128, 40
    grid = rng.uniform(0.2, 0.3, (B, G)).astype(F)                      # non-candidates: outside the band
    cidx = np.stack([np.sort(rng.choice(G, stride, replace=False)) for _ in range(B)]).astype(np.int32)
    ccnt = np.array([100, 300], np.int32)
    csdf = rng.uniform(-0.06, 0.06, (B, stride)).astype(F)
    prev = dict(idx=np.full((B, cap), -7, np.int32), pos=np.full((B, cap), -7, np.int32), cnt=np.full(B, -7, np.int32), over=np.zeros(B, np.int32))
    g1, o = R.candidate_band_ref(grid, csdf, cidx, stride, ccnt, 0.03, cap, prev)
    g2 = R.scatter_values_ref(grid, csdf, cidx, stride, ccnt)
    assert np.array_equal(g1, g2)
    bs = R.band_ref(g2, 0.03, None, None, _prev(B, G, cap, slot=False), cap, 1)
    cslot = np.full((B, G), -1, np.int32)
    for b in range(B):
        n = min(ccnt[b], stride); cslot[b, cidx[b, :n]] = np.arange(n)
    pos, vio = R.candidate_band_map_ref(bs["idx"], cap, bs["cnt"], cslot, stride, np.full((B, cap), -7, np.int32), np.zeros((B, 2), np.int32))
    assert np.array_equal(o["idx"], bs["idx"]) and np.array_equal(o["cnt"], bs["cnt"]) and np.array_equal(o["pos"], pos) and not vio.any()
    assert o["over"].tolist() == [bs["over"][0], bs["over"][1] | 2] and o["cnt"][1] > cap and bs["over"][1] == 1


def _autograd_params(yaw, trans, latent, g_pose, g_rows):
    ty = torch.tensor(yaw, dtype=torch.float64, requires_grad=True); tt = torch.tensor(trans, dtype=torch.float64, requires_grad=True)
    tl = torch.tensor(latent, dtype=torch.float64, requires_grad=True)
    rows = TF.normalize(tl, p=2, dim=1)
    poses = []
    for b in range(ty.shape[0]):
        c, s = torch.cos(ty[b]), torch.sin(ty[b]); z, o = c * 0, c * 0 + 1
        Rm = torch.stack((c, z, s, z, o, z, -s, z, c)).view(3, 3) * torch.tensor([[1.0], [-1.0], [1.0]], dtype=torch.float64)
        poses.append(torch.cat([torch.cat([Rm, tt[b].view(3, 1)], 1), torch.tensor([[0, 0, 0, 1.0]], dtype=torch.float64)], 0))
    pose = torch.stack(poses)
    ((pose * torch.tensor(g_pose, dtype=torch.float64)).sum() + (rows * torch.tensor(g_rows, dtype=torch.float64)).sum()).backward()
    return rows.detach().numpy(), pose.detach().numpy(), ty.grad.numpy(), tt.grad.numpy(), tl.grad.numpy()


def test_params_refs_against_float64_autograd():
    rng = np.random.default_rng(2)
    for L in (1, 3, 9, 256):
        B = 4
        yaw = rng.uniform(-2 * np.pi, 2 * np.pi, B); yaw[0] = 0.0
        trans = rng.standard_normal((B, 3)); latent = rng.standard_normal((B, L)); latent[1] = 0.0
        g_pose = rng.standard_normal((B, 4, 4)); g_rows = rng.standard_normal((B, L))
        rows, pose, gy, gt, gl = _autograd_params(yaw, trans, latent, g_pose, g_rows)
        latnorm, rrows, rpose = R.params_forward_ref(yaw, trans, latent)
        assert latnorm[1] == 1e-12 and (rrows[1] == 0).all()
        assert np.abs(rrows - rows).max() <= 1e-12 and np.abs(rpose - pose).max() <= 1e-12
        for b in range(B):                                             # the oracle's rotation with row 1 negated
            Ro = O.rot_from_yaw(yaw[b], np.float64); Ro[1] *= -1
            assert np.abs(rpose[b, :3, :3] - Ro).max() <= 1e-12 and np.array_equal(rpose[b, :3, 3], trans[b])
        ry, rt, rl, m = R.params_backward_ref(np.cos(yaw), np.sin(yaw), latent, latnorm, g_pose, g_rows)
        assert np.abs(ry - gy).max() <= 1e-12 * max(1.0, m["g_yaw"].max()) and np.array_equal(rt, gt)
        assert (np.abs(rl - gl) <= 1e-12 * np.maximum(1.0, m["g_latent"])).all()
        assert np.array_equal(rl[1], g_rows[1] / 1e-12)                # the clamp holds: the gradient of latent / 1e-12


def test_tail_ref_against_float64_autograd_of_the_composition():
    rng = np.random.default_rng(3)
    n, L = 300, 3
    f = lambda *s: rng.standard_normal(s).astype(F)
    pts, g_pc, g_nc, g_col, g_xf, J = f(n, 3), f(n, 3), f(n, 3), f(n, 3), f(n, 3), f(n, L)
    nrm = f(n, 3); nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    fslot = np.full(n, -1, np.int64); front = rng.random(n) < 0.5; fslot[front] = np.arange(front.sum())
    yaw, trans, latent = F(0.7), f(3), f(L)
    for mode in (1, 2, 5, 6):
        ty = torch.tensor(float(yaw), dtype=torch.float64, requires_grad=True); tt = torch.tensor(trans, dtype=torch.float64, requires_grad=True)
        tl = torch.tensor(latent, dtype=torch.float64, requires_grad=True)
        D = lambda a: torch.tensor(a, dtype=torch.float64)
        z = TF.normalize(tl, p=2, dim=0)
        sdf = D(J) @ z                                                  # a decoder that is linear in the latent rows: d sdf / d z = J
        p = D(pts) - (sdf - sdf.detach())[:, None] * D(nrm)             # grid.py:61 around the band points, n_hat a constant
        c, s = torch.cos(ty), torch.sin(ty); zz = c * 0
        Rm = torch.stack((c, zz, s, zz, zz - 1, zz, -s, zz, c)).view(3, 3)
        pc = p @ Rm.T + tt[None]; nc = D(nrm) @ Rm.T
        col = p * D([1.0 if (mode & 3) == 2 else -1.0, 1.0, 1.0])[None]
        if mode & 4:
            col = (col + 1) * 0.5
        loss = (pc * D(g_pc)).sum() + (nc * D(g_nc)).sum() + (col * D(g_col)).sum() + (pc[torch.tensor(np.nonzero(front)[0])] * D(g_xf[:front.sum()])).sum()
        loss.backward()
        pose = np.eye(4); pose[:3, :3] = Rm.detach().numpy(); pose[:3, 3] = trans
        # (the reference takes the float32 pose the kernel reads: evaluate it at the float64 rotation by handing cos / sin over exactly)
        pose32 = pose.astype(F)
        r = R.tail_ref(pose32, pts, nrm, g_pc, g_nc, g_col, mode, g_xf, fslot, J, latent, np.linalg.norm(latent.astype(np.float64)))
        tol = 2e-7          # the float32 rounding of cos / sin in pose32, relative to the masses
        assert np.abs(r["g_trans"] - tt.grad.numpy()).max() <= 1e-12 * r["mass_g_trans"].max()
        assert abs(r["g_yaw"] - ty.grad.item()) <= tol * r["mass_g_yaw"]
        lat_err = np.abs(r["g_latent"] - tl.grad.numpy())
        assert (lat_err <= tol * r["mass_g_latent"] + 1e-7 * np.abs(tl.grad.numpy())).all(), (lat_err, r["mass_g_latent"])


def test_plan_state_machine_on_a_hand_written_sequence():
    z = np.array([[0.6, 0.8]], F)
    st = dict(lat_ref=np.zeros((1, 2), F), age=np.zeros(1, np.int32), n_full=np.zeros(1, np.int32))
    margin, dev = np.array([0.04], F), np.array([0.01], F)

    def step(zz, margin=margin, dev=dev, max_reuse=3, lip=1.0):
        reuse, st["lat_ref"], st["age"], st["n_full"], dec = R.plan_ref(zz, lip, margin, dev, st["lat_ref"], st["age"], max_reuse, st["n_full"])
        assert dec[0] >= 1e-3
        return int(reuse[0]), int(st["age"][0]), int(st["n_full"][0])

    assert step(z) == (0, 1, 1)                                         # age 0: never planned -> full pass, latent recorded
    assert np.array_equal(st["lat_ref"], z)
    assert step(z) == (1, 2, 1) and step(z) == (1, 3, 1) and step(z) == (1, 4, 1)
    assert step(z) == (0, 1, 2)                                         # age 4 > max_reuse 3
    z2 = z + np.array([[0.02, 0.0]], F)                                 # a latent jump: 0.02 > margin / 4 = 0.01
    assert step(z2) == (0, 1, 3) and np.array_equal(st["lat_ref"], z2)
    z3 = z2 + np.array([[0.005, 0.0]], F)                               # a small move: 0.005 <= 0.01
    assert step(z3) == (1, 2, 3) and np.array_equal(st["lat_ref"], z2)
    assert step(z3, lip=4.0) == (0, 1, 4)                               # the same move under a larger Lipschitz constant
    assert step(z3, dev=np.array([0.03], F)) == (0, 1, 5)               # max_dev above margin / 2


def test_guard_state_machine_on_hand_written_deviations():
    grid = np.zeros((1, 8), F); idx = np.array([[1, 3, 5, 7]], np.int32); cnt = np.array([3], np.int32)
    z2 = np.zeros((1, 2), np.int32)

    def run(dev, margin=0.04, reused=None):
        ex = np.array([[0.0, dev, 0.0, 9.0]], F)
        return R.guard_ref(grid, ex, idx, 4, cnt, np.array([margin], F), np.array([-1.0], F), z2, reused)

    g, m, d, v = run(0.01)                                              # below margin / 2: nothing
    assert g[0].tolist() == [0, 0, 0, F(0.01), 0, 0, 0, 0] and m[0] == F(0.04) and d[0] == F(0.01) and v.tolist() == [[0, 0]]
    g, m, d, v = run(0.03)                                              # between margin / 2 and margin: soft, margin grows to 4 dev
    assert m[0] == F(4) * F(0.03) and v.tolist() == [[1, 0]]
    g, m, d, v = run(0.011, margin=0.02)                                # soft, but 4 dev is the larger
    assert m[0] == F(4) * F(0.011) and v.tolist() == [[1, 0]]
    g, m, d, v = run(0.05)                                              # >= margin: hard as well
    assert m[0] == F(4) * F(0.05) and d[0] == F(0.05) and v.tolist() == [[1, 1]]
    g, m, d, v = run(0.04)                                              # == margin counts as hard
    assert v.tolist() == [[1, 1]]
    g, m, d, v = run(np.nan)                                            # NaN: both, the margin stays
    assert np.isnan(d[0]) and m[0] == F(0.04) and v.tolist() == [[1, 1]] and np.isnan(g[0, 3])
    g, m, d, v = run(0.05, reused=np.array([1]))                        # reused: patched, not judged
    assert g[0, 3] == F(0.05) and m[0] == F(0.04) and d[0] == F(-1) and v.tolist() == [[0, 0]]


def test_remaining_selection_refs_on_small_hand_cases():
    inputs = np.arange(2 * 5 * 2, dtype=F).reshape(2, 5, 2)
    rows = R.candidate_rows_ref(inputs, np.array([[1, 4] + [0] * 126, [2] + [0] * 127], np.int32), 128, np.array([2, 0], np.int32), np.full((2, 128, 2), -7, F))
    assert rows[0, 0].tolist() == [2, 3] and rows[0, 1].tolist() == [8, 9] and (rows[0, 2:] == inputs[0, 0]).all() and (rows[1] == -7).all()
    src = np.arange(12, dtype=F).reshape(1, 2, 6)
    out = R.gather_rows_ref(src, np.array([[0, 1, 2, 3]], np.int32), np.array([[1, -1, 2, 0]], np.int32), 4, np.array([9], np.int32), np.full((1, 4, 6), -7, F))
    assert out[0, 0].tolist() == src[0, 1].tolist() and not out[0, 1].any() and not out[0, 2].any() and out[0, 3].tolist() == src[0, 0].tolist()
    gi, miss = R.sdf_input_grad_ref(np.array([[2.0, 3.0, 0.0]], F), np.array([[0, -1, -1]], np.int32), np.ones((1, 1, 2), F))
    assert gi.tolist() == [[[2, 2], [0, 0], [0, 0]]] and miss == 1
    cslot = np.array([[-1, 0, -1, -1, 1, -1, -1]], np.int32)
    seen = np.concatenate([R.audit_select_ref(cslot, 3, ph)[0] for ph in (3, 4, 5)])
    assert sorted(seen.tolist()) == [0, 2, 3, 5, 6] and R.audit_select_ref(cslot, 3, 4)[0].tolist() == [3, 5]
    dev, vio, ph = R.audit_check_ref(np.array([[0.5, 0.1, 0.9]], F), np.array([0.6, 0.01, np.nan], F), np.array([0, 1, 2]), 3, 8, 3, 0.03, None,
                                     np.zeros(1, F), np.zeros((1, 2), np.int32), 6)
    assert vio.tolist() == [[0, 2]] and dev[0] == np.abs(F(0.5) - F(0.6)) and ph == 7
    g3 = R.gather_rows3_ref(np.arange(9, dtype=F).reshape(1, 3, 3), np.array([[2, 0, 1]], np.int32), np.array([2], np.int32))
    assert g3[0].tolist() == [[6, 7, 8], [0, 1, 2], [0, 0, 0]]
    s3 = R.scatter_add_rows3_ref(np.ones((1, 3, 3), F), np.arange(9, dtype=F).reshape(1, 3, 3), np.array([[2, 0, 1]], np.int32), np.array([2], np.int32))
    assert s3[0].tolist() == [[4, 5, 6], [1, 1, 1], [1, 2, 3]]
