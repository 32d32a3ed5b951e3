"""The decoder's training kernels (csrc/mlp_train.hip) through the C ABI against the float64 restatement of tests/_prior_train_ref.py, every
output element judged by its own c u mass (constants calibrated on the CPU, tests/test_prior_train_cpu.py); the same-bits guarantees; the
autograd Function against golden G23; PriorTrainer's trajectory against torch float64; and a small prior trained end to end.
"""
import numpy as np
import pytest
import torch

from sdflabel_amd import _lib
from sdflabel_amd.deepsdf.train import TrainDesc, decoder_train, expand_latents, train_backward, train_forward
from tests import _prior_train_cases as PC
from tests import _prior_train_loop as TL
from tests import _prior_train_ref as PR
from tests._util import gold

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64
SENT = -777.25

# what the float32 torch CPU run of the trajectory loop shows against float64 (measured, profiles/prior_train_notes.md), times 4
TRAJ_TOL = {"loss": 4 * 2.62e-8, "latents": 4 * 9.62e-8, "params": 4 * 5.17e-7}


class Guarded:
    """a float32 device buffer with sentinel words before and behind it"""

    def __init__(self, size):
        self.buf = torch.full((size + 2 * GUARD,), SENT, dtype=torch.float32, device=DEV)
        self.t = self.buf[GUARD:GUARD + size]

    def intact(self):
        return bool((self.buf[:GUARD] == SENT).all()) and bool((self.buf[-GUARD:] == SENT).all())


def run_kernels(name, n, p, x=None, g=None, seed=PC.SEED):
    """one forward and backward through the C ABI with guard words round every output and the workspace"""
    dec = PC.decoders()[name]
    net = PC.net(name)
    desc = TrainDesc.from_decoder(dec)
    if x is None:
        x, g = PC.rows(name, n)
    W = [torch.from_numpy(w).to(DEV).contiguous() for w in net.W]
    B = [torch.from_numpy(b).to(DEV).contiguous() for b in net.b]
    o = {"desc": desc, "net": net}
    o["ws"], o["sdf"], o["gin"] = Guarded(desc.bytes(n) // 4), Guarded(n), Guarded(n * net.n_inputs)
    o["dW"] = [Guarded(w.numel()) for w in W]
    o["db"] = [Guarded(b.numel()) for b in B]
    xd, gd = torch.from_numpy(np.ascontiguousarray(x)).to(DEV), torch.from_numpy(np.ascontiguousarray(g)).to(DEV)
    train_forward(desc, W, B, xd, p, seed, o["ws"].t, o["sdf"].t)
    train_backward(desc, W, gd, o["ws"].t, [d.t for d in o["dW"]], [d.t for d in o["db"]], o["gin"].t)
    torch.cuda.synchronize()
    L = PR.layout(net, n)
    ws = o["ws"].t.cpu().numpy()
    o["L"], o["ws_np"] = L, ws
    o["acts"] = [ws[L.act[l]:L.act[l] + n * L.in_dim[l + 1]].reshape(n, L.in_dim[l + 1]) for l in range(net.n_lin - 1)]
    tail = ws[L.tail:L.tail + 2 * n].reshape(n, 2)
    o["y1"], o["out_ws"] = tail[:, 0], tail[:, 1]
    o["sdf_np"] = o["sdf"].t.cpu().numpy()
    o["gin_np"] = o["gin"].t.cpu().numpy().reshape(n, net.n_inputs)
    o["dW_np"] = [d.t.cpu().numpy().reshape(w.shape) for d, w in zip(o["dW"], net.W)]
    o["db_np"] = [d.t.cpu().numpy() for d in o["db"]]
    o["guards"] = all(b.intact() for b in [o["ws"], o["sdf"], o["gin"]] + o["dW"] + o["db"])
    return o


@pytest.mark.parametrize("name,n,p", PC.cases(), ids=lambda v: str(v))
def test_kernels_against_the_float64_restatement(name, n, p):
    net = PC.net(name)
    x, g = PC.rows(name, n)
    dl = PC.drop_layers(name)
    keep, scale = PR.keep_masks(net, PC.SEED, n, p, dl), PR.scales(net, p, dl)
    o = run_kernels(name, n, p)
    assert o["guards"], "a guard word was written"
    assert np.array_equal(o["out_ws"], o["sdf_np"])
    acts = [a[:, :od] for a, od in zip(o["acts"], net.out_dims)]
    # the re-injected columns behind the activations are the input columns
    for l in range(1, net.n_lin):
        cnt, off = net.inj[l]
        if cnt:
            assert np.array_equal(o["acts"][l - 1][:, net.out_dims[l - 1]:], x[:, off:off + cnt])
    j, r, bm = PR.judge(net, x, g, keep, scale, o["sdf_np"], o["y1"], acts, o["gin_np"], o["dW_np"], o["db_np"])
    print(name, n, p, {k: (round(v, 4) if isinstance(v, float) else v) for k, v in j.items()})
    assert np.isfinite(o["sdf_np"]).all() and np.isfinite(o["gin_np"]).all()
    assert j["fwd"] <= 1, "sdf outside (1 - out^2) c_fwd u M_fwd + c_t u |out|"
    assert j["bad_units"] == 0, "a certain unit has the wrong zero pattern"
    assert j["wrong_drop"] == 0, "a unit the hash drops is not zero"
    assert j["free_share"] <= PR.FREE_CAP
    assert j["dx"] <= 1 and j["dw"] <= 1 and j["db"] <= 1
    # the second run gives the same bits everywhere
    o2 = run_kernels(name, n, p)
    assert np.array_equal(o2["sdf_np"], o["sdf_np"]) and np.array_equal(o2["gin_np"], o["gin_np"])
    assert all(np.array_equal(a, b) for a, b in zip(o2["dW_np"] + o2["db_np"], o["dW_np"] + o["db_np"]))
    assert all(np.array_equal(a, b) for a, b in zip(o2["acts"], o["acts"]))


def test_kept_values_carry_the_float32_scale_and_dropped_units_are_the_hashs():
    name, n = "w512", 200
    net = PC.net(name)
    a0 = run_kernels(name, n, 0.0)["acts"][0][:, :net.out_dims[0]]
    a1 = run_kernels(name, n, PC.P)["acts"][0][:, :net.out_dims[0]]
    keep = PR.keep_mask(PC.SEED, 0, n, net.out_dims[0], PC.P)
    scale = np.float32(1.0) / (np.float32(1.0) - np.float32(PC.P))
    assert 0.7 < keep.mean() < 0.9
    assert np.array_equal(a1, np.where(keep, a0 * scale, np.float32(0)))       # layer 0 sees the same inputs in both runs: exact
    other = run_kernels(name, n, PC.P, seed=PC.SEED + 1)["acts"][0][:, :net.out_dims[0]]
    assert not np.array_equal(other, a1)


def test_a_row_alone_and_in_a_batch_gives_the_same_bits():
    name, n = "w128", 200
    x, g = PC.rows(name, n)
    full = run_kernels(name, n, 0.0)
    for i in (0, 63, 64, 199):
        one = run_kernels(name, 1, 0.0, x[i:i + 1], g[i:i + 1])
        assert one["sdf_np"][0] == full["sdf_np"][i] and np.array_equal(one["gin_np"][0], full["gin_np"][i]), i
    # at another position: the rows reversed
    rev = run_kernels(name, n, 0.0, x[::-1], g[::-1])
    assert np.array_equal(rev["sdf_np"][::-1], full["sdf_np"]) and np.array_equal(rev["gin_np"][::-1], full["gin_np"])
    # with dropout the hash sees the row index: equal positions give equal bits whatever the batch
    big = run_kernels(name, n, PC.P)
    small = run_kernels(name, 65, PC.P, x[:65], g[:65])
    assert np.array_equal(small["sdf_np"], big["sdf_np"][:65]) and np.array_equal(small["gin_np"], big["gin_np"][:65])
    assert not np.array_equal(big["sdf_np"], full["sdf_np"])


def test_dw_of_one_chunk_is_the_single_partial():
    o = run_kernels("w128", PR.CHUNK, 0.0)
    L, net = o["L"], o["net"]
    assert L.chunks == 1
    n_dw = net.W[0].size
    part = o["ws_np"][L.part:L.part + n_dw].reshape(net.W[0].shape)             # the backward handled layer 0 last
    assert np.array_equal(part, o["dW_np"][0])
    assert np.array_equal(o["ws_np"][L.part + n_dw:L.part + n_dw + net.W[0].shape[0]], o["db_np"][0])
    # three partials: the sum in chunk order
    o = run_kernels("w128", 2 * PR.CHUNK + 76, 0.0)
    L = o["L"]
    parts = o["ws_np"][L.part:L.part + 3 * n_dw].reshape(3, *net.W[0].shape)
    assert np.array_equal((parts[0] + parts[1]) + parts[2], o["dW_np"][0])


def test_errors_are_errors_not_faults():
    dec = PC.decoders()["w128"]
    desc = TrainDesc.from_decoder(dec)
    net = PC.net("w128")
    W = [torch.from_numpy(w).to(DEV) for w in net.W]
    B = [torch.from_numpy(b).to(DEV) for b in net.b]
    x = torch.zeros((10, 6), device=DEV)
    sdf = torch.empty((10,), device=DEV)
    ws = torch.empty((desc.bytes(10) // 4 - 1,), device=DEV)
    with pytest.raises(_lib.SdfrError, match="workspace"):
        train_forward(desc, W, B, x, 0.0, 0, ws, sdf)
    with pytest.raises(_lib.SdfrError, match="inputs must be"):
        decoder_train(torch.zeros((10, 5), device=DEV), W, B, desc)
    # n = 0 is no launch
    out = decoder_train(torch.zeros((0, 6), device=DEV), W, B, desc)
    assert out.shape == (0, 1)


# ---- the autograd Function against golden G23 -----------------------------------------------------------------------------------------

def test_decoder_train_function_against_golden_g23():
    z = gold("g23_prior_train.npz")
    S, K = int(z["S"]), int(z["K"])
    inj = [(0, 0), (0, 0), (6, 0), (0, 0), (0, 0)]
    vs = [z["state.lin%d.weight_v" % l] for l in range(5)]
    gs = [z["state.lin%d.weight_g" % l] for l in range(5)]
    bs = [z["state.lin%d.bias" % l] for l in range(5)]
    desc = TrainDesc([v.shape[1] for v in vs], [v.shape[0] for v in vs], inj, 6)
    tv = [torch.from_numpy(v).to(DEV).requires_grad_(True) for v in vs]
    tg = [torch.from_numpy(g).to(DEV).requires_grad_(True) for g in gs]
    tb = [torch.from_numpy(b).to(DEV).requires_grad_(True) for b in bs]
    lat = torch.from_numpy(z["latents"].astype(np.float32)).to(DEV).requires_grad_(True)
    xyz = torch.from_numpy(z["xyz"].astype(np.float32)).to(DEV)
    target = torch.from_numpy(z["target"].astype(np.float32)).to(DEV)
    Ws = [v * (g / v.norm(2, dim=1, keepdim=True)) for v, g in zip(tv, tg)]
    inputs = torch.cat([expand_latents(lat, K), xyz], 1)
    pred = decoder_train(inputs, Ws, tb, desc)[:, 0]
    loss = (pred.clamp(-0.1, 0.1) - target.clamp(-0.1, 0.1)).abs().mean()
    loss.backward()
    torch.cuda.synchronize()
    u = PR.U32
    assert abs(float(loss) - float(z["loss"])) <= 8 * u * max(1.0, abs(float(z["loss"])))

    # the float64 restatement at the float32 effective weights the kernels saw, on the kernels' own ReLU pattern and tail
    n = S * K
    W32 = [w.detach().cpu().numpy() for w in Ws]
    net = PR.Net64([(w, b) for w, b in zip(W32, bs)], inj)
    x = inputs.detach().cpu().numpy()
    r = PR.forward(net, x)
    _, g_sdf = PR.clamped_l1(pred.detach().cpu().numpy(), z["target"])
    L = PR.layout(net, n)
    ws = desc.workspace(n, torch.device(DEV, torch.cuda.current_device())).cpu().numpy()
    acts = [ws[L.act[l]:L.act[l] + n * L.in_dim[l + 1]].reshape(n, -1)[:, :net.out_dims[l]] for l in range(4)]
    tail = ws[L.tail:L.tail + 2 * n].reshape(n, 2)
    bm = PR.backward(net, r, g_sdf, deriv=PR.deriv_from_acts(acts, [1.0] * 4), tail=(tail[:, 0], tail[:, 1]))
    # the float64 fold at the float32 parameters differs from the float32 fold the kernels saw by the format's rounding: the exact effect
    # of that on each gradient is |restatement(W32) - golden|, computed from the references alone
    v64 = [v.astype(np.float64) for v in vs]
    g64 = [g.astype(np.float64) for g in gs]
    worst = 0.0
    for l in range(5):
        dv, dg = PR.fold_backward(v64[l], g64[l], bm.dW[l])
        tW = PR.C["c_dw"] * u * bm.M_dW[l] + 2 * u * np.abs(bm.dW[l])                # the kernel's dW, g_sdf = +-fl32(1/n)
        nv = np.linalg.norm(v64[l], axis=1, keepdims=True)
        aw = np.abs(bm.dW[l])
        tv_ = tW * np.abs(g64[l] / nv) + np.abs(v64[l]) * (tW * np.abs(v64[l])).sum(1, keepdims=True) * np.abs(g64[l]) / nv ** 3
        fold_v = 8 * u * (aw * np.abs(g64[l] / nv) + np.abs(v64[l]) * (aw * np.abs(v64[l])).sum(1, keepdims=True) * np.abs(g64[l]) / nv ** 3)
        tg_ = (tW * np.abs(v64[l])).sum(1, keepdims=True) / nv
        fold_g = 8 * u * (aw * np.abs(v64[l])).sum(1, keepdims=True) / nv
        gold_v, gold_g, gold_b = z["grad.lin%d.weight_v" % l], z["grad.lin%d.weight_g" % l], z["grad.lin%d.bias" % l]
        tb_ = PR.C["c_dw"] * u * bm.M_db[l] + 2 * u * np.abs(bm.db[l])
        for what, got, ref, tol, goldv in (("v", tv[l].grad, dv, tv_ + fold_v, gold_v), ("g", tg[l].grad, dg, tg_ + fold_g, gold_g),
                                           ("b", tb[l].grad, bm.db[l], tb_, gold_b)):
            got = got.cpu().numpy().astype(np.float64)
            tol = tol + np.abs(ref - goldv)
            ratio = PR._ratio(np.abs(got - goldv), tol).max()
            worst = max(worst, float(ratio))
            assert ratio <= 1, (l, what, float(ratio))
            # the reference's own gradients rounded to float32 lie inside the tolerance
            assert (np.abs(goldv.astype(np.float32).astype(np.float64) - goldv) <= tol).all(), (l, what)
    # the latents: the segmented sum of the input gradient's latent columns, blocks in order
    got = lat.grad.cpu().numpy().astype(np.float64)
    ref = bm.g_inputs[:, :3].reshape(S, K, 3).sum(1)
    tol = (PR.C["c_dx"] * u * bm.M_gin[:, :3] + 2 * u * np.abs(bm.g_inputs[:, :3])).reshape(S, K, 3).sum(1) + \
        K * u * np.abs(bm.g_inputs[:, :3]).reshape(S, K, 3).sum(1) + np.abs(ref - z["g_latents"])
    ratio = PR._ratio(np.abs(got - z["g_latents"]), tol).max()
    print("G23: worst parameter ratio %.3f, latent ratio %.3f" % (worst, ratio))
    assert ratio <= 1
    assert (np.abs(z["g_latents"].astype(np.float32).astype(np.float64) - z["g_latents"]) <= tol).all()


# ---- PriorTrainer ------------------------------------------------------------------------------------------------------------------

def test_trajectory_of_ten_steps_against_torch_float64():
    rows, shapes = TL.analytic_rows()
    batches = [(shapes, rows)] * 10
    ref_l, ref_z, ref_s = TL.torch_loop(TL.fresh_trainer("cpu", drop_p=0.0), batches, torch.float64)
    tr = TL.fresh_trainer(DEV, drop_p=0.0)
    losses = np.array([float(tr.step(b)) for b in batches])
    dl = np.abs(losses - ref_l).max()
    dz = float((tr.latents.detach().cpu().double() - ref_z).abs().max())
    st = tr.decoder.state_dict()
    dp = max(float((st[k].detach().cpu().double() - v).abs().max()) for k, v in ref_s.items())
    print("trajectory: |loss - f64| %.3g (tol %.3g), latents %.3g (%.3g), parameters %.3g (%.3g)"
          % (dl, TRAJ_TOL["loss"], dz, TRAJ_TOL["latents"], dp, TRAJ_TOL["params"]))
    assert ref_l[-1] < 0.3 * ref_l[0]                                           # the loop does train
    assert dl <= TRAJ_TOL["loss"] and dz <= TRAJ_TOL["latents"] and dp <= TRAJ_TOL["params"]
    # scale_net keeps its initial values
    init = TL.fresh_trainer("cpu", drop_p=0.0).decoder.state_dict()
    assert all(torch.equal(st[k].cpu(), v) for k, v in init.items() if k.startswith("scale_net"))
    # the same bits on a second run
    tr2 = TL.fresh_trainer(DEV, drop_p=0.0)
    l2 = np.array([float(tr2.step(b)) for b in batches])
    assert np.array_equal(l2, losses) and torch.equal(tr2.latents, tr.latents)


def test_a_small_prior_trained_end_to_end(tmp_path):
    from sdflabel_amd import mesh as M
    from sdflabel_amd import sdf_samples as S
    from sdflabel_amd.deepsdf.workspace import setup_dsdf
    from tests._mesh_sdf_cases import icosphere, unit_cube
    meshes = []
    for radius in (0.45, 0.75):
        v, f = icosphere(2, radius)
        meshes.append(M.Mesh(torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV)))
    for ext in ((1.0, 0.6, 1.2), (0.6, 1.3, 0.8)):
        v, f = unit_cube()
        meshes.append(M.Mesh(torch.from_numpy(((v - 0.5) * np.array(ext, np.float32)).astype(np.float32)).to(DEV), torch.from_numpy(f).to(DEV)))
    samples = S.draw_sdf_samples(meshes, n=2048, generator=torch.Generator().manual_seed(21))
    rows = torch.cat([s.rows for s in samples])
    shapes = torch.arange(4)
    steps = 150
    batches = [(shapes, rows.cpu())] * steps
    cpu_l, _, _ = TL.torch_loop(TL.fresh_trainer("cpu"), batches, torch.float32, drop_p=0.2)
    tr = TL.fresh_trainer(DEV)
    assert tr.drop_p == 0.2
    dev_batch = (shapes.to(DEV), rows)
    losses = torch.stack([tr.step(dev_batch) for _ in range(steps)]).cpu().numpy()
    print("end to end: final loss %.5f on the device, %.5f in the torch float32 CPU loop (first %.5f)" % (losses[-1], cpu_l[-1], losses[0]))
    assert losses[-1] <= 1.5 * cpu_l[-1]
    path = tr.save(str(tmp_path / "prior"))
    dsdf, _ = setup_dsdf(path, precision=torch.float32)
    dsdf.to(DEV)
    lat = tr.decoder_latents()
    own, _ = S.prior_residuals(dsdf, lat, samples)
    own = own.cpu().numpy()
    for shift in (1, 2, 3):
        other, _ = S.prior_residuals(dsdf, lat.roll(shift, 0), samples)
        other = other.cpu().numpy()
        print("own latent", own, "latent of shape + %d" % shift, other)
        assert (own < other).all()
    for m in M.meshes_many(dsdf, lat, resolution=24):
        assert m.is_closed() and m.volume() > 0
