"""Ties the float64 restatement of the sphere tracer (tests/_trace_ref.py) down before the device sees it: against the oracle
(oracle/sdf_oracle.py, float32 numpy), against torch float64 autograd on an analytic SDF whose hit has a closed form, and the conditions the
GPU cases of tests/test_gpu_trace_ref.py must meet by the reference alone -- at most 2 % of a case's rays with a decision closer to its
threshold than the float32 error bound, and every branch the cases are built for populated by at least 8 decided items."""
import numpy as np
import pytest
import torch

from oracle import sdf_oracle as O
from tests import _trace_cases as C
from tests import _trace_ref as R
from tests._util import fitted_state

F = np.float32


# ---- the error arithmetic itself ----------------------------------------------------------------------------------------------------------------

def test_error_arithmetic_bounds_a_float32_evaluation():
    """a float32 numpy evaluation of ray, slab and point (separate multiplications and additions: the most roundings the kernels can take) stays
    within the carried bounds, and the values the reference calls exact come back bit for bit"""
    worst = 0.0
    for name, (Pm, Ki) in C.POSES.items():
        x, y = R.pixels(C.W0, C.H0)
        rays = R.ray(Pm, Ki, x, y)
        o32, d32, r32 = O.trace_rays(Pm, Ki, np.stack([x, y], 1))
        for j in range(3):
            for got, ref in ((d32[:, j], rays["d"][j]), (r32[:, j], rays["r"][j]), (np.full(x.shape, o32[j]), rays["o"][j])):
                u = R.unit(got, ref)
                assert u.max() <= 1.0, (name, j, u.max())
                worst = max(worst, float(u.max()))
        l0, l1, act, rt = R.slab(rays, C.BOUND, C.NEAR)
        a0, a1, aact = O._trace_slab(o32, d32, C.BOUND, C.NEAR)
        dec = rt > 1
        assert np.array_equal(act[dec], aact[dec]), name
        both = act & aact
        assert R.unit(a0, l0)[both].max(initial=0) <= 1.0 and R.unit(a1, l1)[both].max(initial=0) <= 1.0, name
    # exact values: the principal point's column of the axis poses
    rays = R.ray(*C.POSES["axis_in"], np.full(C.H0, 18.0), np.arange(C.H0, dtype=np.float64))
    assert (rays["d"][0].v == 0).all() and (rays["d"][0].e == 0).all() and (rays["d"][2].e == 0).all()
    assert rays["dn"].e[14] == 0 and rays["dn"].v[14] == 1.0
    print("TRACEREF float32 numpy rays: worst %.3g bounds" % worst)


# ---- against the oracle: polish, images, backward on the asset decoder ----------------------------------------------------------------------------

@pytest.fixture(scope="module")
def traced():
    st, spec = fitted_state()
    layers = O.decoder_layers_from_state(st, spec)
    H, W = 24, 32
    K = np.array([[40.0, 0, 15.5], [0, 40.0, 11.5], [0, 0, 1.0]])
    Kinv = np.linalg.inv(K).astype(F)
    pose = O.render_pose(0.6, [0.05, -0.03, 3.5])
    lat = np.asarray([0.3, -0.5, 0.8], F)
    latn = lat / np.sqrt((lat * lat).sum())
    x, y = R.pixels(W, H)
    tr = O.sphere_trace(layers, spec, latn, pose, Kinv, np.stack([x, y], 1), steps=64)
    return dict(tr=tr, pose=np.asarray(pose, F).reshape(16), Kinv=Kinv.reshape(9), W=W, H=H, x=x, y=y, L=latn.size)


def test_setup_polish_and_images_reproduce_the_oracle(traced):
    """set-up on every pixel; then, from the oracle's marched lam0, f0 and Jacobian rows: polish, depth, colour, normals to 1e-6 (the oracle
    works in float32) on the hits whose gate is decided"""
    tr, L = traced["tr"], traced["L"]
    ref = R.setup_crop(traced["pose"], traced["Kinv"], traced["W"], traced["H"], 1.0, 1e-3)
    dec = ref["ratio"] > 1
    assert np.array_equal(ref["active"][dec], tr["entered"][dec]) and dec.mean() > 0.98
    assert R.unit(tr["far"], ref["l1"])[ref["active"] & dec].max() <= 1.0          # (the oracle's exit is a float32 evaluation: within the bound)
    h = np.nonzero(tr["hit"])[0]
    assert h.size > 100
    rays = R.ray(traced["pose"], traced["Kinv"], traced["x"][h], traced["y"][h])
    J = np.concatenate([tr["gz"][h], tr["gx"][h]], 1)
    pol = R.polish(rays, tr["lam0"][h], tr["f0"][h], J, L)
    good = pol["ratio"] > 1
    assert good.mean() > 0.98 and np.array_equal(pol["ok"][good], tr["ok"][h][good])
    img = R.images(traced["pose"], rays, pol)
    assert np.abs(pol["lam_s"].v - tr["lam_s"][h])[good].max() < 1e-6
    assert np.abs(img["depth"].v - tr["depth"][h])[good].max() < 1e-6
    for c in range(3):
        assert np.abs(img["color"][c].v - tr["color"][h, c])[good].max() < 1e-6
        assert np.abs(img["normals"][c].v - tr["normals"][h, c])[good].max() < 1e-6
    xyz, pix = O.traced_points(tr, traced["H"], traced["W"])
    slot, cnt, keep, pts = R.points_crop(tr["hit"], tr["lam_s"], R.ray(traced["pose"], traced["Kinv"], traced["x"], traced["y"]), 10 ** 6)
    assert cnt == pix.size and np.array_equal(keep, pix) and np.array_equal(slot[pix], np.arange(cnt))
    assert max(np.abs(pts[j].v - xyz[:, j]).max() for j in range(3)) < 1e-6


def test_image_backward_reproduces_the_oracle(traced):
    tr, L = traced["tr"], traced["L"]
    n = tr["hit"].size
    rng = np.random.default_rng(3)
    gC, gD, gN = rng.standard_normal((n, 3)).astype(F), rng.standard_normal(n).astype(F), rng.standard_normal((n, 3)).astype(F)
    g_pose, g_latn = O.sphere_trace_backward(tr, traced["pose"].reshape(4, 4), gC, gD, gN)
    h = np.nonzero(tr["hit"])[0]
    rays = R.ray(traced["pose"], traced["Kinv"], traced["x"][h], traced["y"][h])
    J = np.concatenate([tr["gz"][h], tr["gx"][h]], 1)
    pol = R.polish(rays, tr["lam0"][h], tr["f0"][h], J, L)
    assert np.array_equal(pol["ok"], tr["ok"][h])
    s = R.backward_sum(R.backward_terms(traced["pose"], rays, pol, J, L, gC[h], gD[h], gN[h]), n)
    want = np.concatenate([g_pose[:3, :3].reshape(-1), g_pose[:3, 3], g_latn])
    # the oracle sums in float64 but from float32 lam_s, c, n_hat and rays: it differs from the restatement by roundings of those
    # intermediates only, which the bound of a full float32 evaluation covers
    assert (np.abs(s.v[:12 + L] - want) <= s.e[:12 + L]).all(), (np.abs(s.v[:12 + L] - want) / s.e[:12 + L]).max()


# ---- against autograd: a sphere of radius 0.5 + a . z ---------------------------------------------------------------------------------------------

def _sphere_problem():
    rng = np.random.default_rng(11)
    Pm, Ki = C.POSES["generic"]
    L = 3
    a = np.array([0.05, -0.08, 0.03])
    z0 = C.latn(1, L, 4)[0].astype(np.float64)
    rho = 0.5 + a @ z0
    x, y = R.pixels(C.W0, C.H0)
    rays = R.ray(Pm, Ki, x, y)
    o = np.stack([c.v for c in rays["o"]], 1)
    d = np.stack([c.v for c in rays["d"]], 1)
    od, dd, oo = (o * d).sum(1), (d * d).sum(1), (o * o).sum(1)
    disc = od * od - dd * (oo - rho * rho)
    h = np.nonzero(disc > 1e-3)[0]
    lam = (-od[h] - np.sqrt(disc[h])) / dd[h]
    rays_h = R.ray(Pm, Ki, x[h], y[h])
    xs = o[h] + lam[:, None] * d[h]
    gx = xs / np.linalg.norm(xs, axis=1, keepdims=True)                     # grad_x (|x| - rho)
    J = np.concatenate([np.tile(-a, (h.size, 1)), gx], 1)                   # d f / d z = -a
    pol = R.polish(rays_h, lam, np.zeros(h.size), J, L)
    keep = pol["ok"]
    assert keep.sum() >= 64 and (~keep).sum() >= 1
    n = h.size
    g = dict(c=rng.standard_normal((n, 3)), d=rng.standard_normal(n), n=rng.standard_normal((n, 3)), p=rng.standard_normal((n, 3)))
    for k in g:
        g[k] = g[k] * keep.reshape((n,) + (1,) * (g[k].ndim - 1))           # grazing hits: their lam is held constant, autograd's is not
    return dict(P=Pm.astype(np.float64).reshape(4, 4), Ki=Ki.astype(np.float64).reshape(3, 3), a=a, z0=z0, x=x[h], y=y[h], rays=rays_h, pol=pol, J=J,
                g=g, L=L, n=n, xs=xs, nh=gx, lam=lam)


def _autograd(pr, surfel):
    t64 = lambda v: torch.tensor(np.asarray(v, np.float64))
    Pm = t64(pr["P"]).requires_grad_(True)
    z = t64(pr["z0"]).requires_grad_(True)
    Rm, t = Pm[:3, :3], Pm[:3, 3]
    r = torch.stack([t64(pr["x"]), t64(pr["y"]), torch.ones(pr["n"], dtype=torch.float64)], 1) @ t64(pr["Ki"]).T
    nh = t64(pr["nh"])
    sgn = t64([-1.0, 1.0, 1.0])
    if not surfel:
        d = r @ Rm
        o = -(t @ Rm)
        rho = 0.5 + (t64(pr["a"]) * z).sum()
        od, dd, oo = (o * d).sum(1), (d * d).sum(1), (o * o).sum()
        lam = (-od - torch.sqrt(od * od - dd * (oo - rho * rho))) / dd      # the ray-sphere root
        xs = o + lam[:, None] * d
        p_cam = lam[:, None] * r
        depth = lam * r[:, 2]
    else:
        # the material point of the kernel's comment: rigid with the pose, along its fixed normal with the latent
        df = -(t64(pr["a"]) * (z - t64(pr["z0"]))).sum()                     # g_z . dz, |g_x| = 1
        xs = t64(pr["xs"]) - nh * df
        p_cam = xs @ Rm.T + t
        depth = p_cam[:, 2]
    color = (xs * sgn + 1) / 2
    normals = (nh @ Rm.T + 1) / 2
    g = pr["g"]
    loss = (color * t64(g["c"])).sum() + (depth * t64(g["d"])).sum() + (normals * t64(g["n"])).sum() + (p_cam * t64(g["p"])).sum()
    loss.backward()
    gP = Pm.grad.numpy()
    return np.concatenate([gP[:3, :3].reshape(-1), gP[:3, 3], z.grad.numpy()])


@pytest.mark.parametrize("surfel", [False, True])
def test_backward_terms_equal_autograd(surfel):
    """image semantics: the ray-sphere root differentiated through the pose entries, t and z; surfel semantics: the material-point formula;
    all of g_color, g_depth, g_normals, g_xyzf driven"""
    pr = _sphere_problem()
    g = pr["g"]
    terms = R.backward_terms(pr["P"].reshape(16), pr["rays"], pr["pol"], pr["J"], pr["L"], g["c"], g["d"], g["n"], g["p"], surfel=surfel)
    got = np.array([t.v.sum() for t in terms])[:12 + pr["L"]]
    want = _autograd(pr, surfel)
    assert np.abs(got - want).max() < 1e-10 * max(1.0, np.abs(want).max()), np.abs(got - want).max()


# ---- admission and branch population of the GPU cases ---------------------------------------------------------------------------------------------

def test_setup_cases_are_admissible_and_populated():
    und = tot = 0
    seen = dict(par_in=0, par_out=0, par_edge=0, near=0, culled=0, below=0, between=0, beyond=0)
    for names in C.SETUP_BATCHES:
        for b, name in enumerate(names):
            Pm, Ki = C.POSES[name]
            for block in (0, 2, 4, 8):
                cone = C.cone_starts(C.W0, C.H0, block, C.BOUND, C.NEAR, Pm, Ki, b) if block else None
                ref = R.setup_crop(Pm, Ki, C.W0, C.H0, C.BOUND, C.NEAR, cone, block)
                dec = ref["ratio"] > 1
                assert (~dec).sum() <= 0.02 * dec.size, (name, block, int((~dec).sum()))
                und += int((~dec).sum()); tot += dec.size
                if block == 0:
                    par = (np.abs(ref["rays"]["d"][0].v) < R.T_PAR) & dec
                    seen["par_" + {"axis_in": "in", "axis_out": "out", "axis_edge": "edge"}.get(name, "in")] += int(par.sum()) if name.startswith("axis") else 0
                    seen["near"] += int((ref["active"] & (ref["l0"].v == float(F(C.NEAR))) & dec).sum())
                    if name == "axis_edge":
                        assert ref["active"][par].sum() >= 8, "|o_x| = bound is inside"
                    if name == "axis_out":
                        assert not ref["active"][par].any()
                    if name == "behind":
                        assert not ref["active"].any()
                    if name == "inside":
                        assert ref["active"].all()
                else:
                    base = R.setup_crop(Pm, Ki, C.W0, C.H0, C.BOUND, C.NEAR)
                    nbx = (C.W0 + block - 1) // block
                    c = cone[(ref["y"].astype(int) // block) * nbx + ref["x"].astype(int) // block]
                    a = base["active"] & dec
                    seen["culled"] += int((a & (c < 0)).sum())
                    seen["below"] += int((a & (c >= 0) & (c < base["l0"].v)).sum())
                    seen["between"] += int((a & (c > base["l0"].v) & (c < base["l1"].v)).sum())
                    seen["beyond"] += int((a & (c > base["l1"].v)).sum())
    assert min(seen.values()) >= 8, seen
    print("TRACEREF setup cases: %d of %d undecided, branches %s" % (und, tot, seen))


def test_step_cases_take_every_branch():
    for n in (1, 63, 64, 65, 256, 257, 1000):
        case = C.step_case(n, 100 + n)
        ref = C.step_ref(case)
        assert (ref["ratio"] > 1).all() and np.unique(case["pix"]).size == n
        k = case["kinds"]
        assert (ref["what"][np.isin(k, (0, 1, 2))] == 1).all() and (ref["what"][np.isin(k, (3, 4, 5, 8, 9, 10, 11, 12, 13, 15, 16))] == 0).all()
        assert (ref["what"][np.isin(k, (6, 7, 14, 17))] == -1).all()
        assert (ref["q"][k == 11] == F(0.5)).all() and (ref["q"][np.isin(k, (10, 12))] == 1).all()
        mid = ref["q"][k == 13]
        assert ((mid > 0.5) & (mid < 1)).all()
        assert (ref["lam"].e[np.isin(k, (14, 15))] == 0).all(), "the far-equality rays must be exact"
        if n == 1000:
            assert all((k == kind).sum() >= 8 for kind in range(C.STEP_KINDS)), np.bincount(k)
            assert (k == 14).sum() + (k == 15).sum() == len(C.STEP_EXACT)


def test_render_cases_are_admissible_and_populated():
    for sizes, PS, seed in (([(C.W0, C.H0)] * 3, C.W0 * C.H0, 21), ([C.SIZES_R[0], C.BAD_SIZES[1], C.SIZES_R[1]], C.PS_R, 22)):
        case = C.render_case(sizes, PS, C.L3, seed)
        for cr in case["crops"]:
            if cr is None:
                continue
            dec = cr["pol"]["ratio"] > 1
            assert (~dec).sum() <= 0.02 * dec.size
            on = cr["pol"]["ok"]
            assert (on & dec & (cr["kinds"] <= 1)).sum() >= 8 and (~on & dec & (cr["kinds"] == 2)).sum() >= 8
            assert (~on & (cr["kinds"] == 4)).sum() >= 8 and (on[cr["kinds"] <= 1]).all() and not on[cr["kinds"] == 2].any()
        ax = case["crops"][1 if sizes[1][0] == C.W0 else 2]
        exact0 = (ax["pol"]["gd"].v == 0) & (ax["pol"]["gd"].e == 0) & (ax["kinds"] == 3)
        assert exact0.sum() >= 8 or sizes[1][0] != C.W0, "g . d = 0 exactly on the principal point's column"
    for W, H, L, seed in ((16, 16, 0, 56), (16, 16, 3, 59), (16, 16, 8, 64), (17, 16, 3, 60)):
        case = C.render_case([(W, H)] * 3, W * H, L, seed, density=0.6)
        for cr in case["crops"]:
            assert (cr["pol"]["ratio"] > 1).all()
            assert cr["pol"]["ok"].sum() >= 8 and (~cr["pol"]["ok"]).sum() >= 8


# ---- the slab decoder -----------------------------------------------------------------------------------------------------------------------------

def test_slab_decoder_is_the_analytic_slab():
    from tests import _decoder_ref as D
    layers = C.slab_decoder_layers(s=2.0)
    net = D.Net(layers, [(0, 0), (0, 0), (C.L3 + 3, 0), (0, 0)])
    rng = np.random.default_rng(2)
    x = np.concatenate([np.tile(C.latn(1, C.L3), (200, 1)), rng.uniform(-1, 1, (200, 3))], 1).astype(F)
    r = D.evaluate(net, x)
    assert np.array_equal(r.out, C.slab_value(x[:, -1].astype(np.float64), s=2.0))
    assert D.fwd_tol(net, r, "f32").max() < 2e-6


def test_trimmed_slab_net_has_the_same_values_and_tolerances():
    from tests import _decoder_ref as D
    rng = np.random.default_rng(0)
    x = np.concatenate([np.tile(C.latn(1, C.L3), (300, 1)), rng.uniform(-1, 1, (300, 3))], 1).astype(F)
    for arith in ("f32", "f16"):
        d = C.SlabDecoder(1.0, arith)
        r1, r2 = D.evaluate(d.net, x, arith), D.evaluate(d.net_small, x, arith)
        assert np.array_equal(r1.out, r2.out) and np.array_equal(D.fwd_tol(d.net, r1, arith), D.fwd_tol(d.net_small, r2, arith))


SPEC_N = {4: (1, 15, 16, 17, 1000), 8: (1, 7, 8, 9, 1000), 16: (1, 3, 4, 5, 1000), 32: (1, 2, 3, 1000, 2100)}


@pytest.mark.parametrize("arith", ["f32", "f16"])
@pytest.mark.parametrize("K", [4, 8, 16, 32])
def test_speculative_pass_cases_are_decided_and_take_every_branch(K, arith):
    """every crafted state of every case is decided (admission: 0 % <= 2 %); the 1000-ray cases meet every accepted-prefix length 0 .. K-1 on
    at least 8 survivors, exits, hits, a prefix ended by v <= 0, rho = 0, q at 0.5 and at q_max, q' at its lower clamp and free; float32 also hits at a sample j > 0"""
    for n in SPEC_N[K]:
        case = C.spec_case(K, n, arith, 1000 * K + n)
        assert np.unique(case["pix"]).size == n
        ref = C.spec_ref(case)
        assert (ref["ratio"] > 1).all(), (K, n, arith, int((ref["ratio"] <= 1).sum()))
        if n != 1000:
            continue
        keep, hit, J = ref["keep"], ref["hit"], ref["J"]
        assert np.bincount(J[keep], minlength=K).min() >= 8, np.bincount(J[keep], minlength=K)
        assert (~keep & ~hit).sum() >= 8 and (ref["neg_end"] & ~hit).sum() >= 8
        assert (case["st"][:, 1] == 0).sum() >= 1          # (rho = 0 is one of several ways to prefix length 0, which is counted above)
        q = ref["q"]
        assert (case["st"][:, 2] == 0.5).sum() >= 8 and (case["st"][:, 2] == C.QMAX).sum() >= 8
        assert ((q.v == 0.5) & (q.e == 0) & keep).sum() >= 8 and ((q.v > 0.5) & (q.v < C.QMAX) & keep).sum() >= 8
        if arith == "f32":           # (the float16 decoder's tolerance on this decoder is about eps itself: no float16 hit is a decided one)
            assert hit.sum() >= 8 and (hit & (J > 0)).sum() >= 8


def test_slab_decoder_tolerance_constants_come_from_its_cpu_emulation():
    """the float32 / float16 numpy emulations of _decoder_ref on 4000 rows of the slab decoder stay within a quarter of the constants the
    device is judged with (float32: C_BOUND; float16: SlabDecoder.C16), and within the tolerance itself"""
    from tests import _decoder_ref as D
    rng = np.random.default_rng(0)
    x = np.concatenate([np.tile(C.latn(1, C.L3), (4000, 1)), rng.uniform(-1, 1, (4000, 3))], 1).astype(F)
    for arith, c in (("f32", D.C_BOUND["f32_fwd"]), ("f16", C.SlabDecoder.C16)):
        d = C.SlabDecoder(1.0, arith)
        with np.errstate(invalid="ignore", divide="ignore"):
            ratios, e, r0, _ = D.emulation_ratios(d.net_small, x, arith)
        assert ratios["fwd"] <= c / 4, (arith, ratios["fwd"])
        assert (np.abs(e.out - r0.out) <= d.tol(r0)).all()
        print("TRACEREF slab decoder %s emulation: %.3g u mass (constant %.3g)" % (arith, ratios["fwd"], c))


def test_cone_pass_cases_are_admissible_and_populated():
    """per case at most 2 % of the cones undecided; over the cases: cones that stop (the rays take over), culled, still marching, counted
    samples outside the cube and blocks that miss the cube on at least 8 decided cones each"""
    kinds, clamped, missed = np.zeros(3, int), 0, 0
    for block in (2, 4, 8):
        for K in (1, 4, 8):
            und = tot = 0
            for cs, res in C.cone_ref(block, K):
                dec = res["ratio"] > 1
                und += int((~dec).sum()); tot += dec.size
                kinds += np.bincount(res["kind"][dec], minlength=3)
                clamped += int((res["clamped"] & dec).sum())
                missed += int((~cs["keep"]).sum())
            assert und <= 0.02 * tot, (block, K, und, tot)
    assert kinds.min() >= 8 and clamped >= 8 and missed >= 8, (kinds, clamped, missed)
    print("TRACEREF cone cases: stop / culled / marching %s, clamped %d, blocks missing the cube %d" % (kinds.tolist(), clamped, missed))


# ---- whole marches: the restatement against the oracle's float32 loop, the accumulated bound's constant, admission ------------------------------------

class _slab_oracle:
    """oracle/sdf_oracle.py's march loops (float32 numpy) on _decoder_ref's float32 emulation of the slab decoder"""

    def __init__(self, arith="f32"):
        from tests import _decoder_ref as D
        self.D, self.dec, self.arith = D, C.SlabDecoder(1.0, arith), arith

    def __enter__(self):
        self.keep = O.decoder_forward, O.decoder_backward_inputs

        def fwd(layers, spec, rows, want_cache=False):
            out = np.asarray(self.D.emulate(self.dec.net_small, np.asarray(rows, F), self.arith).out, F).reshape(-1, 1)
            return (out, None) if want_cache else out
        O.decoder_forward, O.decoder_backward_inputs = fwd, (lambda layers, spec, rows, cache, g: np.zeros(rows.shape, F))
        return self

    def __exit__(self, *exc):
        O.decoder_forward, O.decoder_backward_inputs = self.keep


MARCH_CASES = [(nm, C.MW, C.MH) for nm in C.MARCH_BATCH] + [(nm, W, H) for nm, (W, H) in zip(C.MARCH_BATCH, C.MARCH_SIZES_R)][1:]


def test_march_restatement_against_the_oracles_float32_loop_and_the_accumulated_constant():
    """R.march (set-up, spec_pass chained over 32 passes, K = 1 and speculative schedules) against oracle.sphere_trace run in float32 on the
    emulated slab decoder: the same hit set on decided rays, the same evaluation count where no ray is undecided, and the float32 hit
    parameters within C_ACC / 4 of the sum of one-step bounds (the constant the device is judged with is 4 x this emulation's worst ratio).
    Admission: at most 2 % of a case's rays undecided."""
    worst = {}
    with _slab_oracle("f32"):
        for nm, W, H in MARCH_CASES:
            Pm, Ki = C.MARCH_POSES[nm]
            x, y = R.pixels(W, H)
            for sched in C.SCHEDULES:
                with np.errstate(all="ignore"):
                    tr = O.sphere_trace(None, None, C.latn(1, C.L3, 5)[0], Pm, Ki, np.stack([x, y], 1), steps=C.MSTEPS, eps=C.EPS, bound=C.BOUND,
                                        near=C.NEAR, spec_from=C.SCHEDULES[sched] or None, sigma=C.SIGMA, q_max=C.QMAX)
                su, m = C.march_ref(nm, sched, "f32", W, H)
                px, dec = m["px"], m["ratio"] > 1
                assert (~dec).sum() <= 0.02 * dec.size, (nm, W, H, sched, int((~dec).sum()), dec.size)
                assert np.array_equal(tr["hit"][px][dec], m["hit"][dec]) and np.array_equal(tr["unresolved"][px][dec], m["unresolved"][dec])
                assert not tr["hit"][~su["active"] & (su["ratio"] > 1)].any()
                assert abs(int(tr["evals"]) - m["evals"]) <= int((~dec).sum()) * m["max_evals"]
                both = tr["hit"][px] & m["hit"] & dec
                assert both.sum() >= 8
                r = float((np.abs(tr["lam0"][px] - m["hit_lam"].v)[both] / m["acc"][both]).max())
                worst[sched] = max(worst.get(sched, 0.0), r)
    print("TRACEREF march emulation, worst |lam32 - lam64| / sum of one-step bounds: %s (C_ACC %.3g)" % (
        " ".join("%s %.3f" % kv for kv in worst.items()), C.C_ACC["f32"]))
    assert max(worst.values()) <= C.C_ACC["f32"] / 4


@pytest.mark.parametrize("block", [4, 8])
def test_cone_restatement_against_the_oracles_cone_march(block):
    """R.cone_setup + R.cone_pass against oracle.cone_march (float32 numpy, one pass, 1 / 4 / 8 samples) on the emulated slab decoder: culled or
    not on decided cones, the start within the restatement's bound"""
    with _slab_oracle("f32"):
        for K in (1, 4, 8):
            for b, (nm, (cs, res)) in enumerate(zip(C.CONE_POSES, C.cone_ref(block, K))):
                Pm, Ki = C.POSES[nm]
                with np.errstate(all="ignore"):
                    start, _, evals = O.cone_march(None, None, C.latn(3, C.L3, 5)[b], Pm, Ki, (C.W0, C.H0), block, np.arange(cs["keep"].size), cone_steps=1,
                                                   eps=C.EPS, bound=C.BOUND, near=C.NEAR, spec_k=K, sigma=C.SIGMA)
                assert (start[~cs["keep"]] == -1).all() and evals == int(cs["keep"].sum()) * K
                got, dec = start[res["sel"]], res["ratio"] > 1
                culled = res["kind"] == 1
                assert np.array_equal((got == -1)[dec], culled[dec])
                ok = dec & ~culled
                assert R.unit(got, res["start"])[ok].max() <= 1.0


# ---- the whole chain on the asset decoder against the oracle ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sched,block", [([], 4), ([], 8), ([(4, 4), (6, 16)], 4), ([(4, 4), (6, 16)], 8)])
def test_chain_on_the_asset_decoder_reproduces_the_oracle(traced, sched, block):
    """cone set-up and pass, set-up with the cone starts, march, polish and images chained in float64 on the asset decoder (8 x 512, weight
    norm; 24 x 32) against oracle.sphere_trace with the same cone phase and schedule.  No per-ray bound here -- the asset decoder has no
    slope bound to carry a point's error into its value -- so rays are screened by the ORACLE's own recorded margin (> 1e-4, the figure the
    end-to-end tracer tests use): on those the hit sets are equal and the evaluation counts of the two marches agree; the marched parameter
    agrees to 2e-6 (32 passes of float32 steps in the oracle, each rounding lam ~ 3.5 at 2e-7 and not amplified), depth, colour and normals
    after the Newton polish to 1e-6."""
    import sdflabel_amd
    from tests import _decoder_ref as D
    from tests._util import ASSET
    dsdf, _ = sdflabel_amd.setup_dsdf(ASSET + ".pt", precision=torch.float32)
    net = D.Net.from_decoder(dsdf)
    st, spec = fitted_state()
    layers = O.decoder_layers_from_state(st, spec)
    pose, Kinv, W, H, x, y, L = (traced[k] for k in ("pose", "Kinv", "W", "H", "x", "y", "L"))
    lat = np.asarray([0.3, -0.5, 0.8], F)
    latn = (lat / np.sqrt((lat * lat).sum())).astype(F)
    tr = O.sphere_trace(layers, spec, latn, pose, Kinv, np.stack([x, y], 1), steps=64, spec_from=sched or None, cone_block=block, cone_steps=1,
                        cone_spec_k=4, image_wh=(W, H))

    def rows_of(pts, n):
        return np.concatenate([np.tile(latn.astype(np.float64), (n, 1)), np.stack([p.v for p in pts], 1)], 1)

    def value_of(idx):
        return lambda pts: R.Ap(D.evaluate(net, rows_of(pts, idx.size), "f32", want_masses=False).out)
    cs = R.cone_setup(pose, Kinv, W, H, block, 1.0, 1e-3)
    with np.errstate(all="ignore"):
        res = R.cone_pass(cs, 4, 0.9, 2e-3, 1.0, value_of(np.nonzero(cs["keep"])[0]))
    cone = np.full(cs["keep"].size, -1.0, F)
    cone[res["sel"]] = res["start"].v.astype(F)
    su = R.setup_crop(pose, Kinv, W, H, 1.0, 1e-3, cone, block)
    px = np.nonzero(su["active"])[0]
    rays = dict(o=[c[px] for c in su["rays"]["o"]], d=[c[px] for c in su["rays"]["d"]], dn=su["rays"]["dn"][px])
    with np.errstate(all="ignore"):
        m = R.march(su["l0"][px], rays, su["l1"].v[px].astype(F), 64, sched, 0.9, 2e-3, 1.0, value_of, 1.0)
    hit, lam = np.zeros(W * H, bool), np.zeros(W * H)
    hit[px], lam[px] = m["hit"], m["hit_lam"].v
    safe = tr["margin"] > 1e-4
    assert safe.mean() > 0.9 and np.array_equal(hit[safe], tr["hit"][safe]) and hit.sum() > 100
    assert abs(m["evals"] - (tr["evals"] - tr["cone_evals"])) <= int((~safe).sum()) * m["max_evals"]      # (equal unless a screened-out ray differs)
    both = np.nonzero(safe & hit & tr["hit"])[0]
    assert np.abs(lam - tr["lam0"])[both].max() < 2e-6
    hr = R.ray(pose, Kinv, x[both], y[both])
    r = D.evaluate(net, rows_of(R.point(hr, lam[both]), both.size), "f32", want_masses=False)
    pol = R.polish(hr, lam[both], r.out, r.J, L)
    same_gate = pol["ok"] == tr["ok"][both]
    assert same_gate.mean() > 0.98
    img = R.images(pose, hr, pol)
    assert np.abs(img["depth"].v - tr["depth"][both])[same_gate].max() < 1e-6
    for c in range(3):
        assert np.abs(img["color"][c].v - tr["color"][both, c])[same_gate].max() < 1e-6
    dn = np.max([np.abs(img["normals"][c].v - tr["normals"][both, c]) for c in range(3)], 0)[same_gate]
    assert np.median(dn) < 1e-6 and (dn > 1e-4).sum() <= 3          # (a hit on a ReLU kink takes its gradient from either side: isolated rays)
