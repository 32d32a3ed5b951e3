"""The float64 references of the renderer kernels (tests/_splat_ref.py) and the inputs they are applied to (tests/_splat_cases.py), tied
down without a GPU: the float64 restatement equals float64 torch autograd on the torch restatement of oracle/torch_cpu_port.py, in
float32 it reproduces the goldens captured from the reference within their existing bounds, the committed inputs are decidable in float32
(admission), and the constants of the bounds are 4 x the float32 error of the reference's own arithmetic."""
import numpy as np
import pytest
import torch

from oracle import sdf_oracle as O
from oracle import torch_cpu_port as TP
from tests import _splat_cases as SC
from tests import _splat_ref as R
from tests._util import gold

KINDS = (("color_pre", "mass_color", 0), ("depth", "mass_depth", 0), ("normals_pre", "mass_normals", 0),
         ("g_p", "mass_g_p", 1), ("g_n", "mass_g_n", 1), ("g_attr", "mass_g_attr", 1))


# ---- float64 restatement == float64 autograd ----------------------------------------------------------------------------------------

def _tie_scene():
    sc = SC.sheet(31, 16, 20, 90, zc=1.2, az=0.3)
    sc["attr"] = sc["attr"].copy()
    return sc


@pytest.mark.parametrize("use_bg", [False, True])
@pytest.mark.parametrize("prim,alt", SC.PRIM_CASES + [("disc", True)])
def test_float64_reference_equals_torch_autograd(prim, alt, use_bg):
    """images, dense weights and the three gradient arrays against torch.autograd in float64 on the torch restatement, to 1e-12 of the
    array's scale.  The background logit and, for the circles, the projections and the depth norm are constants handed in, as the kernels
    receive them (the Python layer adds the background row's own gradient)."""
    sc = _tie_scene()
    H, W = sc["H"], sc["W"]
    kw = SC.ref_kwargs(sc, prim, alt, use_bg)
    diam, C, cc = R.DEFAULTS[prim]
    kw["exp_ovf"] = 709.782712893384      # float64's sigmoid(x) = 1 / (1 + exp(-x)) is positive down to -log(DBL_MAX), float32's to -88.7
    grads = SC.upstream(sc)
    ref = R.splat_ref(prim, sc["K"], sc["Kinv"], sc["p"], sc["n"], sc["attr"], W, H, grads=grads, want_W=True, **kw)
    D = lambda a: torch.from_numpy(np.asarray(a, np.float32).astype(np.float64))
    K, Kinv = D(sc["K"]), D(sc["Kinv"])
    p, n, a = (D(sc[k]).requires_grad_(True) for k in ("p", "n", "attr"))
    diam = R.f32(diam)
    bgl = float(kw["bg_logit"]) if use_bg else None
    grid = torch.from_numpy(O.pixel_grid((W, H))[None])
    if prim == "disc":
        prob = TP.inside_surfel(K, grid, p, n, diam=diam, depth_constant=C, softclamp=alt, softclamp_constant=cc, bg_logit=bgl, Kinv=Kinv, eps=R.EPS32)
    elif prim == "circle":
        prob = TP.inside_circle(K, grid, D(kw["uv"]), p, diam=diam, depth_constant=C, softclamp=not alt, softclamp_constant=cc, bg_logit=bgl,
                                znorm=float(kw["znorm"]), eps=R.EPS32)
    else:
        prob = TP.inside_circle_opt(K, D(kw["uv"]), p, (W, H), diam=diam, depth_constant=C, softclamp=not alt, softclamp_constant=cc,
                                    bg_logit=bgl, znorm=float(kw["znorm"]), eps=R.EPS32)
    out = TP.composite(prob, a, p, n, bg=D(kw["bg"]) if use_bg else None)
    loss = sum((out[k] * D(g).reshape(out[k].shape)).sum() for k, g in zip(("color", "mask", "depth", "normals"), grads))
    loss.backward()
    close = lambda got, want, what: np.testing.assert_array_less(np.abs(np.asarray(got) - np.asarray(want)).max(),
                                                                 1e-12 * max(1.0, np.abs(np.asarray(want)).max()), err_msg=what)
    close(ref["W"], prob.detach().numpy(), "weights")
    for k in ("color", "mask", "depth", "normals"):
        close(ref[k].reshape(-1), out[k].detach().numpy().reshape(-1), k)
    assert (ref["ncov"] > 0).mean() > 0.5 and np.abs(ref["g_p"]).max() > 1e-3
    close(ref["g_p"], p.grad.numpy(), "g_p")
    close(ref["g_n"], n.grad.numpy(), "g_n")
    close(ref["g_attr"], a.grad.numpy(), "g_attr")


def test_float64_reference_equals_the_numpy_oracle():
    """the same against oracle/sdf_oracle.py in float64 (inside_surfel + splat_backward; inside_circle(_opt) + circle_backward), which the
    goldens G7 / G9 pin in float32"""
    sc = _tie_scene()
    H, W = sc["H"], sc["W"]
    grads = SC.upstream(sc)
    D = lambda a: np.asarray(a, np.float32).astype(np.float64)
    ref = R.splat_ref("disc", sc["K"], sc["Kinv"], sc["p"], sc["n"], sc["attr"], W, H, grads=grads, want_W=True)
    g2 = O.pixel_grid((W, H))
    # (the oracle takes eps from the dtype: float64's 2.2e-16 instead of float32's 1.2e-7 in nu + eps -- a relative 1e-7 on the logits)
    Wo = O.inside_surfel(D(sc["Kinv"]), g2, D(sc["p"]), D(sc["n"]), diam=R.f32(0.04))
    assert np.abs(Wo - ref["W"]).max() < 1e-4 and ((Wo > 0) == (ref["W"] > 0)).all()
    gp, gn, ga = O.splat_backward(D(sc["Kinv"]), (W, H), D(sc["p"]), D(sc["n"]), D(sc["attr"]), *[D(g) for g in grads], diam=R.f32(0.04))
    for got, want in ((ref["g_p"], gp), (ref["g_n"], gn), (ref["g_attr"], ga)):
        assert np.abs(got - want).max() < 1e-4 * max(1.0, np.abs(want).max())


# ---- float32: the goldens captured from the reference -----------------------------------------------------------------------------------

def _weights32(prim, z, bg, **kw):
    W, H = [int(v) for v in z["res"]]
    K = z["K"].astype(np.float32)
    Kinv = np.linalg.inv(K).astype(np.float32)
    sc = dict(K=K, Kinv=Kinv, p=z["points"], n=z["normals"], W=W, H=H, seed=0)
    ex = {}
    C = kw.get("depth_constant", R.DEFAULTS[prim][1])
    if prim != "disc":
        ex["uv"] = z["uv"]
        ex["znorm"] = np.float32(np.sqrt((z["points"][:, 2].astype(np.float32) ** 2).sum(dtype=np.float32)))
    if bg:
        ex["bg"] = np.zeros((3, H, W), np.float32)
        ex["bg_logit"] = SC.background(sc, prim, C)[1]
    return R.splat_ref(prim, K, Kinv, z["points"], z["normals"], z["normals"], W, H, want_W=True, dtype=np.float32, **ex, **kw)["W"]


@pytest.mark.parametrize("name", ["disc", "circle", "circle_opt"])
@pytest.mark.parametrize("bg", [False, True])
def test_float32_reference_reproduces_g13(name, bg):
    z = gold("g13_primitives.npz")
    w = _weights32(name, z, bg)
    ref = z["%s_bg%d_w" % (name, int(bg))]
    assert w.shape == ref.shape
    assert np.abs(w - ref).max() < (1e-3 if name == "circle_opt" else 2e-6)


G13S = {
    "disc_default_bg1": ("disc", True, dict(diam=0.03, alt=True, clamp_c=5)),
    "disc_soft_bg0": ("disc", False, dict(diam=0.04, alt=True, clamp_c=5)),
    "disc_soft_c40_bg1": ("disc", True, dict(diam=0.04, alt=True, clamp_c=40)),
    "circle_hard_bg0": ("circle", False, dict(diam=0.02, alt=True)),
    "circle_hard_bg1": ("circle", True, dict(diam=0.02, alt=True)),
    "circle_c30_default_diam_bg0": ("circle", False, dict(diam=0.07, alt=False, clamp_c=30)),
    "circle_opt_hard_bg0": ("circle_opt", False, dict(diam=0.025, alt=True)),
    "circle_opt_hard_bg1": ("circle_opt", True, dict(diam=0.025, alt=True)),
}


@pytest.mark.parametrize("case", sorted(G13S))
def test_float32_reference_reproduces_g13s(case):
    z, zs = gold("g13_primitives.npz"), gold("g13s_primitive_clamps.npz")
    name, bg, kw = G13S[case]
    w = _weights32(name, z, bg, **kw)
    ref = zs[case + "_w"]
    assert w.shape == ref.shape
    assert ((w > 0) == (ref > 0)).mean() > 0.9999
    assert np.abs(w - ref).max() < (1e-3 if name == "circle_opt" else 5e-6)


def test_float32_reference_reproduces_g5():
    z = gold("g5_inside_surfel.npz")
    W, H = [int(v) for v in z["res"]]
    for bg in (0, 1):
        ex = {}
        if bg:
            ex = dict(bg=np.zeros((3, H, W), np.float32), bg_logit=np.float32((-z["points"][:, 2] * np.float32(150)).min() - np.float32(1)))
        w = R.splat_ref("disc", np.linalg.inv(z["Kinv"].astype(np.float64)), z["Kinv"], z["points"], z["normals"], z["normals"], W, H, want_W=True,
                        dtype=np.float32, **ex)["W"]
        assert w.shape == z["w_bg%d" % bg].shape
        assert np.allclose(w, z["w_bg%d" % bg], atol=2e-6)


def _render32(prim, K, Kinv, W, H, proj, attr, bg=None):
    f = np.float32
    v3, nc = proj["points_3d"].astype(f), proj["normals_3d"].astype(f)
    sc = dict(K=K.astype(f), Kinv=Kinv.astype(f), p=v3, n=nc, W=W, H=H, seed=0)
    ex = {}
    if prim != "disc":
        ex["uv"] = proj["points_2d"].astype(f)
        ex["znorm"] = f(np.sqrt((v3[:, 2] ** 2).sum(dtype=f)))
    if bg is not None:
        ex["bg"], ex["bg_logit"] = bg, SC.background(sc, prim, R.DEFAULTS[prim][1])[1]
    return R.splat_ref(prim, K, Kinv, v3, nc, attr.astype(f), W, H, dtype=f, **ex)


@pytest.mark.parametrize("res", [(32, 32), (64, 48)])
def test_float32_reference_reproduces_g6(res):
    z = gold("g6_rasterer.npz")
    H, W = res
    t0 = "r%dx%d_" % (H, W)
    K, Kinv = z[t0 + "K"], z[t0 + "Kinv"]
    for flag, name in ((True, "nocs_"), (False, "col_")):
        proj = O.project_in_2D(K, z["pose"], z["points"], z["normals"], z["colors"], (W, H), flag)
        attr = (proj["colors_3d"] + 1) / 2 if flag else proj["colors_3d"]
        r = _render32("disc", K, Kinv, W, H, proj, attr)
        for k in ("color", "mask", "depth", "normals"):
            assert r[k].shape == z[t0 + name + k].shape
            assert np.abs(r[k] - z[t0 + name + k]).max() < 1e-4, k
    proj = O.project_in_2D(K, z["pose"], z["points"], z["normals"], z["colors"], (W, H), True)
    r = _render32("disc", K, Kinv, W, H, proj, (proj["colors_3d"] + 1) / 2, bg=z[t0 + "bg"])
    for k in ("color", "mask"):
        assert np.abs(r[k] - z[t0 + "bg_" + k]).max() < 1e-4, k


@pytest.mark.parametrize("prim,use_bg", [("circle", False), ("circle", True), ("circle_opt", False), ("circle_opt", True), ("disc", True)])
def test_float32_reference_reproduces_g9_images(prim, use_bg):
    z = gold("g9_secondary.npz")
    H = W = 32
    t = "%s_bg%d_" % (prim, int(use_bg))
    K, Kinv = z["K"], z["Kinv"]
    proj = O.project_in_2D(K, z[t + "pose"], z["points"], z["normals"], z["normals"], (W, H), True)
    r = _render32(prim, K, Kinv, W, H, proj, (proj["colors_3d"] + 1) / 2, bg=z["bg"] if use_bg else None)
    tol = 1e-3 if prim == "circle_opt" else 1e-4
    for k in (("color", "mask") if use_bg else ("color", "mask", "depth", "normals")):
        assert np.abs(r[k] - z[t + "out_" + k]).max() < tol, k


# ---- admission of the committed inputs --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", SC.ALL_CASES, ids=SC.case_id)
def test_committed_cases_are_decidable_in_float32(c):
    """on the reference alone: at most 2 % of the scene's surfels were dropped, no pair, truncation or clamp gate of what is left lies within
    the float32 decision error of its threshold, and no pre-clamp logit argument is negative (the clamp(min=0) gate is open everywhere)"""
    sc, ref, rec = SC.case(*c)
    fam, prim, alt, bg = c
    print("SPLATTEST admit %s: %d of %d dropped in %d rounds, live rows %.2f, min pair ratio %.3g, min gate ratio %.3g, q_min %.3g"
          % (SC.case_id(c), rec["dropped"], rec["n0"], rec["rounds"], SC.live_share(ref), ref["ratio"].min(), ref["gate_ratio"].min(), ref["q_min"]))
    assert rec["dropped"] <= SC.MAX_DROP * rec["n0"]
    assert (ref["ratio"] >= 1).all() and (ref["gate_ratio"] >= 1).all()
    assert ref["q_min"] >= 0
    assert (ref["ncov"] > 0).mean() > 0.3
    # the undecided part of the clamp(min=0) gate carries no gradient: q is within rounding of 0 only where a surfel is alone on its pixel
    assert ref["q_und"] <= 1e-9
    if fam in SC.SHEET_FAMILIES:
        assert SC.live_share(ref) >= 0.5


def test_families_reach_their_paths():
    """counted on the admitted disc scenes.  The queue family: at least 20 surfels covering 65-127 pixels (one mid-scan drain), 20 covering
    more than 128 (several), and 20 whose covered extent -- a lower bound of the screen box the backward scans 64 pixels at a time -- holds
    more than 64 pixels (a 48 x 48 image has no box wider than 48 pixels: "more than 64 pixels" is meant by area, more than one scan step).
    The stacks: about 300, 1300 and more than 3072 candidates in one 8 x 8 tile."""
    sc, ref, _ = SC.case("near", "disc", False, False)
    nc = ref["ncov"]
    box = (ref["ext"][:, 2] - ref["ext"][:, 0] + 1) * (ref["ext"][:, 3] - ref["ext"][:, 1] + 1)
    print("SPLATTEST near: covering 65-127 px %d, > 128 px %d, extent > 64 px %d, > 128 px %d"
          % (((nc > 64) & (nc < 128)).sum(), (nc > 128).sum(), ((box > 64) & (nc > 0)).sum(), ((box > 128) & (nc > 0)).sum()))
    assert ((nc > 64) & (nc < 128)).sum() >= 20 and (nc > 128).sum() >= 20 and ((box > 64) & (nc > 0)).sum() >= 20
    for fam, lo, hi in (("stack300", 280, 320), ("stack1300", 1250, 1350), ("stack3300", 3073, 3400)):
        sc, ref, _ = SC.case(fam, "disc", False, False)
        uv, _ = SC.circle_inputs(sc)
        in_tile = ((uv[:, 0] >= 0) & (uv[:, 0] < 8) & (uv[:, 1] >= 0) & (uv[:, 1] < 8)).sum()
        print("SPLATTEST %s: %d surfels project into tile (0, 0), up to %d cover one pixel" % (fam, in_tile, ref["npix_cov"].max()))
        assert lo <= in_tile <= hi
    sc, ref, _ = SC.case("grazing", "disc", False, False)
    assert (sc["p"][:, 2] < 0).sum() >= 10 and ref["ncov"].max() < 0.1 * sc["W"] * sc["H"]
    sc, ref, _ = SC.case("cropped", "disc", False, False)
    assert not (0 <= sc["K"][0, 2] < sc["W"]) and sc["K"][0, 0] != sc["K"][1, 1]


# ---- the constants of the bounds -------------------------------------------------------------------------------------------------------

def test_bound_constants_are_four_times_the_float32_reference_error():
    worst = {}
    for c in SC.ALL_CASES:
        sc, ref, _ = SC.case(*c)
        r32 = SC.run_ref(sc, c[1], c[2], c[3], grads=SC.upstream(sc), dtype=np.float32)
        assert (r32["ncov"] == ref["ncov"]).all(), "float32 and float64 cover different pixels on an admitted case: " + SC.case_id(c)
        for k, mk, kind in KINDS:
            sh = np.asarray(ref[mk]).shape
            u = float(R.unit_error(np.asarray(r32[k]).reshape(sh), np.asarray(ref[k]).reshape(sh), ref[mk], ref["logit_scale"]).max())
            worst[(c[1], kind)] = max(worst.get((c[1], kind), 0.0), u)
    for prim, cs in R.C_BOUND.items():
        for kind in (0, 1):
            print("SPLATTEST float32 reference, %s %s: %.4g units of eps32 (1 + C) mass; c = %.3g" % (prim, ("images", "gradients")[kind], worst[(prim, kind)], cs[kind]))
            # (c is 4 x the figure measured when the constants were set, rounded up by a tenth so that another numpy / BLAS build, whose float32
            # sums round differently in the last bits, does not fail this test; 6 x would mean the constants no longer follow the measurement)
            assert 4 * worst[(prim, kind)] <= cs[kind] <= 6 * worst[(prim, kind)]


# ---- the batches ---------------------------------------------------------------------------------------------------------------------------

def test_ragged_batch_and_replicated_crop_are_admitted():
    cases, b = SC.ragged_batch()
    assert cases[0] is None and b["cnt"][0] == 0
    assert 0 < b["cnt"][1] < b["cnt"][2] < b["cap"]
    assert len({tuple(w) for w in b["wh"]}) == 3 and (b["wh"][:, 0] * b["wh"][:, 1]).max() <= b["pix_stride"]
    for c in cases[1:]:
        sc, ref, rec = c
        assert (ref["ratio"] >= 1).all() and (ref["gate_ratio"] >= 1).all() and rec["dropped"] <= SC.MAX_DROP * rec["n0"]
    sc, ref, rec = SC.replicated_crop()
    assert (ref["ratio"] >= 1).all() and (ref["gate_ratio"] >= 1).all() and rec["dropped"] <= SC.MAX_DROP * rec["n0"]
    assert SC.live_share(ref) >= 0.5
    assert SC.WAVE_PER_TILE_CROPS * ((sc["W"] + 7) // 8) * ((sc["H"] + 7) // 8) >= 16384


# ---- projection and surface references ----------------------------------------------------------------------------------------------------

def _proj_inputs(n=400, seed=5):
    rng = np.random.default_rng(seed)
    pts = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    nrm = rng.standard_normal((n, 3)); nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    col = rng.uniform(0, 1, (n, 3)).astype(np.float32)
    pose = O.render_pose(0.6, [0.1, -0.2, 3.5]).astype(np.float32)
    K = SC.K_for(32, 40).astype(np.float32)
    K[0, 0] *= 3.0; K[1, 1] *= 2.6
    return pose, K, pts, nrm, col


@pytest.mark.parametrize("mode", [0, 1, 2, 5, 6])
def test_projection_reference_equals_torch_autograd_and_the_oracle(mode):
    """project_ref / project_bwd_ref in float64 against autograd on a torch restatement in every colour mode (1: torch_cpu_port.project_in_2D
    itself), and in mode 1 against oracle.project_in_2D / project_backward_dcm: values, front-face list, rows, the 12 pose sums and the
    xyzf / fslot routing, to 1e-12"""
    pose, K, pts, nrm, col = _proj_inputs()
    n = pts.shape[0]
    rx, ry = 40, 32
    ref = R.project_ref(pose, K, pts, nrm, col, mode, rx, ry)
    D = lambda a: torch.from_numpy(np.asarray(a, np.float32).astype(np.float64))
    tpose, tp, tn, tc = D(pose).requires_grad_(True), D(pts).requires_grad_(True), D(nrm).requires_grad_(True), D(col).requires_grad_(True)
    out = TP.project_in_2D(D(K), tpose, tp, tn, (rx, ry))
    p3, n3 = out["points_3d"], out["normals_3d"]
    if mode == 0:
        c3 = tc * 1.0
    else:
        c3 = tp * torch.tensor([1.0 if (mode & 3) == 2 else -1.0, 1.0, 1.0], dtype=torch.float64)       # projection.py:53-55 / :147-149
        if mode & 4:
            c3 = (c3 + 1) / 2                                                                              # rasterer.py:113-114
    close = lambda got, want, what: np.testing.assert_array_less(np.abs(np.asarray(got) - np.asarray(want)).max(initial=0.0),
                                                                 1e-12 * max(1.0, np.abs(np.asarray(want)).max(initial=0.0)), err_msg=what)
    close(ref["p_cam"], p3.detach().numpy(), "p_cam"); close(ref["n_cam"], n3.detach().numpy(), "n_cam"); close(ref["col"], c3.detach().numpy(), "col")
    # (the restatement takes eps from the dtype, the reference float32's: 1.2e-7 on a depth of about 3.5 -- compared at that size)
    assert np.abs(ref["uv"] - out["points_2d"].detach().numpy()).max() < 1e-5
    front = (n3 * p3).sum(1) < 0
    assert (ref["front"] == front.numpy()).all() and (ref["fidx"] == np.nonzero(front.numpy())[0]).all()
    close(ref["xyzf"], out["points_3d_filt"].detach().numpy(), "xyzf")
    assert (ref["fslot"][ref["fidx"]] == np.arange(ref["fidx"].shape[0])).all() and (ref["fslot"][~ref["front"]] == -1).all()
    rng = np.random.default_rng(mode)
    g_pc, g_nc, g_col, g_xf = (rng.standard_normal((n, 3)).astype(np.float32) for _ in range(4))
    nf = ref["fidx"].shape[0]
    loss = (p3 * D(g_pc)).sum() + (n3 * D(g_nc)).sum() + (c3 * D(g_col)).sum() + (out["points_3d_filt"] * D(g_xf[:nf])).sum()
    loss.backward()
    rb = R.project_bwd_ref(pose, pts, nrm, g_pc, g_nc, g_col, mode, g_xyzf=g_xf, fslot=ref["fslot"])
    close(rb["g_points"], tp.grad.numpy(), "g_points"); close(rb["g_normals"], tn.grad.numpy(), "g_normals")
    close(rb["g_pose"], tpose.grad.numpy()[:3], "g_pose")
    if mode == 0:
        close(rb["g_colors"], tc.grad.numpy(), "g_colors")
    assert (rb["mass_g_pose"] >= np.abs(rb["g_pose"]) * (1 - 1e-12)).all() and (rb["mass_g_points"] >= np.abs(rb["g_points"]) * (1 - 1e-12)).all()
    if mode == 1:
        o = O.project_in_2D(K.astype(np.float64), pose.astype(np.float64), pts.astype(np.float64), nrm.astype(np.float64), None, (rx, ry), True)
        close(ref["p_cam"], o["points_3d"], "oracle p_cam"); close(ref["col"], o["colors_3d"], "oracle col")
        assert (o["filt_idx"] == ref["fidx"]).all()
        g3 = g_pc.astype(np.float64)
        gp, gn, _, gpose = O.project_backward_dcm(pose.astype(np.float64), pts.astype(np.float64), nrm.astype(np.float64), g3, g_nc.astype(np.float64),
                                                  g_col.astype(np.float64), output_nocs=True, filt_idx=ref["fidx"], g_p3_filt=g_xf[:nf].astype(np.float64))
        close(rb["g_points"], gp, "oracle g_points"); close(rb["g_normals"], gn, "oracle g_normals"); close(rb["g_pose"], gpose[:3], "oracle g_pose")


def test_projection_reference_reproduces_g4_in_float32():
    z = gold("g4_project.npz")
    K = z["K"]
    for i in range(3):
        for mode, name in ((1, "nocs"), (0, "col")):
            t = "dcm%d_%s_" % (i, name)
            r = R.project_ref(z[t + "pose"], K, z["points"], z["normals"], z["normals"], mode, 32, 32, dtype=np.float32)
            for k, rk in (("points_3d", "p_cam"), ("normals_3d", "n_cam"), ("colors_3d", "col"), ("points_2d", "uv"), ("points_3d_filt", "xyzf")):
                assert r[rk].shape == z[t + k].shape, k
                assert np.allclose(r[rk], z[t + k], atol=1e-5), k
            assert np.allclose(r["n_cam"][r["fidx"]], z[t + "normals_3d_filt"], atol=1e-5) and np.allclose(r["col"][r["fidx"]], z[t + "colors_3d_filt"], atol=1e-5)
    # the quaternion path as the Python layer calls it: the same kernel on the quaternion's rotation matrix, colour mode 2 (no flip of x)
    q = z["quat_pose"].astype(np.float32)
    pose = np.eye(4, dtype=np.float32)
    pose[:3, :3] = O.qrot(np.broadcast_to(q[None, :4], (3, 4)), np.eye(3, dtype=np.float32)).T
    pose[:3, 3] = q[4:]
    r = R.project_ref(pose, K, z["points"], z["normals"], z["normals"], 2, 32, 32, dtype=np.float32)
    for k, rk in (("points_3d", "p_cam"), ("normals_3d", "n_cam"), ("colors_3d", "col"), ("points_2d", "uv")):
        assert np.allclose(r[rk], z["quat_" + k], atol=1e-5), k


def test_surface_references_equal_the_oracle_and_autograd():
    """surface_project_ref / _bwd_ref / latent_grad_ref in float64 against oracle.get_surface_points(_backward) and against autograd of
    x - sdf * n_hat with a constant unit normal (grid.py:56-67), to 1e-12"""
    rng = np.random.default_rng(8)
    G, Lz = 500, 3
    xyz = rng.uniform(-1, 1, (G, 3)).astype(np.float32); sdf = rng.uniform(-0.05, 0.05, (G, 1)).astype(np.float32)
    J = rng.standard_normal((G, Lz + 3)).astype(np.float32)
    D = lambda a: np.asarray(a, np.float32).astype(np.float64)
    pm, nocs, nm, idx, n_hat = O.get_surface_points(D(xyz), D(sdf), D(J[:, Lz:]), 0.03)
    rp, rn, rc = R.surface_project_ref(xyz[idx], sdf[idx, 0], J[idx, Lz:])
    assert 100 < idx.shape[0] < G
    for got, want in ((rp, pm), (rn, nm), (rc, nocs)):
        assert np.abs(got - want).max() < 1e-12
    g_pts = rng.standard_normal((idx.shape[0], 3)).astype(np.float32); g_nocs = rng.standard_normal((idx.shape[0], 3)).astype(np.float32)
    gs, gx, ms = R.surface_project_bwd_ref(nm.astype(np.float32), g_pts, g_nocs)
    g_sdf, g_xyz = O.get_surface_points_backward(D(sdf), D(n_hat.astype(np.float32)), idx, D(g_pts), D(g_nocs))
    assert np.abs(gs - g_sdf[idx, 0]).max() < 1e-12 and np.abs(gx - g_xyz[idx]).max() < 1e-12 and (ms >= np.abs(gs) - 1e-15).all()
    tx, ts = torch.from_numpy(D(xyz[idx])).requires_grad_(True), torch.from_numpy(D(sdf[idx])).requires_grad_(True)
    tn = torch.from_numpy(D(nm.astype(np.float32)))
    tpts = tx - ts * tn
    ((tpts * torch.from_numpy(D(g_pts))).sum() + (((tpts + 1) / 2) * torch.from_numpy(D(g_nocs))).sum()).backward()
    assert np.abs(gs - ts.grad.numpy()[:, 0]).max() < 1e-12 and np.abs(gx - tx.grad.numpy()).max() < 1e-12
    # the latent sum: d loss / d latent = sum over the band rows of g_sdf * d sdf / d latent
    gl, ml = R.surface_latent_grad_ref(gs.astype(np.float32), J[idx, :Lz])
    want = (D(gs.astype(np.float32))[:, None] * D(J[idx, :Lz])).sum(0)
    assert np.abs(gl - want).max() < 1e-12 and (ml >= np.abs(gl)).all()
