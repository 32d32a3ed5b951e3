"""The renderer's kernels (csrc/splat.hip, csrc/project.hip, csrc/surface.hip) against the float64 references of tests/_splat_ref.py, through
the C ABI, on the admitted inputs of tests/_splat_cases.py: every pixel of every image, every entry of the dense weights and every row of
every gradient array is judged on its own, against

    c * eps32 * (1 + C) * mass   (+ 1e-30 for float32 underflow)

with `mass` the sum of the absolute values of the terms of that element, C the primitive's depth constant (the size of the logits whose
float32 rounding every softmax weight carries) and c = 4 x the error of the reference's own arithmetic run in float32
(_splat_ref.C_BOUND; tests/test_splat_refs_cpu.py asserts the relation).  Coverage patterns must be identical: the inputs hold no
(surfel, pixel) pair, truncation or clamp gate within the float32 decision error of its threshold, so no pixel is forgiven.
Figures of one run: profiles/splat_tests_notes.md (`pytest -s` prints them, lines starting with SPLATTEST)."""
import functools

import numpy as np
import pytest
import torch

from sdflabel_amd import _lib
from tests import _splat_cases as SC
from tests import _splat_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
BINS, READY = 512, 256          # SDFR_PRIM_BINS, SDFR_PRIM_BOXES_READY (include/sdfr.h)


def T(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV, dtype=dtype)


def N(t):
    return t.detach().cpu().numpy()


P = _lib.ptr


class Scene:
    """device copies of one admitted case"""

    def __init__(self, c):
        self.c = c
        self.sc, self.ref, _ = SC.case(*c)
        fam, self.prim, self.alt, self.use_bg = c
        self.pid = R.PRIM_ID[self.prim]
        sc = self.sc
        self.W, self.H, self.n = sc["W"], sc["H"], sc["p"].shape[0]
        self.kw = SC.ref_kwargs(sc, self.prim, self.alt, self.use_bg)
        self.diam, self.C, self.cc = R.DEFAULTS[self.prim]
        self.K, self.Kinv, self.p, self.nrm, self.attr = (T(sc[k]) for k in ("K", "Kinv", "p", "n", "attr"))
        self.uv = T(self.kw["uv"]) if self.pid else None
        self.zn = T(np.array([self.kw["znorm"]], np.float32)) if self.pid else None
        self.bg = T(self.kw["bg"]) if self.use_bg else None
        self.bgl = T(np.array([self.kw["bg_logit"]], np.float32)) if self.use_bg else None
        self.ws = _lib.splat_ws(1, self.n, self.W, self.H, DEV)
        self.c_img, self.c_grad = R.C_BOUND[self.prim]
        self.ls = self.ref["logit_scale"]

    def forward(self, flags=0):
        H, W = self.H, self.W
        o = dict(color=torch.full((3, H, W), 7.0, device=DEV), mask=torch.full((1, H, W), 7.0, device=DEV),
                 depth=torch.full((1, H, W), 7.0, device=DEV), normals=torch.full((3, H, W), 7.0, device=DEV),
                 aux=torch.zeros((H * W, 4), device=DEV))
        L = _lib.lib()
        args = (P(self.K), P(self.Kinv), P(self.p), P(self.nrm), P(self.attr), P(self.uv), P(self.zn), P(self.bg), P(self.bgl), 1, self.n, None,
                W, H, self.diam, self.C)
        outs = (P(self.ws), P(o["color"]), P(o["mask"]), P(o["depth"]), P(o["normals"]), P(o["aux"]), _lib.stream_ptr())
        if self.alt:
            _lib.check(L.sdfr_splat_forward_clamp(self.pid | flags, *args, 1, self.cc, *outs), "sdfr_splat_forward_clamp")
        else:
            _lib.check(L.sdfr_splat_forward(self.pid | flags, *args, *outs), "sdfr_splat_forward")
        torch.cuda.synchronize()
        return o


@functools.lru_cache(maxsize=None)
def scene(c):
    return Scene(c)


def judge(what, got, ref, mass, c, ls, stats=None):
    """every element within c eps32 ls mass of the reference; returns the largest error in those units"""
    mass = np.asarray(mass, np.float64)
    got = np.asarray(got, np.float64).reshape(mass.shape)
    ref = np.asarray(ref, np.float64).reshape(mass.shape)
    assert np.isfinite(got).all(), what
    u = R.unit_error(got, ref, mass, ls)
    worst = float(u.max()) if u.size else 0.0
    i = np.unravel_index(int(u.argmax()), u.shape) if u.size else ()
    print("SPLATTEST %s: max error %.3g units (bound %.3g), abs %.3g" % (what, worst, c, float(np.abs(got - ref).max()) if u.size else 0.0))
    assert worst <= c, "%s: element %s is %.3g units of eps32 (1 + C) mass from the reference (bound %.3g): got %r, reference %r, mass %r" % (
        what, i, worst, c, got[i], ref[i], mass[i])
    return worst


# ---- forward images ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", SC.ALL_CASES, ids=SC.case_id)
def test_forward_images_every_pixel(c):
    """sdfr_splat_forward / sdfr_splat_forward_clamp: colour, mask, depth and normal images at every pixel; the coverage pattern (pixels
    that hold a surfel) identical; the tile-list and boxes-ready launches return the bits of the plain one."""
    s = scene(c)
    ref = s.ref
    o = s.forward()
    tag = SC.case_id(c)
    covered = ref["npix_cov"] > 0
    m = N(o["mask"]).reshape(-1)
    if s.use_bg:
        assert (m > 0).all()
    else:
        assert ((m > 0) == covered).all(), "coverage pattern differs at %d pixels" % ((m > 0) != covered).sum()
    a = N(o["aux"])
    if s.prim != "circle":
        assert ((a[:, 2] > 0) == (covered | s.use_bg)).all()
    judge(tag + " color", N(o["color"]), ref["color"], ref["mass_color"], s.c_img, s.ls)
    judge(tag + " mask", m, ref["mask"], ref["mask"].reshape(-1), s.c_img, s.ls)
    judge(tag + " depth", N(o["depth"]), ref["depth"], ref["mass_depth"], s.c_img, s.ls)
    judge(tag + " normals", N(o["normals"]), ref["normals"], ref["mass_normals"], s.c_img, s.ls)
    if not s.alt:
        for flags in (BINS, BINS | READY):          # (READY: the workspace holds the boxes and lists the BINS call before it built)
            o2 = s.forward(flags)
            for k in ("color", "mask", "depth", "normals", "aux"):
                assert torch.equal(o[k], o2[k]), (k, flags)


# ---- dense weights -------------------------------------------------------------------------------------------------------------------

def _dense_weights(s, o):
    rows = s.n + (1 if s.use_bg else 0)
    Wt = torch.zeros((rows, s.H * s.W), device=DEV)
    L = _lib.lib()
    args = (s.pid, P(s.K), P(s.Kinv), P(s.p), P(s.nrm), P(s.uv), P(s.zn), P(s.bgl), 1, s.n, None, s.W, s.H, s.diam, s.C)
    if s.alt:
        _lib.check(L.sdfr_splat_weights_clamp(*args, 1, s.cc, P(o["aux"]), P(Wt), _lib.stream_ptr()), "sdfr_splat_weights_clamp")
    else:
        _lib.check(L.sdfr_splat_weights(*args, P(o["aux"]), P(Wt), _lib.stream_ptr()), "sdfr_splat_weights")
    torch.cuda.synchronize()
    return Wt


DENSE_CASES = [c for c in SC.ALL_CASES if c[0] != "centred_64"]


@pytest.mark.parametrize("c", DENSE_CASES, ids=SC.case_id)
def test_dense_weights_every_entry(c):
    """sdfr_splat_weights(_clamp), i.e. the per-pixel softmax state `aux` of the forward applied to every (surfel, pixel) pair: each entry
    within the bound of its own size, the set of non-zero entries identical"""
    s = scene(c)
    o = s.forward()
    Wt = N(_dense_weights(s, o))
    ref = SC.run_ref(s.sc, s.prim, s.alt, s.use_bg, want_W=True)["W"]
    # (a float64 weight below float32's range is a covered pair all the same: the pattern is compared on the coverage, through ncov)
    nz = (Wt[:s.n] > 0).sum(axis=1)
    assert ((nz <= s.ref["ncov"]) & (nz >= (ref[:s.n] >= 1e-37).sum(axis=1))).all()
    assert not ((Wt > 0) & (ref == 0)).any()
    judge(SC.case_id(c) + " weights", Wt, ref, ref, s.c_img, s.ls)


@pytest.mark.parametrize("c", [c for c in DENSE_CASES if c[0] in ("centred_small", "partial", "near", "narrow")], ids=SC.case_id)
def test_dense_weights_backward_every_row(c):
    """sdfr_splat_weights_backward(_clamp) with a dense upstream gradient and the caller's per-pixel sum, as the Python layer forms it"""
    s = scene(c)
    o = s.forward()
    Wt = _dense_weights(s, o)
    rng = np.random.default_rng(5)
    gW = rng.standard_normal(tuple(Wt.shape)).astype(np.float32)
    tg = T(gW)
    wsum = (Wt * tg).sum(0).contiguous()
    g_p = torch.zeros((s.n, 3), device=DEV); g_n = torch.zeros((s.n, 3), device=DEV)
    L = _lib.lib()
    args = (s.pid, P(s.K), P(s.Kinv), P(s.p), P(s.nrm), P(s.uv), P(s.zn), int(s.use_bg), 1, s.n, None, s.W, s.H, s.diam, s.C)
    tail = (P(o["aux"]), P(tg), P(wsum), P(g_p), P(g_n), _lib.stream_ptr())
    if s.alt:
        _lib.check(L.sdfr_splat_weights_backward_clamp(*args, 1, s.cc, *tail), "sdfr_splat_weights_backward_clamp")
    else:
        _lib.check(L.sdfr_splat_weights_backward(*args, *tail), "sdfr_splat_weights_backward")
    torch.cuda.synchronize()
    ref = SC.run_ref(s.sc, s.prim, s.alt, s.use_bg, gW=gW)
    tag = SC.case_id(c) + " dense"
    # the caller's own per-pixel sum over the kernel's weights: each weight within c_img of its size, plus the float32 sum over the rows (one unit)
    judge(tag + " wsum", N(wsum), ref["wsum"], ref["mass_wsum"], s.c_img + 1.0, s.ls)
    judge(tag + " g_p", N(g_p), ref["g_p"], ref["mass_g_p"], s.c_grad, s.ls)
    judge(tag + " g_n", N(g_n), ref["g_n"], ref["mass_g_n"], s.c_grad, s.ls)


# ---- backward ------------------------------------------------------------------------------------------------------------------------

def _backward(s, o, grads):
    g_p = torch.full((s.n, 3), 7.0, device=DEV); g_n = torch.full((s.n, 3), 7.0, device=DEV); g_a = torch.full((s.n, 3), 7.0, device=DEV)
    tg = [T(g) if g is not None else None for g in grads]
    _lib.check(_lib.lib().sdfr_splat_backward(s.pid, P(s.K), P(s.Kinv), P(s.p), P(s.nrm), P(s.attr), P(s.uv), P(s.zn), P(s.bg), P(s.bgl), 1, s.n, None,
                                              s.W, s.H, s.diam, s.C, P(o["aux"]), P(o["color"]), P(o["mask"]), P(o["depth"]), P(o["normals"]),
                                              P(tg[0]), P(tg[1]), P(tg[2]), P(tg[3]), P(g_p), P(g_n), P(g_a), _lib.stream_ptr()), "sdfr_splat_backward")
    torch.cuda.synchronize()
    return g_p, g_n, g_a


@pytest.mark.parametrize("c", SC.DISC_CASES + SC.CIRCLE_CASES, ids=SC.case_id)
def test_backward_every_row(c):
    """sdfr_splat_backward: every row of g_p, g_n and g_attr, all four image gradients flowing"""
    s = scene(c)
    ref = s.ref
    o = s.forward()
    g_p, g_n, g_a = _backward(s, o, SC.upstream(s.sc))
    tag = SC.case_id(c)
    live = SC.live_share(ref)
    print("SPLATTEST %s: %d surfels, %.0f %% live rows, %d cover more than 64 pixels" % (tag, s.n, 100 * live, (ref["ncov"] > 64).sum()))
    judge(tag + " g_p", N(g_p), ref["g_p"], ref["mass_g_p"], s.c_grad, s.ls)
    judge(tag + " g_n", N(g_n), ref["g_n"], ref["mass_g_n"], s.c_grad, s.ls)
    judge(tag + " g_attr", N(g_a), ref["g_attr"], ref["mass_g_attr"], s.c_grad, s.ls)


@pytest.mark.parametrize("fam", ["centred_small", "partial", "near", "stack1300"])
def test_backward_x_with_kscale_and_handed_over_boxes(fam):
    """sdfr_splat_backward_x: the colour gradient arrives un-normalised with a per-crop factor; with the forward's screen boxes handed over
    and without, the same bits; every row against the reference of the scaled gradient"""
    s = scene((fam, "disc", False, False))
    o = s.forward()
    gC = SC.upstream(s.sc, salt=3)[0]
    k = np.float32(0.37)
    ks = T(np.array([[k, 5.0]], np.float32))
    tg = T(gC)
    res = []
    for boxes in (None, s.ws):
        g_p = torch.full((s.n, 3), 7.0, device=DEV); g_n = torch.full((s.n, 3), 7.0, device=DEV); g_a = torch.full((s.n, 3), 7.0, device=DEV)
        _lib.check(_lib.lib().sdfr_splat_backward_x(P(s.K), P(s.Kinv), P(s.p), P(s.nrm), P(s.attr), 1, s.n, None, s.W, s.H, None, s.W * s.H, s.diam, s.C,
                                                    P(o["aux"]), P(o["color"]), P(tg), P(ks), P(g_p), P(g_n), P(g_a), P(boxes), _lib.stream_ptr()),
                   "sdfr_splat_backward_x")
        torch.cuda.synchronize()
        res.append((g_p, g_n, g_a))
    for a, b in zip(*res):
        assert torch.equal(a, b)
    # the plain entry point on the product the kernel forms on load: the same bits
    plain = _backward(s, o, ((gC * k).astype(np.float32), None, None, None))
    for a, b in zip(res[0], plain):
        assert torch.equal(a, b)
    # (the reference takes float32 inputs: the exact product is handed over in two float32 parts)
    hi = (gC.astype(np.float64) * float(k)).astype(np.float32)
    lo = (gC.astype(np.float64) * float(k) - hi).astype(np.float32)
    r1 = SC.run_ref(s.sc, "disc", grads=(hi, None, None, None))
    r2 = SC.run_ref(s.sc, "disc", grads=(lo, None, None, None))
    tag = fam + "-disc backward_x"
    # gates are decided by the forward alone, so the backward is linear in the upstream gradient: r1 + r2 is the reference of the product
    for key, got in (("g_p", res[0][0]), ("g_n", res[0][1]), ("g_attr", res[0][2])):
        judge(tag + " " + key, N(got), r1[key] + r2[key], r1["mass_" + key], s.c_grad, s.ls)


# ---- ragged extents ------------------------------------------------------------------------------------------------------------------

def test_ragged_batch_forward_and_backward():
    """sdfr_splat_forward_r / sdfr_splat_backward_r: an empty crop (zeros), a partly filled one and a full one, each with its own image size
    and intrinsics, every pixel and row; tile lists and boxes-ready give the same bits"""
    cases = list(SC.RAGGED_BATCH)
    _, bt = SC.ragged_batch()
    scs = [scene(c) if c else None for c in cases]
    B, cap, PS, tiles_cap = len(cases), bt["cap"], bt["pix_stride"], bt["tiles_cap"]
    K, Ki, p, nr, at, cnt, wh = (bt[k] for k in ("K", "Kinv", "p", "n", "attr", "cnt", "wh"))
    tK, tKi, tp, tn, ta, tc, twh = T(K), T(Ki), T(p), T(nr), T(at), T(cnt, torch.int32), T(wh, torch.int32)
    L = _lib.lib()
    ws = torch.zeros((int(L.sdfr_splat_ws_words_r(B, cap, tiles_cap)),), dtype=torch.int32, device=DEV)

    def fwd(flags):
        o = dict(color=torch.full((B, 3, PS), 7.0, device=DEV), mask=torch.full((B, 1, PS), 7.0, device=DEV), depth=torch.full((B, 1, PS), 7.0, device=DEV),
                 normals=torch.full((B, 3, PS), 7.0, device=DEV), aux=torch.zeros((B, PS, 4), device=DEV))
        _lib.check(L.sdfr_splat_forward_r(flags, P(tK), P(tKi), P(tp), P(tn), P(ta), B, cap, P(tc), P(twh), PS, tiles_cap, 0.04, 150.0, P(ws),
                                          P(o["color"]), P(o["mask"]), P(o["depth"]), P(o["normals"]), P(o["aux"]), _lib.stream_ptr()), "sdfr_splat_forward_r")
        torch.cuda.synchronize()
        return o

    o = fwd(0)
    for flags in (BINS, BINS | READY):
        o2 = fwd(flags)
        for b in range(B):
            npx = int(wh[b, 0] * wh[b, 1])
            for k in ("color", "mask", "depth", "normals"):
                assert torch.equal(o[k][b, :, :npx], o2[k][b, :, :npx]), (k, b, flags)
    gr = {k: np.zeros((B, c, PS), np.float32) for k, c in (("color", 3), ("mask", 1), ("depth", 1), ("normals", 3))}
    ups = [None] + [SC.upstream(scs[b].sc) for b in (1, 2)]
    for b in (1, 2):
        npx = int(wh[b, 0] * wh[b, 1])
        for k, g in zip(("color", "mask", "depth", "normals"), ups[b]):
            gr[k][b, :, :npx] = g.reshape(g.shape[0], -1)
    gr["color"][0] = 1.0
    tg = {k: T(v) for k, v in gr.items()}
    g_p = torch.full((B, cap, 3), 7.0, device=DEV); g_n = torch.full((B, cap, 3), 7.0, device=DEV); g_a = torch.full((B, cap, 3), 7.0, device=DEV)
    _lib.check(L.sdfr_splat_backward_r(P(tK), P(tKi), P(tp), P(tn), P(ta), B, cap, P(tc), P(twh), PS, 0.04, 150.0, P(o["aux"]), P(o["color"]), P(o["mask"]),
                                       P(o["depth"]), P(o["normals"]), P(tg["color"]), P(tg["mask"]), P(tg["depth"]), P(tg["normals"]), P(g_p), P(g_n), P(g_a),
                                       _lib.stream_ptr()), "sdfr_splat_backward_r")
    torch.cuda.synchronize()
    # the empty crop: zero images over its 16 x 16 extent, no gradient row written
    for k in ("color", "mask", "depth", "normals"):
        assert (N(o[k][0, :, :256]) == 0).all(), k
    assert (N(g_p[0]) == 7).all() and (N(g_a[0]) == 7).all()
    for b in (1, 2):
        s, ref = scs[b], scs[b].ref
        npx = s.W * s.H
        tag = "ragged crop %d (%s)" % (b, cases[b][0])
        assert ((N(o["mask"][b, 0, :npx]) > 0) == (ref["npix_cov"] > 0)).all()
        judge(tag + " color", N(o["color"][b, :, :npx]), ref["color"], ref["mass_color"], s.c_img, s.ls)
        judge(tag + " depth", N(o["depth"][b, :, :npx]), ref["depth"], ref["mass_depth"], s.c_img, s.ls)
        judge(tag + " normals", N(o["normals"][b, :, :npx]), ref["normals"], ref["mass_normals"], s.c_img, s.ls)
        for key, got in (("g_p", g_p), ("g_n", g_n), ("g_attr", g_a)):
            judge(tag + " " + key, N(got[b, :s.n]), ref[key], ref["mass_" + key], s.c_grad, s.ls)
            assert (N(got[b, s.n:]) == 7).all()


# ---- the wave-per-tile launch geometry ---------------------------------------------------------------------------------------------------

def test_wave_per_tile_geometry_on_replicated_crops():
    """from 16 384 tiles per launch the forward runs one wave per tile: 1024 copies of a 32 x 32 crop (16 tiles each), judged on three of
    them and bit-equal across all copies (tests/_splat_cases.py::replicated_crop)"""
    sc, ref, _ = SC.replicated_crop()
    c_img, ls = R.C_BOUND["disc"][0], ref["logit_scale"]
    B, n, H, W = SC.WAVE_PER_TILE_CROPS, sc["p"].shape[0], sc["H"], sc["W"]
    rep = lambda a: T(a).unsqueeze(0).expand(B, *a.shape).contiguous()
    tK, tKi, tp, tn, ta = (rep(sc[k]) for k in ("K", "Kinv", "p", "n", "attr"))
    color = torch.empty((B, 3, H * W), device=DEV); mask = torch.empty((B, 1, H * W), device=DEV); depth = torch.empty((B, 1, H * W), device=DEV)
    nimg = torch.empty((B, 3, H * W), device=DEV); aux = torch.empty((B, H * W, 4), device=DEV)
    ws = _lib.splat_ws(B, n, W, H, DEV)
    _lib.check(_lib.lib().sdfr_splat_forward(BINS, P(tK), P(tKi), P(tp), P(tn), P(ta), None, None, None, None, B, n, None, W, H, 0.04, 150.0, P(ws),
                                             P(color), P(mask), P(depth), P(nimg), P(aux), _lib.stream_ptr()), "sdfr_splat_forward")
    torch.cuda.synchronize()
    for img in (color, mask, depth, nimg):
        assert torch.equal(img, img[:1].expand_as(img))
    for b in (0, 511, 1023):
        assert ((N(mask[b, 0]) > 0) == (ref["npix_cov"] > 0)).all()
        judge("wave-per-tile crop %d color" % b, N(color[b]), ref["color"], ref["mass_color"], c_img, ls)
        judge("wave-per-tile crop %d depth" % b, N(depth[b]), ref["depth"], ref["mass_depth"], c_img, ls)
        judge("wave-per-tile crop %d normals" % b, N(nimg[b]), ref["normals"], ref["mass_normals"], c_img, ls)


# ---- projection ----------------------------------------------------------------------------------------------------------------------

C_PROJ = 4.0        # units of eps32 * mass: a projected coordinate is three products, two sums and the translation -- at most six roundings of
                    # half an eps32, each relative to a partial sum below the mass -- so 3 eps32 mass bounds it; the quotient of uv adds one more
                    # on each operand


@functools.lru_cache(maxsize=None)
def _proj_case(n=1500, res=(40, 32)):
    rng = np.random.default_rng(77)
    pts = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    nrm = rng.standard_normal((n, 3)); nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    col = rng.uniform(0, 1, (n, 3)).astype(np.float32)
    c, s_ = np.cos(0.6), np.sin(0.6)
    pose = np.eye(4, dtype=np.float32)
    pose[:3, :3] = np.array([[c, 0, s_], [0, -1, 0], [-s_, 0, c]], np.float32)
    pose[:3, 3] = [0.1, -0.2, 3.5]
    from sdflabel_amd.fixtures import K_for
    K = K_for(res[1], res[0]).astype(np.float32)
    K[0, 0] *= 3.0; K[1, 1] *= 2.6           # wide enough that some projections leave the image: the clamps of uv
    r = R.project_ref(pose, K, pts, nrm, col, 1, res[0], res[1])
    keep = (r["front_ratio"] >= 1) & (r["uv_ratio"] >= 1)
    assert keep.mean() >= 0.98
    return pose, K, pts[keep], nrm[keep], col[keep], res


@pytest.mark.parametrize("mode", [0, 1, 2, 5, 6])
def test_project_forward_and_backward_every_row(mode):
    """sdfr_project_dcm / sdfr_project_dcm_bwd in every colour mode: camera-frame points and normals, colours, clamped projections, the
    front-face list with its xyzf / fslot routing (exact), and the backward's rows and 12 pose sums"""
    pose, K, pts, nrm, col, (rx, ry) = _proj_case()
    n = pts.shape[0]
    ref = R.project_ref(pose, K, pts, nrm, col, mode, rx, ry)
    assert 0.3 < ref["front"].mean() < 0.7 and ((ref["uv"] == -1) | (ref["uv"][:, :1] == rx)).any()
    tpose, tK, tp, tn, tc = T(pose), T(K), T(pts), T(nrm), T(col)
    o = {k: torch.full((n, 3), 7.0, device=DEV) for k in ("p_cam", "n_cam", "col", "xyzf")}
    uv = torch.full((n, 2), 7.0, device=DEV)
    fidx = torch.full((n,), -5, dtype=torch.int32, device=DEV); fslot = torch.full((n,), -5, dtype=torch.int32, device=DEV)
    fcnt = torch.zeros((1,), dtype=torch.int32, device=DEV)
    L = _lib.lib()
    _lib.check(L.sdfr_project_dcm(P(tpose), P(tK), P(tp), P(tn), P(tc), 1, n, None, mode, rx, ry, P(o["p_cam"]), P(o["n_cam"]), P(o["col"]), P(uv),
                                  P(fidx), P(fcnt), P(o["xyzf"]), P(fslot), _lib.stream_ptr()), "sdfr_project_dcm")
    torch.cuda.synchronize()
    tag = "project mode %d" % mode
    judge(tag + " p_cam", N(o["p_cam"]), ref["p_cam"], ref["mass_p_cam"], C_PROJ, 1.0)
    judge(tag + " n_cam", N(o["n_cam"]), ref["n_cam"], ref["mass_n_cam"], C_PROJ, 1.0)
    judge(tag + " col", N(o["col"]), ref["col"], np.abs(ref["col"]) + (1.0 if mode & 4 else 0.0), 1.0, 1.0)
    aK = np.abs(K.astype(np.float64))
    ah = ref["mass_p_cam"] @ aK.T
    hz = np.abs(ref["p_cam"] @ K.astype(np.float64).T)[:, 2:]
    judge(tag + " uv", N(uv), ref["uv"], ah[:, :2] / hz + np.abs(ref["uv"]) * ah[:, 2:] / hz, C_PROJ, 1.0)
    nf = int(N(fcnt)[0])
    assert nf == ref["fidx"].shape[0]
    assert (N(fidx)[:nf] == ref["fidx"]).all() and (N(fslot) == ref["fslot"]).all()
    assert torch.equal(o["xyzf"][:nf], o["p_cam"][T(ref["fidx"], torch.int64)])
    # backward
    rng = np.random.default_rng(mode + 3)
    g_pc, g_nc, g_col, g_xf = (rng.standard_normal((n, 3)).astype(np.float32) for _ in range(4))
    g_xf[nf:] = 0
    rb = R.project_bwd_ref(pose, pts, nrm, g_pc, g_nc, g_col, mode, g_xyzf=g_xf, fslot=ref["fslot"])
    g_points = torch.full((n, 3), 7.0, device=DEV); g_normals = torch.full((n, 3), 7.0, device=DEV); g_colors = torch.full((n, 3), 7.0, device=DEV)
    g_pose = torch.full((16,), 7.0, device=DEV)
    tg = [T(g) for g in (g_pc, g_nc, g_col, g_xf)]
    _lib.check(L.sdfr_project_dcm_bwd(P(tpose), P(tp), P(tn), P(tg[0]), P(tg[1]), P(tg[2]), 1, n, None, mode, P(g_points), P(g_normals), P(g_colors),
                                      P(g_pose), P(tg[3]), P(fslot), _lib.stream_ptr()), "sdfr_project_dcm_bwd")
    torch.cuda.synchronize()
    judge(tag + " g_points", N(g_points), rb["g_points"], rb["mass_g_points"], C_PROJ, 1.0)
    judge(tag + " g_normals", N(g_normals), rb["g_normals"], rb["mass_g_normals"], C_PROJ, 1.0)
    if mode == 0:
        assert torch.equal(g_colors, tg[2])
    # a pose sum adds n terms of two products each: per thread ceil(n / 1024) sequential additions, 6 across the wave, 16 across the waves --
    # each one rounding of half an eps32 relative to a partial sum below the mass
    c_pose = 0.5 * (-(-n // 1024) + 6 + 16 + 3)
    gp = N(g_pose).reshape(4, 4)
    judge(tag + " g_pose", gp[:3], rb["g_pose"], rb["mass_g_pose"], c_pose, 1.0)
    assert (gp[3] == 0).all()


# ---- iso-surface projection ----------------------------------------------------------------------------------------------------------------

def test_surface_project_backward_and_latent_gradient():
    """sdfr_surface_project, sdfr_surface_project_bwd and sdfr_surface_latent_grad on two crops with different band sizes"""
    rng = np.random.default_rng(123)
    B, G, cap, NI, Lz = 2, 700, 300, 6, 3
    cnt = np.array([300, 211], np.int32)
    xyz = rng.uniform(-1, 1, (B * G, 3)).astype(np.float32)
    sdf = rng.uniform(-0.03, 0.03, (B * G,)).astype(np.float32)
    idx = np.stack([np.sort(rng.choice(G, cap, replace=False)) for _ in range(B)]).astype(np.int32)
    J = rng.standard_normal((B, cap, NI)).astype(np.float32)
    L = _lib.lib()
    t = dict(xyz=T(xyz), sdf=T(sdf), idx=T(idx, torch.int32), cnt=T(cnt, torch.int32), J=T(J))
    pts = torch.full((B, cap, 3), 7.0, device=DEV); nocs = torch.full((B, cap, 3), 7.0, device=DEV); nh = torch.full((B, cap, 3), 7.0, device=DEV)
    _lib.check(L.sdfr_surface_project(P(t["xyz"]), 3, P(t["sdf"]), G, B, P(t["idx"]), cap, P(t["cnt"]), P(t["J"]), NI, Lz, P(pts), P(nocs), P(nh),
                                      _lib.stream_ptr()), "sdfr_surface_project")
    torch.cuda.synchronize()
    g_pts = rng.standard_normal((B, cap, 3)).astype(np.float32); g_nocs = rng.standard_normal((B, cap, 3)).astype(np.float32)
    g_sdf = torch.full((B * G,), 7.0, device=DEV); g_xyz = torch.full((B * G, 3), 7.0, device=DEV)
    tgp, tgn = T(g_pts), T(g_nocs)
    _lib.check(L.sdfr_surface_project_bwd(P(tgp), P(tgn), P(nh), G, B, P(t["idx"]), cap, P(t["cnt"]), P(g_sdf), P(g_xyz), _lib.stream_ptr()),
               "sdfr_surface_project_bwd")
    g_latn = torch.full((B, Lz), 7.0, device=DEV)
    _lib.check(L.sdfr_surface_latent_grad(P(tgp), P(tgn), P(nh), P(t["J"]), NI, Lz, B, cap, P(t["cnt"]), P(g_latn), _lib.stream_ptr()),
               "sdfr_surface_latent_grad")
    torch.cuda.synchronize()
    nh_gpu = N(nh)
    for b in range(B):
        c = int(cnt[b])
        rows = b * G + idx[b, :c]
        rp, rn, rc = R.surface_project_ref(xyz[rows], sdf[rows], J[b, :c, Lz:Lz + 3])
        tag = "surface crop %d" % b
        judge(tag + " normals", nh_gpu[b, :c], rn, np.ones_like(rn), 4.0, 1.0)             # three squares, two sums, a root, a quotient
        judge(tag + " points", N(pts)[b, :c], rp, np.abs(xyz[rows]) + np.abs(sdf[rows])[:, None], 6.0, 1.0)
        judge(tag + " nocs", N(nocs)[b, :c], rc, (np.abs(rp) + 1) / 2 + np.abs(xyz[rows]) + np.abs(sdf[rows])[:, None], 6.0, 1.0)
        # the backward takes the kernel's own float32 unit normals as its input
        gs, gx, ms = R.surface_project_bwd_ref(nh_gpu[b, :c], g_pts[b, :c], g_nocs[b, :c])
        judge(tag + " g_sdf", N(g_sdf)[rows], gs, ms, 3.0, 1.0)
        judge(tag + " g_xyz", N(g_xyz)[rows], gx, np.abs(g_pts[b, :c]) + np.abs(g_nocs[b, :c]) / 2, 1.0, 1.0)
        other = np.setdiff1d(np.arange(b * G, (b + 1) * G), rows)
        assert (N(g_sdf)[other] == 0).all() and (N(g_xyz)[other] == 0).all()
        gl, ml = R.surface_latent_grad_ref(gs, J[b, :c, :Lz])
        # (g_sdf itself carries 3 roundings; the sum over up to 300 rows any order: a tree of depth <= 5 + 6 + 4)
        judge(tag + " g_latn", N(g_latn)[b], gl, ml, 3.0 + 0.5 * 16, 1.0)


@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("mode", [1, 2, 5, 6])
def test_surfels_forward_against_the_composition_of_the_references(mode, ragged):
    """sdfr_surfels_forward(_r): band rows -> surfels -> camera frame -> front-face list -> screen boxes in one launch, against
    surface_project_ref followed by project_ref; the boxes and tile lists it leaves must serve sdfr_splat_forward(_r) with boxes-ready to the
    bits of a forward that builds its own"""
    rng = np.random.default_rng(40 + mode)
    B, G, cap, NI, Lz, H, W = 2, 900, 400, 6, 3, 24, 32
    cnt = np.array([400, 277], np.int32)
    xyz = rng.uniform(-0.7, 0.7, (B * G, 3)).astype(np.float32)
    sdf = rng.uniform(-0.03, 0.03, (B * G,)).astype(np.float32)
    idx = np.stack([np.sort(rng.choice(G, cap, replace=False)) for _ in range(B)]).astype(np.int32)
    J = rng.standard_normal((B, cap, NI)).astype(np.float32)
    from oracle import sdf_oracle as O
    pose = np.stack([O.render_pose(0.6, [0.0, 0.0, 3.5]), O.render_pose(-0.4, [0.1, -0.1, 3.0])]).astype(np.float32)
    K = np.stack([SC.K_for(H, W), SC.K_for(H, W)]).astype(np.float32)
    wh = np.array([[W, H], [W - 7, H - 3]], np.int32)
    L = _lib.lib()
    t = dict(xyz=T(xyz), sdf=T(sdf), idx=T(idx, torch.int32), cnt=T(cnt, torch.int32), J=T(J), pose=T(pose), K=T(K), wh=T(wh, torch.int32))
    f3 = lambda: torch.full((B, cap, 3), 7.0, device=DEV)
    o = {k: f3() for k in ("points", "normals", "p_cam", "n_cam", "col", "xyzf")}
    fidx = torch.full((B, cap), -5, dtype=torch.int32, device=DEV); fslot = torch.full((B, cap), -5, dtype=torch.int32, device=DEV)
    fcnt = torch.zeros((B,), dtype=torch.int32, device=DEV)
    tiles_cap = ((W + 7) // 8) * ((H + 7) // 8)
    ws = torch.zeros((int(L.sdfr_splat_ws_words_r(B, cap, tiles_cap)) if ragged else int(L.sdfr_splat_ws_words(B, cap, W, H)),), dtype=torch.int32, device=DEV)
    head = (P(t["xyz"]), 3, P(t["sdf"]), G, P(t["idx"]), P(t["J"]), NI, Lz, P(t["pose"]), P(t["K"]), B, cap, P(t["cnt"]), mode | 8)
    tail = (0.04, P(o["points"]), P(o["normals"]), P(o["p_cam"]), P(o["n_cam"]), P(o["col"]), P(fidx), P(fcnt), P(o["xyzf"]), P(fslot), P(ws), _lib.stream_ptr())
    if ragged:
        _lib.check(L.sdfr_surfels_forward_r(*head, P(t["wh"]), tiles_cap, *tail), "sdfr_surfels_forward_r")
    else:
        _lib.check(L.sdfr_surfels_forward(*head, W, H, *tail), "sdfr_surfels_forward")
    torch.cuda.synchronize()
    for b in range(B):
        c = int(cnt[b])
        rows = b * G + idx[b, :c]
        rp, rn, _ = R.surface_project_ref(xyz[rows], sdf[rows], J[b, :c, Lz:Lz + 3])
        tag = "surfels_forward%s mode %d crop %d" % ("_r" if ragged else "", mode, b)
        judge(tag + " normals", N(o["normals"])[b, :c], rn, np.ones_like(rn), 4.0, 1.0)
        judge(tag + " points", N(o["points"])[b, :c], rp, np.abs(xyz[rows]) + np.abs(sdf[rows])[:, None], 6.0, 1.0)
        # the projection takes the kernel's own float32 surfels as its input
        gp, gn = N(o["points"])[b, :c], N(o["normals"])[b, :c]
        ref = R.project_ref(pose[b], K[b], gp, gn, None, mode, int(wh[b, 0]) if ragged else W, int(wh[b, 1]) if ragged else H)
        ok = ref["front_ratio"] >= 1
        assert ok.mean() > 0.98
        judge(tag + " p_cam", N(o["p_cam"])[b, :c], ref["p_cam"], ref["mass_p_cam"], C_PROJ, 1.0)
        judge(tag + " n_cam", N(o["n_cam"])[b, :c], ref["n_cam"], ref["mass_n_cam"], C_PROJ, 1.0)
        judge(tag + " col", N(o["col"])[b, :c], ref["col"], np.abs(ref["col"]) + (1.0 if mode & 4 else 0.0), 1.0, 1.0)
        front = N(fslot)[b, :c] >= 0
        assert (front == ref["front"])[ok].all()
        nf = int(N(fcnt)[b])
        assert nf == front.sum() and (N(fidx)[b, :nf] == np.nonzero(front)[0]).all()
        assert (N(fslot)[b, :c][front] == np.arange(nf)).all()
        assert torch.equal(o["xyzf"][b, :nf], o["p_cam"][b][T(np.nonzero(front)[0], torch.int64)])
    # the boxes and lists left in the workspace: boxes-ready forward == a forward that builds its own
    PS = H * W
    attr = o["col"] if mode & 4 else (o["col"] + 1) / 2
    Kinv = torch.linalg.inv(t["K"].double()).float().contiguous()
    def fwd(flags, wsx):
        im = dict(color=torch.full((B, 3, PS), 7.0, device=DEV), mask=torch.full((B, 1, PS), 7.0, device=DEV), depth=torch.full((B, 1, PS), 7.0, device=DEV),
                  normals=torch.full((B, 3, PS), 7.0, device=DEV), aux=torch.zeros((B, PS, 4), device=DEV))
        common = (P(t["K"]), P(Kinv), P(o["p_cam"]), P(o["n_cam"]), P(attr))
        outs = (P(wsx), P(im["color"]), P(im["mask"]), P(im["depth"]), P(im["normals"]), P(im["aux"]), _lib.stream_ptr())
        if ragged:
            _lib.check(L.sdfr_splat_forward_r(flags, *common, B, cap, P(t["cnt"]), P(t["wh"]), PS, tiles_cap, 0.04, 150.0, *outs), "sdfr_splat_forward_r")
        else:
            _lib.check(L.sdfr_splat_forward(flags, *common, None, None, None, None, B, cap, P(t["cnt"]), W, H, 0.04, 150.0, *outs), "sdfr_splat_forward")
        torch.cuda.synchronize()
        return im
    a = fwd(BINS | READY, ws)
    b2 = fwd(0, torch.zeros_like(ws))
    for b in range(B):
        npx = int(wh[b, 0] * wh[b, 1]) if ragged else PS
        for k in ("color", "mask", "depth", "normals"):
            assert torch.equal(a[k][b, :, :npx], b2[k][b, :, :npx]), (k, b)
        assert float(a["mask"][b, 0, :npx].sum()) > 20
