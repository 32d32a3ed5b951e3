"""The CSS network's output head on the GPU (csrc/css_head.hip through sdflabel_amd.css and networks.resnet_css) against the float64
restatement of tests/_css_ref.py, which tests/test_css_cpu.py pins to golden G20 (recorded from the reference's own module).  The
tolerances are the derived ones of _css_ref; figures are printed before they are asserted."""
import numpy as np
import pytest
import torch

import sdflabel_amd
from sdflabel_amd import _lib, css
from tests import _css_ref as R
from tests._util import ASSET, gold

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HEADS = ("u", "v", "w", "mask")
ALL = ("uvw_sm", "uvw_sm_masked", "mask", "mask_sm", "u", "v", "w")


@pytest.fixture(scope="module")
def z():
    return gold("g20_css_head.npz")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def run(x, wts, logprobs=True):
    """x: {'x_u', ...} numpy, wts: {'u': (W, b), ...} numpy -> the kernel's outputs as numpy"""
    out = css.css_head(dev(x["x_u"]), dev(x["x_v"]), dev(x["x_w"]), dev(x["x_mask"]), {h: (dev(w), dev(b)) for h, (w, b) in wts.items()},
                       logprobs=logprobs)
    assert all(not t.requires_grad for t in out.values())
    return {k: t.cpu().numpy() for k, t in out.items()}


def synthetic(B, H, W, seed=1, scale=1.0):
    """non-negative features (the head's inputs follow a ReLU) and normal weights of the given seed"""
    g = np.random.default_rng(seed)
    x = {k: (np.abs(g.standard_normal((B, 64, H, W))) * scale).astype(np.float32) for k in ("x_u", "x_v", "x_w", "x_mask")}
    wts = {h: ((g.standard_normal((256, 64)) * 0.09).astype(np.float32), (g.uniform(-0.125, 0.125, 256)).astype(np.float32)) for h in ("u", "v", "w")}
    wts["v"] = (wts["v"][0] * 0.05, wts["v"][1] * 0.05)                                  # one head in the mixing regime
    wm = (g.standard_normal((2, 64)) * 0.1).astype(np.float32)
    gap = np.sort(np.einsum("c,bchw->bhw", (wm[1] - wm[0]).astype(np.float64), x["x_mask"].astype(np.float64)).ravel())
    n = gap.size                                       # the boundary goes half way between the two middle pixels: half of them are foreground
    wts["mask"] = (wm, np.array([0.0, -(gap[n // 2 - 1] + gap[n // 2]) / 2 if n > 1 else 0.05 - gap[0]], np.float32))
    return x, wts


def test_golden_features_through_the_head_and_the_latent(z):
    x = {k: z[k] for k in ("x_u", "x_v", "x_w", "x_mask")}
    wts = {h: (z["w_" + h], z["b_" + h]) for h in HEADS}
    got = run(x, wts)
    out, tol, unsure = R.head(x["x_u"], x["x_v"], x["x_w"], x["x_mask"], wts)
    got["latent"] = css.css_latent(dev(z["x4"]), dev(z["w_lat"]), dev(z["b_lat"])).cpu().numpy()
    out["latent"], tol["latent"] = R.latent(z["x4"], z["w_lat"], z["b_lat"])
    R.compare(got, out, tol, unsure, label="g20:")
    # second check: the kernel's error on uvw_sm against the reference's own recorded float32 error (same 65-term sums, another order)
    d = got["uvw_sm"].astype(np.float64) - out["uvw_sm"]
    mx, rms = float(np.abs(d).max()), float(np.sqrt((d * d).mean()))
    ref_mx, ref_rms = (float(v) for v in z["err_uvw_sm"])
    print("g20: uvw_sm error against float64: max %.3e (reference float32 %.3e, ratio %.2f), rms %.3e (reference %.3e, ratio %.2f)"
          % (mx, ref_mx, mx / ref_mx, rms, ref_rms, rms / ref_rms))
    assert mx <= 4 * ref_mx and rms <= 2 * ref_rms


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("H,W", [(1, 1), (5, 7), (31, 33)])
def test_odd_pixel_counts(B, H, W):
    x, wts = synthetic(B, H, W)
    got = run(x, wts)
    out, tol, unsure = R.head(x["x_u"], x["x_v"], x["x_w"], x["x_mask"], wts)
    R.compare(got, out, tol, unsure, label="%dx%dx%d:" % (B, H, W))
    assert got["uvw_sm"].min() >= 0 and got["uvw_sm"].max() <= 255


@pytest.mark.parametrize("B,h,w", [(1, 1, 1), (3, 3, 5), (2, 8, 8), (2, 17, 19)])
def test_latent_sizes(B, h, w):
    g = np.random.default_rng(1)
    x4 = np.abs(g.standard_normal((B, 256, h, w))).astype(np.float32)
    wl, bl = (g.standard_normal((3, 256)) * 0.1).astype(np.float32), g.uniform(-0.06, 0.06, 3).astype(np.float32)
    got = css.css_latent(dev(x4), dev(wl).view(3, 256, 1, 1), dev(bl)).cpu().numpy()
    ref, tol = R.latent(x4, wl, bl)
    err = np.abs(got - ref)
    print("latent %dx%dx%d: max error %.3e, largest error / tolerance %.3f" % (B, h, w, err.max(), (err / tol).max()))
    assert (err <= tol).all()
    assert np.abs(np.linalg.norm(got.astype(np.float64), axis=1) - 1).max() < 1e-6
    one = css.css_latent(dev(x4[B - 1:]), dev(wl), dev(bl)).cpu().numpy()
    assert one.tobytes() == got[B - 1:].tobytes()                        # a crop's latent does not depend on the batch


def test_large_logits_do_not_overflow():
    # seed 2: with it no pixel's two best classes are closer than 0.13, so that the float64 expectation itself is the arg-max class to a tenth
    # of the tolerance (with seed 1 one pixel's gap is 0.05 and the second class carries 0.7 % of the weight: a property of the inputs)
    x, wts = synthetic(2, 5, 7, seed=2)
    lg, _ = R._logits(x["x_u"], *wts["u"])
    s = np.float32(300.0 / np.abs(lg).max())
    x = {k: v * s for k, v in x.items()}
    wts["v"] = (wts["v"][0] * 20, wts["v"][1])                          # every head peaked
    lg = {h: R._logits(x["x_" + h], *wts[h])[0] for h in ("u", "v", "w")}
    print("largest |logit| %.1f: 100 * logit reaches %.0f" % (max(np.abs(v).max() for v in lg.values()), 100 * max(np.abs(v).max() for v in lg.values())))
    assert max(np.abs(v).max() for v in lg.values()) > 250
    got = run(x, wts)
    assert all(np.isfinite(v).all() for v in got.values())
    out, tol, unsure = R.head(x["x_u"], x["x_v"], x["x_w"], x["x_mask"], wts)
    R.compare(got, out, tol, unsure, label="large:")
    arg = np.stack([lg[h].argmax(axis=1) for h in ("u", "v", "w")], axis=1).astype(np.float64)
    assert (np.abs(out["uvw_sm"] - arg) <= 0.5 * tol["uvw_sm"]).all()                  # the inputs are peaked enough for the claim below
    err = np.abs(got["uvw_sm"] - arg)
    print("large: uvw_sm against the arg-max class: max %.3e, largest error / tolerance %.3f" % (err.max(), (err / tol["uvw_sm"]).max()))
    assert (err <= tol["uvw_sm"]).all()


def test_exact_class_tie():
    x, wts = synthetic(2, 5, 7)
    wu, bu = wts["u"][0].copy(), wts["u"][1].copy()
    wu[10] = np.abs(wu[10]) + 0.5                                        # dominant on non-negative features
    bu[10] = 0.125
    wu[200], bu[200] = wu[10], bu[10]
    wts["u"] = (wu, bu)
    a, b = run(x, wts), run(x, wts)
    out, tol, unsure = R.head(x["x_u"], x["x_v"], x["x_w"], x["x_mask"], wts)
    err = np.abs(a["uvw_sm"][:, 0] - 105.0)
    print("class tie: |uvw_sm[:, 0] - 105| max %.3e, tolerance at least %.3e; log-probabilities equal: %s"
          % (err.max(), tol["uvw_sm"][:, 0].min(), np.array_equal(a["u"][:, 10], a["u"][:, 200])))
    assert (err <= tol["uvw_sm"][:, 0]).all()
    assert np.array_equal(a["u"][:, 10], a["u"][:, 200])                 # the same k order for every class row: the same bits
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k                       # and the same bits in every call
    R.compare(a, out, tol, unsure, label="class tie:")


def test_exact_mask_tie():
    x, wts = synthetic(2, 5, 7)
    wm, bm = wts["mask"]
    wts["mask"] = (np.stack([wm[0], wm[0]]), np.array([bm[1], bm[1]], np.float32))
    got = run(x, wts)
    assert np.array_equal(got["mask"][:, 0], got["mask"][:, 1])
    assert (got["uvw_sm_masked"] == 0).all()                             # argmax returns the first index on a tie: background
    assert (got["mask_sm"] == 0.5).all()
    assert (got["uvw_sm"] > 0).any()


def test_a_crop_does_not_depend_on_its_batch():
    x, wts = synthetic(3, 31, 33)
    three = run(x, wts)
    one = run({k: v[1:2] for k, v in x.items()}, wts)
    for k in ALL:
        assert one[k].tobytes() == three[k][1:2].tobytes(), k


def test_refusals_and_empty_inputs():
    x, wts = synthetic(1, 4, 4)
    w = {h: (dev(a), dev(b)) for h, (a, b) in wts.items()}
    t = {k: dev(v) for k, v in x.items()}
    ok = (t["x_u"], t["x_v"], t["x_w"], t["x_mask"])
    with pytest.raises(_lib.SdfrError, match="float32"):
        css.css_head(ok[0].half(), *ok[1:], w)
    with pytest.raises(_lib.SdfrError, match="64"):
        css.css_head(*(v[:, :32].contiguous() for v in ok), w)
    cl = ok[1].contiguous(memory_format=torch.channels_last)
    assert cl.shape == ok[1].shape and not cl.is_contiguous()
    with pytest.raises(_lib.SdfrError, match="contiguous"):
        css.css_head(ok[0], cl, ok[2], ok[3], w)
    with pytest.raises(_lib.SdfrError, match="float32"):
        css.css_latent(torch.zeros(1, 256, 2, 2, device=DEV, dtype=torch.float16), torch.zeros(3, 256), torch.zeros(3))
    with pytest.raises(_lib.SdfrError, match="256"):
        css.css_latent(torch.zeros(1, 64, 2, 2, device=DEV), torch.zeros(3, 256), torch.zeros(3))
    # the library refuses C != 64 itself
    h = _lib.lib()
    outs = [torch.full((1, c, 4, 4), -7.0, device=DEV) for c in (3, 3, 2, 1)]
    args = lambda B, C, H: [_lib.ptr(v) for v in ok] + [B, C, H, 4] + [_lib.ptr(v) for hd in HEADS for v in w[hd]] + [_lib.ptr(o) for o in outs] \
        + [None, None, None, _lib.stream_ptr()]                                                   # noqa: E731
    assert h.sdfr_css_head(*args(1, 32, 4)) == -1 and b"64" in h.sdfr_last_error()
    # B = 0 and H * W = 0 succeed and write nothing
    assert h.sdfr_css_head(*args(0, 64, 4)) == 0 and h.sdfr_css_head(*args(1, 64, 0)) == 0
    lat = torch.full((1, 3), -7.0, device=DEV)
    x4 = torch.ones(1, 256, 2, 2, device=DEV)
    wl, bl = torch.ones(3, 256, device=DEV), torch.ones(3, device=DEV)
    assert h.sdfr_css_latent(_lib.ptr(x4), 0, 256, 2, 2, _lib.ptr(wl), _lib.ptr(bl), _lib.ptr(lat), _lib.stream_ptr()) == 0
    assert h.sdfr_css_latent(_lib.ptr(x4), 1, 256, 0, 2, _lib.ptr(wl), _lib.ptr(bl), _lib.ptr(lat), _lib.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert all(bool((o == -7.0).all()) for o in outs) and bool((lat == -7.0).all())
    empty = css.css_head(*(v[:0] for v in ok), w, logprobs=True)
    assert tuple(empty["uvw_sm"].shape) == (0, 3, 4, 4) and tuple(empty["u"].shape) == (0, 256, 4, 4)
    assert tuple(css.css_latent(x4[:0], wl, bl).shape) == (0, 3)
    # the same call with B = 1 does write (the sentinel is not what the kernel leaves)
    assert h.sdfr_css_head(*args(1, 64, 4)) == 0
    torch.cuda.synchronize()
    assert all(bool((o != -7.0).all()) for o in outs)


def test_drop_in_network_end_to_end():
    from sdflabel_amd.fixtures import synthetic_sample
    from sdflabel_amd.networks.resnet_css import setup_css
    from sdflabel_amd.pipelines import optimizer as OP
    from sdflabel_amd.pipelines.frame import refine_sample
    torch.manual_seed(1)
    net = setup_css(mode="eval", logprobs=True).to(DEV)
    with torch.no_grad():
        net.out_mask.conv.bias.copy_(torch.tensor([0.0, 10.0]))          # a random mask head marks nothing: make most pixels foreground
    x = torch.randn(2, 3, 32, 32, device=DEV)
    with torch.no_grad():
        f = {k: v.cpu().numpy() for k, v in net.features(x).items()}
        pred = net(x)
    assert sorted(pred) == ["latent", "mask", "mask_sm", "u", "uvw_sm", "uvw_sm_masked", "v", "w"]
    wts = {h: tuple(p.detach().cpu().numpy() for p in wb) for h, wb in net.head_weights().items()}
    out, tol, unsure = R.head(f["x_u"], f["x_v"], f["x_w"], f["x_mask"], wts)
    out["latent"], tol["latent"] = R.latent(f["x4"], net.out_lat.conv.weight.detach().cpu().numpy(), net.out_lat.conv.bias.detach().cpu().numpy())
    R.compare({k: v.cpu().numpy() for k, v in pred.items()}, out, tol, unsure, label="drop-in:")
    net.logprobs = False
    with torch.no_grad():
        assert sorted(net(x)) == ["latent", "mask", "mask_sm", "uvw_sm", "uvw_sm_masked"]
    # refine_sample takes the module as its css_net
    dec32 = sdflabel_amd.setup_dsdf(ASSET + ".pt", precision=torch.float32)[0].to(DEV)
    dec16 = sdflabel_amd.setup_dsdf(ASSET + ".pt", precision=torch.float16)[0].to(DEV)
    smp, lidar = synthetic_sample(dec32, 40, 32, DEV)
    OP.clear_refiner_cache()
    est, kept, frame_annos, st = refine_sample(smp, net, dec16, sdflabel_amd.Grid3D(40, DEV), 2, {"2d": 0.3, "3d": 0.5}, lidar=lidar, seed=7,
                                               return_stages=True)
    nocs = torch.stack(st["nocs_pred"])
    print("refine_sample with the drop-in network: %d annotations, %d kept, NOCS in [%.3f, %.3f]" % (len(st["annos"]), len(kept), float(nocs.min()),
                                                                                                   float(nocs.max())))
    assert tuple(nocs.shape[1:]) == (3, 128, 128) and float(nocs.min()) >= 0.0 and float(nocs.max()) <= 1.0
