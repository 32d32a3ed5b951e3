"""The joint fit of one shape to several views without a GPU: the numpy restatement (tests/_track_ref.py) against torch float64 autograd +
torch.optim.Adam -- the shared latent and scale from the track loss sum w_v loss_v / W, each view's pose from its own loss_v -- with each
of yaw, trans, scale and latent frozen in turn; csrc/track_cells.h compiled into a host program (tests/track_host/track_host.cpp) against
the restatement bit for bit, also under ASan/UBSan with exact-size buffers and broken tables; a track of one view against
_align_ref.step in every bit; exports / header / binding; argument checks; the association of proposals with tracks on crafted centres;
the calibration of the trajectory bound of tests/test_gpu_track.py; and the three-view case in float64.
"""
import copy
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from sdflabel_amd import _lib
from tests import _align_ref as AR
from tests import _encode_traj as ET
from tests import _prior_train_cases as PC
from tests import _track_cases as TC
from tests import _track_ref as TR
from tests._util import build_host_program
from tests.test_align_cpu import _torch_loss
from tests.test_complete_cpu import _f32_bits, _run, _split, same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement's loop against torch ------------------------------------------------------------------------------------------------

def _torch_fit(dec, samples, soff, voff, z0, scale0, theta0, weights, share, iters, k, lr, lr_pose, lr_step, lr_factor, clamp, code_reg, unit):
    """float64 autograd + torch.optim.Adam on the first k rows of every view.  The shared parameters (latent, and scale with share) take the
    gradient of sum_t (sum_v w_v loss_v / W_t [+ code_reg ||z_t||]); each view's own parameters the gradient of ITS loss_v.  One parameter
    group per learning rate, a rate of 0 frozen."""
    dec = copy.deepcopy(dec).double()
    for p in dec.parameters():
        p.requires_grad_(False)
    own = torch.tensor(TR.track_of(voff))
    T, V = len(voff) - 1, len(theta0)
    w = torch.ones(V, dtype=torch.float64) if weights is None else torch.tensor(np.asarray(weights, np.float64))
    W = torch.zeros(T, dtype=torch.float64).index_add(0, own, w)
    z = torch.tensor(np.asarray(z0, np.float64), requires_grad=lr != 0)
    th = [torch.tensor(np.asarray(theta0, np.float64)[:, i].copy(), requires_grad=lr_pose[i] != 0 and not (share and i == 4)) for i in range(5)]
    sc = torch.tensor(np.asarray(scale0, np.float64).copy(), requires_grad=bool(share) and lr_pose[4] != 0)
    shared = [z] + ([sc] if share else [])
    named = [(z, lr)] + [(th[i], lr_pose[i]) for i in range(5)] + ([(sc, lr_pose[4])] if share else [])
    opt = torch.optim.Adam([{"params": [p], "lr": r, "base": r} for p, r in named if p.requires_grad])
    rows = torch.tensor(np.stack([np.asarray(samples, np.float64)[int(soff[b]):int(soff[b]) + k] for b in range(V)]))
    ok = (rows[:, :, 3] <= rows[:, :, 4]) & (torch.isfinite(rows[:, :, 3]) | torch.isfinite(rows[:, :, 4]))
    lo, hi = torch.nan_to_num(rows[:, :, 3], nan=0.0).clamp(-clamp, clamp), torch.nan_to_num(rows[:, :, 4], nan=0.0).clamp(-clamp, clamp)
    losses = []
    for it in range(iters):
        for grp in opt.param_groups:
            grp["lr"] = grp["base"] * lr_factor ** (it // lr_step)
        zn = z / z.norm(dim=1, keepdim=True) if unit else z
        per, _ = _torch_loss(dec, zn[own], th[:4] + [sc[own] if share else th[4]], rows[:, :, :3], lo, hi, ok, clamp)
        track = torch.zeros(T, dtype=torch.float64).index_add(0, own, w * per) / W
        total = track.sum() if unit else (track + code_reg * z.norm(dim=1)).sum()
        opt.zero_grad(set_to_none=True)
        mine = [p for p in th if p.requires_grad]
        ours = [p for p in shared if p.requires_grad]
        for p, gr in zip(mine, torch.autograd.grad(per.sum(), mine, retain_graph=True) if mine else ()):
            p.grad = gr
        for p, gr in zip(ours, torch.autograd.grad(total, ours) if ours else ()):
            p.grad = gr
        opt.step()
        losses.append(track.detach().numpy().copy())
    theta = np.stack([t.detach().numpy() for t in th], 1)
    if share:
        theta[:, 4] = sc.detach().numpy()[own.numpy()]
    return z.detach().numpy(), sc.detach().numpy(), theta, np.array(losses)


FROZEN = {None: {}, "yaw": {0: 0.0}, "trans": {1: 0.0, 2: 0.0, 3: 0.0}, "scale": {4: 0.0}, "latent": {}}


@pytest.mark.parametrize("share", [1, 0], ids=["shared_scale", "own_scale"])
@pytest.mark.parametrize("name,unit,frozen", [("w128", u, f) for u in (True, False) for f in FROZEN] + [("lat8", True, None)],
                         ids=lambda v: "all" if v is None else ("no_" + v if v in FROZEN else str(v)))
def test_restatement_loop_equals_torch_float64_autograd_and_adam(name, unit, frozen, share):
    dec, net = PC.decoders()[name], PC.net(name)
    samples, soff, voff, z0, scale0, theta0, weights, k, clamp = TC.fit_case(name, 3, 66)
    lr_pose = [0.0 if i in FROZEN[frozen] else r for i, r in enumerate((4e-3, 3e-3, 2e-3, 3e-3, 5e-3))]
    kw = dict(lr=0.0 if frozen == "latent" else 5e-3, lr_pose=lr_pose, lr_step=5, lr_factor=0.1, clamp=clamp, code_reg=1e-4)
    ref = TR.loop(ET.decoder64(net), samples, soff, voff, z0, scale0, theta0, 10, k, False, weights=weights, share=share, unit=unit, ft=np.float64, **kw)
    z_t, sc_t, th_t, losses = _torch_fit(dec, samples, soff, voff, z0, scale0, theta0, weights, share, 10, k, unit=unit, **kw)
    assert np.abs(ref["z"] - z_t).max() <= 1e-12, float(np.abs(ref["z"] - z_t).max())
    assert np.abs(ref["theta"] - th_t).max() <= 1e-12, float(np.abs(ref["theta"] - th_t).max())
    assert np.abs(ref["history"] - losses).max() <= 1e-12
    if share:
        assert np.abs(ref["scale"] - sc_t).max() <= 1e-12
        assert (ref["theta"][:, 4] == ref["scale"][TR.track_of(voff)]).all()
    start = np.array(theta0, np.float64)
    if share:
        start[:, 4] = np.asarray(scale0, np.float64)[TR.track_of(voff)]
    moved = np.abs(ref["theta"] - start).max(0)
    for i in range(5):
        assert (moved[i] == 0) if lr_pose[i] == 0 else (moved[i] > 1e-4), (i, moved)
    assert (np.abs(ref["z"] - z0).max() == 0) if frozen == "latent" else (np.abs(ref["z"] - z0).max() > 1e-3)
    assert (ref["z_view"] == ref["z"][TR.track_of(voff)]).all()
    assert not ref["tflags"].any() and not ref["vflags"].any()
    # the two views of the first track pull at one latent: it is neither view's own fit
    if frozen is None and unit:
        solo = AR.loop(ET.decoder64(net), samples, soff, z0[TR.track_of(voff)], start, 10, k, False, unit=unit, ft=np.float64, **kw)
        assert np.abs(solo["z"][0] - ref["z"][0]).max() > 1e-6 and np.abs(solo["z"][1] - ref["z"][0]).max() > 1e-6
        assert np.abs(solo["z"][2] - ref["z"][1]).max() <= 1e-12                 # the track of one view is that view's own fit


# ---- the header on the host -----------------------------------------------------------------------------------------------------------------

def host_step(exe, tmp, c):
    T, L, V = c["T"], c["L"], c["V"]
    has_w = c["weight"] is not None
    arrays = [np.asarray(c["lr_pose"], np.float32), c["voff"]] + ([c["weight"]] if has_w else []) + \
        [c[k] for k in ("z", "m", "v", "scale", "sm", "sv", "theta", "tm", "tv", "pose", "z_view", "g", "view_loss", "vflags", "loss", "tflags")] + \
        [c["loss"].astype(np.float32)]
    blob = _run(exe, "step", tmp, [T, L, c["unit"], c["t"], _f32_bits(c["code_reg"]), _f32_bits(c["lr"]), c["share"], V, int(has_w)], arrays)
    out = _split(blob, [(np.float32, (T, L))] * 3 + [(np.float32, (T,))] * 3 + [(np.float32, (V, 5))] * 3 + [(np.float32, (V, 6)), (np.float32, (V, L)),
                        (np.int32, (V,)), (np.float64, (T,)), (np.int32, (T,)), (np.float32, (T,))])
    return dict(zip(TR.KEYS, out))


def same_track_step(got, want, what):
    """every word of a step bit for bit, but the cos / sin words of the pose rows: within one float32 ulp"""
    for key in TR.KEYS:
        g, w = got[key], want[key]
        if key == "pose":
            same_bits(g[:, 2:], w[:, 2:], (what, key))
            assert (np.abs(g[:, :2].view(np.int32).astype(np.int64) - w[:, :2].view(np.int32).astype(np.int64)) <= 1).all(), (what, "cos / sin")
        else:
            same_bits(g, w, (what, key))


def _host_checks(exe, tmp):
    for case in TC.step_cases():
        c = TC.step_case(*case)
        want = TC.restate(c)
        same_track_step(host_step(exe, tmp, c), want, TC.case_id(case))
        TC.check_step_case(case, want)


def test_track_cells_on_the_host_equal_the_restatement_bit_for_bit(tmp_path):
    _host_checks(build_host_program(tmp_path, "track_host/track_host.cpp", "track_host"), tmp_path)


def test_track_cells_host_program_under_sanitizers(tmp_path):
    _host_checks(build_host_program(tmp_path, "track_host/track_host.cpp", "track_host_san",
                                    ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]), tmp_path)


@pytest.mark.parametrize("share", [0, 1])
def test_a_track_of_one_view_is_the_align_step_in_every_bit(share):
    """_align_cases's step cases, each shape a track of its own: z, m, v, theta, tm, tv, pose and the flags of _align_ref.step; with a shared
    scale the track's scale and its state are the shape's theta[4], tm[4], tv[4].  -0.0 gradient entries included."""
    from tests import _align_cases as AC
    for case in AC.step_cases():
        B, L, unit, t, rates = case
        z, m, v, theta, tm, tv, pose, g, flags, code_reg, lr, lr_pose = AC.step_case(*case)
        g = np.array(g)
        g[0, 0], g[0, L + 1] = -0.0, -0.0
        want = AR.step(z, m, v, theta, tm, tv, pose, g, flags, unit, code_reg, lr, lr_pose, t)
        voff = np.arange(B + 1)
        stm, stv = (np.array(a) for a in (tm, tv))
        if share:                                             # the views' own scale state rests; the track's carries it
            stm[:, 4], stv[:, 4] = 7.0, 7.0
        got = TR.step(z, m, v, theta[:, 4], tm[:, 4], tv[:, 4], share, voff, None, theta, stm, stv, pose, np.zeros_like(z), g, np.linspace(0.01, 0.02, B),
                      flags, unit, code_reg, lr, lr_pose, t)
        gtm, gtv = got["tm"].copy(), got["tv"].copy()
        if share:
            assert (gtm[:, 4] == 7.0).all() and (gtv[:, 4] == 7.0).all()
            gtm[:, 4], gtv[:, 4] = got["sm"], got["sv"]
            same_bits(got["scale"], want[3][:, 4], (case, "scale"))
        for a, b, n in zip((got["z"], got["m"], got["v"], got["theta"], gtm, gtv, got["pose"], got["vflags"]), want, ("z", "m", "v", "theta", "tm", "tv", "pose", "flags")):
            same_bits(a, b, (case, share, n))
        stepped = (want[7] & 4) == 0
        assert stepped.any() and (got["tflags"][stepped] == 0).all() and (got["tflags"][~stepped] != 0).all()
        same_bits(got["z_view"][stepped], want[0][stepped], (case, "z_view"))
        same_bits(got["loss"][stepped], np.linspace(0.01, 0.02, B)[stepped], (case, "loss"))


# ---- exports, header, binding -------------------------------------------------------------------------------------------------------------

def test_exports_header_and_binding_agree():
    from sdflabel_amd import track as T
    header = open(os.path.join(ROOT, "include", "sdfr.h")).read()
    assert _lib.ABI_VERSION >= 423 and int(re.search(r"#define SDFR_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION
    assert "423: one shape fitted to several views, sdfr_track_step" in header
    body = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    h = _lib.lib()
    assert h.sdfr_version() == _lib.ABI_VERSION
    name = "sdfr_track_step"
    assert name in _lib.EXPORTS and hasattr(h, name) and re.search(r"\bint %s\(" % name, body)
    args = re.search(r"\bint %s\((.*?)\);" % name, body, flags=re.S).group(1)
    assert len(args.split(",")) == len(_lib._PROTOS[name][1]) == 30
    cells = open(os.path.join(ROOT, "sdflabel_amd", "csrc", "track_cells.h")).read()
    for macro, val in (("TRK_MAX_VIEWS", TR.MAX_VIEWS), ("TRK_NO_VIEWS", TR.NO_VIEWS), ("TRK_NO_USABLE", TR.NO_USABLE), ("TRK_SKIPPED", TR.SKIPPED),
                       ("TRK_BAD_TABLE", TR.BAD_TABLE)):
        assert int(re.search(r"#define %s (\d+)" % macro, cells).group(1)) == val, macro
    assert (T.NO_VIEWS, T.NO_USABLE, T.SKIPPED, T.BAD_TABLE, T.MAX_VIEWS) == (TR.NO_VIEWS, TR.NO_USABLE, TR.SKIPPED, TR.BAD_TABLE, TR.MAX_VIEWS)
    # the step reuses the encoder's and the aligner's rules; it has no copy of them
    assert "align_cells.h" in cells and all(n not in cells for n in ("0.999f", "sqrtf"))
    unit = open(os.path.join(ROOT, "sdflabel_amd", "csrc", "track.hip")).read()
    assert all(n in unit for n in ("latent_norm", "latent_unit_dot", "enc_raw_norm", "enc_step_grad", "latent_adam", "enc_bias")) and "atomicAdd" not in unit and "hipMemset" not in unit
    build = open(os.path.join(ROOT, "sdflabel_amd", "csrc", "build.sh")).read()
    assert re.search(r"-ffp-contract=off -c \"\$HERE/track.hip\"", build) and ",track," in build


def test_c_argument_checks_need_no_gpu():
    h = _lib.lib()
    d, inv = 4096, -1            # never dereferenced: every call below is refused before a launch
    rates = (ctypes.c_float * 5)(1e-2, 1e-2, 1e-2, 1e-2, 1e-2)

    def call(**kw):
        a = dict(z=d, m=d, v=d, L=3, T=1, unit=1, scale=d, sm=d, sv=d, share=1, voff=d, V=1, weight=None, theta=d, tm=d, tv=d, pose=d, z_view=d, g=d,
                 view_loss=d, vflags=d, loss=d, tflags=d, code_reg=1e-4, lr=5e-3, lr_pose=rates, t=1, history=None, stride=0, stream=None)
        a.update(kw)
        return h.sdfr_track_step(*a.values())

    for key in ("z", "m", "v", "scale", "sm", "sv", "voff", "theta", "tm", "tv", "pose", "z_view", "g", "view_loss", "vflags", "loss", "tflags", "lr_pose"):
        assert call(**{key: None}) == inv and b"sdfr_track_step: NULL" in h.sdfr_last_error(), key
    assert call(L=0) == inv and b"bad size" in h.sdfr_last_error()
    assert call(L=257) == inv and call(T=-1) == inv and call(T=65536) == inv and call(V=-1) == inv and call(V=65536) == inv
    assert call(t=0) == inv and b"starts at 1" in h.sdfr_last_error()
    assert call(T=2, history=d, stride=1) == inv and b"history_stride" in h.sdfr_last_error()
    assert call(lr=float("inf")) == inv and b"non-finite" in h.sdfr_last_error()
    assert call(code_reg=float("nan")) == inv
    rates[4] = float("nan")
    assert call() == inv and b"non-finite" in h.sdfr_last_error()
    rates[4] = 0.0
    assert call(T=0) == 0 and call(T=0, V=0) == 0
    assert call(T=0, share=0, scale=None, sm=None, sv=None, weight=None, history=None) == 0           # read with share_scale alone; optional


def test_python_argument_checks_come_before_any_launch():
    from sdflabel_amd import track as T
    dec = PC.decoders()["w128"]                                                    # on the CPU
    cloud = np.zeros((4, 3), np.float32)
    view = {"yaw": torch.zeros(1), "trans": torch.zeros(3), "cloud": cloud}
    track = {"latent": torch.zeros(3), "scale": torch.ones(1), "views": [view, view]}
    for bad in (dict(iters=-1), dict(clamp=0.0), dict(rows_per_iter=0), dict(fit=("yaw", "roll")), dict(fit=()), dict(lr_pose=float("nan")), dict(lr_step=0),
                dict(free_rows=65), dict(s_max=-1.0), dict(weights="area"), dict(weights=[1.0]), dict(samples=[])):
        with pytest.raises(ValueError):
            T.align_tracks(dec, [track], **bad)
    with pytest.raises(ValueError, match="1 .. 1024 views"):
        T.align_tracks(dec, [dict(track, views=[])])
    with pytest.raises(ValueError, match="1 .. 1024 views"):
        T.align_tracks(dec, [dict(track, views=[view] * 1025)])
    with pytest.raises(ValueError):
        T.align_tracks(dec, [dict(track, latent=torch.zeros(8))])
    with pytest.raises(_lib.SdfrError, match="no CPU fallback"):
        T.align_tracks(dec, [track])
    doc = T.__doc__
    assert "WITHOUT A CLAIMED OPERATING POINT" in doc and "'scale' IS ON HERE" in doc and "REMAIN COUPLED THROUGH THE PRIOR ALONE" in doc


# ---- association ---------------------------------------------------------------------------------------------------------------------------------

def test_associate_on_crafted_centres():
    from sdflabel_amd.pipelines.sequence import associate
    c0 = [[0, 0, 10], [5, 0, 10], [20, 0, 30]]
    # scan 1: proposal 0 is 0.5 m from track 1 and 4.5 m from track 0; proposal 1 is 1.0 m from track 0; proposal 2 is far from everything
    c1 = [[4.5, 0, 10], [1.0, 0, 10], [40, 0, 5]]
    tracks, assigned = associate([c0, c1], gate=2.0)
    assert assigned[0].tolist() == [0, 1, 2] and assigned[1].tolist() == [1, 0, 3]
    assert tracks == [[(0, 0), (1, 1)], [(0, 1), (1, 0)], [(0, 2)], [(1, 2)]]
    # the gate: exactly on it is accepted, a hair beyond is not
    assert associate([[[0, 0, 0]], [[2.0, 0, 0]]], gate=2.0)[1][1].tolist() == [0]
    assert associate([[[0, 0, 0]], [[np.nextafter(2.0, 3.0), 0, 0]]], gate=2.0)[1][1].tolist() == [1]
    # two proposals competing for one track: the nearer takes it, the other opens a track; a track takes one proposal of a scan
    tracks, assigned = associate([[[0, 0, 0]], [[0.9, 0, 0], [-0.5, 0, 0]]], gate=2.0)
    assert assigned[1].tolist() == [1, 0] and tracks == [[(0, 0), (1, 1)], [(1, 0)]]
    # ties: the same distance to two tracks -> the lower track; two proposals at the same distance from one track -> the lower proposal
    tracks, assigned = associate([[[-1, 0, 0], [1, 0, 0]], [[0, 0, 0]]], gate=2.0)
    assert assigned[1].tolist() == [0]
    tracks, assigned = associate([[[0, 0, 0]], [[1, 0, 0], [-1, 0, 0]]], gate=2.0)
    assert assigned[1].tolist() == [0, 1]
    # a track that finds nothing stays open with the centre it has; tracks follow their LAST centre
    tracks, assigned = associate([[[0, 0, 0]], [], [[1.5, 0, 0]], [[3.0, 0, 0]]], gate=2.0)
    assert [a.tolist() for a in assigned] == [[0], [], [0], [0]] and tracks == [[(0, 0), (2, 0), (3, 0)]]
    # within one scan nothing is merged, however close
    assert associate([[[0, 0, 0], [0.1, 0, 0]]], gate=2.0)[1][0].tolist() == [0, 1]
    assert associate([], gate=2.0) == ([], []) and associate([[], []], gate=2.0)[0] == []
    with pytest.raises(ValueError):
        associate([c0], gate=-1.0)
    again = associate([c0, c1], gate=2.0)
    assert again[0] == [[(0, 0), (1, 1)], [(0, 1), (1, 0)], [(0, 2)], [(1, 2)]]                       # deterministic


# ---- the trajectory cases and their bound -----------------------------------------------------------------------------------------------------

from tests._track_traj import NAMES as TRAJ_NAMES  # noqa: E402


@pytest.fixture(scope="module")
def trajectories():
    """name -> (float64 run with its kink margins, float32 emulation run); computed once"""
    from tests import _track_traj as TT
    return {name: TT.cpu_runs(name) for name in TT.NAMES}


@pytest.mark.parametrize("name", TRAJ_NAMES)
def test_float64_run_admits_every_row_of_the_trajectory_cases(trajectories, name):
    ref, _ = trajectories[name]
    fin = ref["margin"][np.isfinite(ref["margin"])]
    assert ref["margin"].shape[0] == ET.STEPS and fin.size > ref["margin"].size // 2
    assert fin.min() > 1.0, float(fin.min())                                      # no row within 100 fwd_tol of a kink of the loss on any step
    assert ref["face"].min() > 1.0, float(ref["face"].min())                     # nor within 100 roundings of a face of the cube
    assert not ref["tflags"].any() and not ref["vflags"].any()


@pytest.mark.parametrize("name", TRAJ_NAMES)
def test_trajectory_bound_is_four_times_the_emulations_worst_deviation(trajectories, name):
    from tests import _align_cases as AC
    from tests import _track_traj as TT
    ref, emu = trajectories[name]
    worst = AC.deviation(emu["trace"], ref["trace"])
    print("%s: emulation deviates %.3e from float64 over %d steps; bound %.3e" % (name, worst, ET.STEPS, TT.TRAJECTORY_BOUND[name]))
    assert worst > 0
    assert 4 * worst <= TT.TRAJECTORY_BOUND[name] <= 4 * worst * 1.05, (worst, TT.TRAJECTORY_BOUND[name])


def test_three_view_reference_lowers_the_loss():
    """the end-to-end case of tests/test_gpu_track.py in float64: the completion fixture's mesh seen from three sides, one latent and one
    scale fitted over the three views from the antipodal latent.  Asserted: the loss falls.  The cosine to the true latent and the
    whole-shape residual are RECORDED beside those of the three one-view fits (tests/_track_traj.one_view_reference; profiles/track_notes.md),
    whichever way they come out."""
    from tests import _track_traj as TT
    ref = TT.three_reference()
    h = ref["history"]
    print("three views: float64 loss %.4e -> %.4e; cosine %.4f, residual %.4e -> %.4e, scale %.4f (seed %d)"
          % (h[0], h[-1], ref["cosine"], ref["residual_start"], ref["residual"], ref["scale"][0], TT.THREE["seed"]))
    assert not ref["tflags"].any() and not ref["vflags"].any() and len(h) == TT.THREE["iters"]
    assert h[-1] < h[0], (h[0], h[-1])
