"""A numpy restatement of the joint fit of one shape to several views (csrc/track.hip, csrc/track_cells.h; include/sdfr.h has the contract),
written from the header's comments.  TEST INFRASTRUCTURE ONLY: no device code.

step restates sdfr_track_step: which views are usable, the fold in ascending view order from its first term, the track's latent and scale,
each usable view's own pose step and what every view of a stepped track receives.  loop chains tests/_align_ref.py's rows and reduce over
the V views with it around any decoder callable.  `ft` as in _align_ref: np.float32 restates the kernel, np.float64 gives the loop that
torch's float64 autograd and torch.optim.Adam run.
"""
import numpy as np

from tests import _align_ref as AR
from tests import _complete_ref as CR
from tests import _encode_ref as ER

MAX_VIEWS = 1024
NO_VIEWS, NO_USABLE, SKIPPED, BAD_TABLE = 1, 2, 4, 8
POSE = AR.POSE


def count(voff, t, V):
    a, e = int(voff[t]), int(voff[t + 1])
    return -1 if (a < 0 or e < a or e > V or e - a > MAX_VIEWS) else e - a


def latent_grad(zb, gl, unit, code_reg, ft):
    """the gradient of the raw latent from gl, the gradient with respect to what the decoder saw: _align_ref.step's lines"""
    L = len(zb)
    if unit:
        nrm = ER.latent_norm(zb, ft)
        dot = ft(0)
        for i in range(L):
            dot = ft(dot + ft(ft(zb[i] / nrm) * gl[i]))
        return ((gl - (zb / nrm) * dot) / nrm).astype(ft)
    nz = ft(np.sqrt(ER.seq_sumsq(zb, ft)))
    return (gl + code_reg * (zb / nz)).astype(ft) if nz > 0 else gl.copy()


def fold(x, w, ok):
    """sum of w_i x[i] over the usable i in ascending order, float64, from its first term; x [n] or [n][C]"""
    a = None
    for i in np.nonzero(ok)[0]:
        term = np.float64(w[i]) * np.asarray(x[i], np.float64)
        a = term if a is None else a + term
    return a


def step(z, m, v, scale, sm, sv, share, voff, weight, theta, tm, tv, pose, z_view, g, view_loss, vflags, unit, code_reg, lr, lr_pose, t, ft=np.float32,
         loss=None, tflags=None):
    """sdfr_track_step: a dict of every array after the call (copies).  z, m, v [T][L]; scale, sm, sv [T]; voff [T + 1]; weight [V] or None;
    theta, tm, tv [V][5]; pose [V][6]; z_view [V][L]; g float64 [V][L + 5]; view_loss float64 [V]; vflags [V].  loss / tflags: what the
    output arrays hold before the call (a broken table entry leaves its loss word alone)."""
    z, m, v, theta, tm, tv, pose, z_view = (np.array(a, ft) for a in (z, m, v, theta, tm, tv, pose, z_view))
    scale, sm, sv = (np.array(a, ft).reshape(-1) for a in (scale, sm, sv))
    vflags = np.asarray(vflags, np.int32).copy()
    g, view_loss = np.asarray(g, np.float64), np.asarray(view_loss, np.float64)
    T, L = z.shape
    V = len(theta)
    loss = np.zeros((T,), np.float64) if loss is None else np.array(loss, np.float64)
    tflags = np.zeros((T,), np.int32) if tflags is None else np.array(tflags, np.int32)
    hist = np.array(loss, np.float32)                   # the history row: the same words, where they are written
    wrote = np.zeros((T,), bool)
    bc1, bc2 = ER.bias(t, ft)
    f32 = ft is np.float32
    lr, code_reg = ft(np.float32(lr) if f32 else lr), ft(np.float32(code_reg) if f32 else code_reg)
    lr_pose = [ft(np.float32(r) if f32 else r) for r in lr_pose]
    with np.errstate(all="ignore"):
        for tr in range(T):
            n = count(voff, tr, V)
            if n < 0:
                tflags[tr] = BAD_TABLE
                continue
            v0 = int(voff[tr])
            wrote[tr] = True
            w = np.ones((n,), ft) if weight is None else np.asarray(weight, ft)[v0:v0 + n]
            ok = np.zeros((n,), bool)
            for i in range(n):
                vi = v0 + i
                gv = g[vi].astype(ft)
                good = not (vflags[vi] & AR.NO_STEP) and bool(np.isfinite(w[i]) and w[i] > 0) and bool(np.isfinite(gv).all())
                if good and not share:
                    sc = AR.adam(theta[vi, 4], tm[vi, 4], tv[vi, 4], gv[L + 4], lr_pose[4], bc1, bc2, ft)[0] if lr_pose[4] != 0 else theta[vi, 4]
                    good = bool(np.isfinite(sc) and sc > 0)
                ok[i] = good
                if not good:
                    vflags[vi] |= SKIPPED
            if not ok.any():
                loss[tr], tflags[tr] = 0.0, (NO_VIEWS if n == 0 else 0) | NO_USABLE | SKIPPED
                continue
            W = fold(np.ones((n,)), w, ok)
            G = fold(g[v0:v0 + n], w, ok) / W
            loss[tr] = fold(view_loss[v0:v0 + n], w, ok) / W
            gz = latent_grad(z[tr], G[:L].astype(ft), unit, code_reg, ft)
            stepped = bool(np.isfinite(gz).all())
            sc, scm, scv = scale[tr] if share else ft(0), None, None
            if share:
                if lr_pose[4] != 0:
                    sc, scm, scv = AR.adam(scale[tr], sm[tr], sv[tr], ft(G[L + 4]), lr_pose[4], bc1, bc2, ft)
                stepped = stepped and bool(np.isfinite(sc) and sc > 0)
            if not stepped:
                tflags[tr] = SKIPPED
                vflags[v0:v0 + n][ok] |= SKIPPED
                continue
            tflags[tr] = 0
            if share and lr_pose[4] != 0:
                scale[tr], sm[tr], sv[tr] = sc, scm, scv
            if lr != 0:
                z[tr], m[tr], v[tr] = AR.adam(z[tr], m[tr], v[tr], gz, lr, bc1, bc2, ft)
            for i in range(n):
                vi = v0 + i
                z_view[vi] = z[tr]
                if ok[i]:
                    gp = g[vi, L:].astype(ft)
                    for c in range(POSE):
                        r = ft(0) if (share and c == 4) else lr_pose[c]
                        if r != 0:
                            theta[vi, c], tm[vi, c], tv[vi, c] = AR.adam(theta[vi, c], tm[vi, c], tv[vi, c], gp[c], r, bc1, bc2, ft)
                    pose[vi] = AR.pose_row(theta[vi], ft)[0]
                if share:
                    theta[vi, 4] = pose[vi, 5] = sc
    hist[wrote] = loss[wrote].astype(np.float32)
    return {"z": z, "m": m, "v": v, "scale": scale, "sm": sm, "sv": sv, "theta": theta, "tm": tm, "tv": tv, "pose": pose, "z_view": z_view,
            "vflags": vflags, "loss": loss, "tflags": tflags, "history": hist}


KEYS = ("z", "m", "v", "scale", "sm", "sv", "theta", "tm", "tv", "pose", "z_view", "vflags", "loss", "tflags", "history")


def track_of(voff):
    """the track of every view, for a well-formed table"""
    return np.concatenate([np.full((int(voff[t + 1]) - int(voff[t]),), t, np.int64) for t in range(len(voff) - 1)]) if len(voff) > 1 else np.zeros((0,), np.int64)


def loop(decoder, samples, soff, voff, z0, scale0, theta0, iters, k, draw_on, weights=None, share=True, seed=0, lr=5e-3, lr_pose=(1e-2,) * POSE, lr_step=None,
         lr_factor=0.1, clamp=0.2, code_reg=1e-4, unit=True, ft=np.float32, watch=None, trace=None):
    """The joint fit with any decoder callable: decoder(inputs [n][L + 3]) -> (pred [n], J [n][L + 3]).  samples / soff: the views' rows, view
    v the shape v of _align_ref.rows; z0 [T][L], scale0 [T], theta0 [V][5].  Before iteration 0 every view takes its track's latent and
    (with share) scale.  Returns a dict: z (raw), zn [T][L], scale [T], theta [V][5], history [iters][T] (the track loss per iteration, before
    its step), view_history [iters][V], tflags / vflags of the last iteration.  watch(it, inputs, pred, lo, hi, J, pose): called per iteration;
    trace: a list that receives (z, theta) after every step."""
    z, theta = np.array(z0, ft), np.array(theta0, ft).reshape(-1, POSE)
    T, L = z.shape
    V = len(theta)
    own = track_of(voff)
    scale = np.array(scale0, ft).reshape(-1)
    if share:
        theta[:, 4] = scale[own]
    m, v, sm, sv, tm, tv = np.zeros_like(z), np.zeros_like(z), np.zeros_like(scale), np.zeros_like(scale), np.zeros_like(theta), np.zeros_like(theta)
    z_view = z[own].copy()
    pose = AR.pose_row(theta, ft)
    lr_step = max(1, iters // 2) if lr_step is None else lr_step
    hist, vhist = np.zeros((iters, T), np.float64), np.zeros((iters, V), np.float64)
    vflags, tflags = np.zeros((V,), np.int32), np.zeros((T,), np.int32)
    for it in range(iters):
        inputs, cam, lo, hi, _, vflags = AR.rows(samples, soff, V, k, draw_on, seed, it, z_view.astype(np.float32), unit, pose.astype(np.float32))
        if ft is not np.float32:                    # the float64 loop, as _align_ref.loop has it
            inputs, zn = inputs.astype(ft), ER.normalised(z_view, unit, ft)
            _, lo, hi, _, _ = CR.rows(samples, soff, V, k, draw_on, seed, it, z_view.astype(np.float32), unit)
            for b in range(V):
                if vflags[b]:
                    continue
                sl = slice(b * k, (b + 1) * k)
                x = AR.lattice_x(cam[sl], pose[b])
                inside = (np.abs(x) <= 1).all(1)
                inputs[sl, :L], inputs[sl, L:] = zn[b], np.where(inside[:, None], x, 0.0)
                lo[sl], hi[sl] = np.where(inside, lo[sl], np.nan), np.where(inside, hi[sl], np.nan)
        pred, J = decoder(inputs)
        if watch is not None:
            watch(it, inputs, pred, lo, hi, J, pose)
        if ft is np.float32:
            vloss, g, vflags, _ = AR.reduce(pred, lo, hi, J, cam, pose, L, V, k, clamp, vflags)
        else:
            vloss, g, vflags = AR.reduce64(pred, lo, hi, J, cam, pose, L, V, k, clamp, vflags)
        f = lr_factor ** (it // lr_step)
        out = step(z, m, v, scale, sm, sv, share, voff, weights, theta, tm, tv, pose, z_view, g, vloss, vflags, unit, code_reg, lr * f,
                   [r * f for r in lr_pose], it + 1, ft)
        z, m, v, scale, sm, sv, theta, tm, tv, pose, z_view, vflags, loss, tflags = (out[key] for key in KEYS[:-1])
        hist[it], vhist[it] = loss, vloss
        if trace is not None:
            trace.append((z.copy(), theta.copy()))
    return {"z": z, "zn": ER.normalised(z, unit, ft), "scale": scale, "theta": theta, "pose": pose, "history": hist, "view_history": vhist, "tflags": tflags,
            "vflags": vflags, "z_view": z_view}
