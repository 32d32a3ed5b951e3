"""High-precision references of the renderer's kernels (csrc/splat.hip, csrc/project.hip, csrc/surface.hip).  TEST INFRASTRUCTURE ONLY.

`splat_ref` restates, densely over (surfel, pixel) pairs and in float64 by default, what the three primitives and the compositing compute
(primitives.py:4-242, rasterer.py:92-144 of the reference, the same formulas as oracle/sdf_oracle.py) and what torch autograd returns for
them, with the kernels' contract for their inputs: the float32 arrays the C entry points receive (K, K^-1, camera-frame surfels, the
attribute, for the circle primitives the clamped 2-D projections and the depth norm, the background image and its logit) are taken as
exact numbers.  Besides values and gradients it returns

  * the MASS of every output element: the sum of the absolute values of the terms added into it, each term's factors taken by absolute
    value as well (so that the cancellation inside dL/dw - S counts).  A float32 evaluation in any summation order differs from the exact
    result by a small multiple of eps32 * (1 + logit scale) * mass: every term carries the relative rounding of its softmax weight,
    eps32 times the size of its logit (C: 150 for the disc, 100 for the circle, 10 000 for circle_opt), see `bound`;
  * per surfel the smallest DECISION RATIO of its (surfel, pixel) pairs: |margin| / (float32 decision error) of every threshold the pair
    passes -- the disc edge, |n.ray| against 0.01, the circle edge, the stamp's truncation -- and per pixel the ratio of the clamp(max=1)
    gates.  A ratio below 1 means float32 arithmetic may decide the other way: tests/_splat_cases.py admits no such surfel or pixel.

With dtype=np.float32 the same code is "the reference's own arithmetic in float32", against which the bounds' constants are measured.
`project_ref` and the three `surface_*` functions do the same for the projection and the iso-surface kernels."""
import numpy as np

EPS32 = float(np.finfo(np.float32).eps)
EXP_OVF = 88.72283905206835          # log(FLT_MAX): float32 sigmoid(x) = 1 / (1 + exp(-x)) is positive while exp(-x) is finite
PRIM_ID = {"disc": 0, "circle": 1, "circle_opt": 2}
DEFAULTS = {"disc": (0.04, 150.0, 5.0), "circle": (0.02, 100.0, 3.0), "circle_opt": (0.025, 10000.0, 5.0)}   # diam, depth_constant, softclamp_constant


def f32(x):
    return float(np.float32(x))


def logit_scale(C):
    """size of the logits' float32 rounding in units of eps32 = 2 unit roundoffs: logits are q C, and q = 1 - t / nu (disc) or 1 - z / ||z||
    (circles) is a quotient and a sum of magnitude about 1 for surfels in front of the camera -- two roundings"""
    return 1.0 + float(C)


def pixel_xy(W, H):
    return np.tile(np.arange(W), H), np.repeat(np.arange(H), W)


def _stamp_mask(uv, rad, W, H, alt):
    """coverage of circle_opt (primitives.py:118-127,135-138,155): (N, H W) bool, and per surfel the decision ratio of the truncations"""
    N = uv.shape[0]
    yy, xx = np.mgrid[-7:8, -7:8]
    off = np.stack([xx.reshape(-1), yy.reshape(-1)], 1).astype(np.float64)
    pos = off[None] + uv[:, None, :].astype(np.float64)
    ids = np.trunc(pos).astype(np.int64)
    ids[..., 0] = np.clip(ids[..., 0], 0, W - 1)
    ids[..., 1] = np.clip(ids[..., 1], 0, H - 1)
    if alt:
        val = np.maximum(rad.astype(np.float64)[:, None] - np.sqrt((off * off).sum(-1))[None], 0.0)
    else:
        val = np.ones((N, off.shape[0]))
    dense = np.zeros((N, H * W))
    np.add.at(dense, (np.arange(N)[:, None], ids[..., 1] * W + ids[..., 0]), val)
    u = uv.astype(np.float64)
    fr = u - np.floor(u)
    marg = np.where(fr == 0, np.inf, np.minimum(fr, 1 - fr))
    ratio = (marg / (EPS32 * (np.abs(u) + 8.0))).min(axis=1)
    if alt:                                                        # r - ||offset|| > 0 for the integer offsets: sqrt of 0..98
        dists = np.sqrt(np.unique((off * off).sum(-1)))
        r = rad.astype(np.float64)
        ratio = np.minimum(ratio, np.abs(r[:, None] - dists[None]).min(axis=1) / (4 * EPS32 * (r + 10.0)))
    return dense > 0, ratio


def splat_ref(prim, K, Kinv, p, n, attr, W, H, diam=None, C=None, alt=False, clamp_c=None, uv=None, znorm=None, bg=None, bg_logit=None,
              grads=None, gW=None, want_W=False, chunk=1024, dtype=np.float64, exp_ovf=EXP_OVF):
    """Forward (and, with grads = (gC, gM, gD, gN) -- any of them None -- or a dense gW (rows, P), backward) of one crop.

    prim 'disc' | 'circle' | 'circle_opt'; alt: the primitive's other clamp (disc: sigmoid; circles: hard edge).  Returns a dict:
      color, mask, depth, normals (post-clamp, (3|1, H, W)), *_pre, mass_color, mass_depth, mass_normals ((3|1, P)),
      ncov (N,) covered pixels per surfel, ext (N, 4) covered extent x0, y0, x1, y1, npix_cov (P,) surfels per pixel,
      ratio (N,) decision ratio per surfel, gate_ratio (7, P), und_px (P,) pixels with an undecided pair or gate, top (P,) heaviest surfel per pixel, q_min the smallest pre-clamp logit
      argument of a covered pair, q_und the largest |dl| / mass over pairs with |q| < 8 eps32 (the clamp(min=0) gate's weighted margin), W (rows, P) if want_W; with a backward: g_p, g_n, g_attr (N, 3), their masses mass_g_*, and for a
      dense gW additionally wsum (P,) = sum_rows w gW and its mass."""
    EXP_OVF = exp_ovf        # (float64 autograd restatements pass log(DBL_MAX): where THEIR sigmoid(.) > 0 ends)
    dt = np.dtype(dtype)
    d0, C0, c0 = DEFAULTS[prim]
    diam = f32(d0 if diam is None else diam)
    C = f32(C0 if C is None else C)
    cc = f32(c0 if clamp_c is None else clamp_c)
    A = lambda a: np.asarray(a, np.float32).astype(dt)
    K, Kinv, p, n, attr = A(K), A(Kinv), A(p).reshape(-1, 3), A(n).reshape(-1, 3), A(attr).reshape(-1, 3)
    N = p.shape[0]
    P = W * H
    xs, ys = pixel_xy(W, H)
    mattr = (n + 1) / 2
    pz = p[:, 2]
    has_bg = bg is not None
    if has_bg:
        bgv = A(bg).reshape(3, P)
        lbg = dt.type(float(bg_logit))
    out = {}
    ratio = np.full(N, np.inf)
    stamp = None
    if prim != "disc":
        uv = A(uv).reshape(-1, 2)
        zn = dt.type(float(znorm))
        rad = np.abs(K[0, 0] * diam / (pz + EPS32))
        q0 = -pz / (zn + EPS32) + 1
        zl = np.maximum(q0, 0) * C
        if prim == "circle_opt":
            stamp, ratio = _stamp_mask(uv, rad, W, H, alt)
    a = (n * p).sum(1)
    absnp = (np.abs(n) * np.abs(p)).sum(1).astype(np.float64)
    imgs = {k: np.zeros((c, P), dt) for k, c in (("color", 3), ("mask", 1), ("depth", 1), ("normals", 3))}
    mass = {k: np.zeros((c, P)) for k, c in (("color", 3), ("depth", 1), ("normals", 3))}
    ncov = np.zeros(N, np.int64)
    ext = np.stack([np.full(N, W), np.full(N, H), np.full(N, -1), np.full(N, -1)], 1)
    npc = np.zeros(P, np.int64)
    top = np.zeros(P, np.int64)
    qmin = np.inf
    q_und = 0.0
    Wd = np.zeros((N + (1 if has_bg else 0), P), dt) if want_W else None
    back = grads is not None or gW is not None
    if back:
        z3 = np.zeros((3, P), dt)
        if gW is None:
            gC, gM, gD, gN = grads
            gC = A(gC).reshape(3, P) if gC is not None else z3
            gM = A(gM).reshape(P) if gM is not None else np.zeros(P, dt)
            gD = A(gD).reshape(P) if gD is not None else np.zeros(P, dt)
            gN = A(gN).reshape(3, P) if gN is not None else z3
        else:
            gWd = A(gW).reshape(-1, P)
            wsum = np.zeros(P, dt)
            mwsum = np.zeros(P)
        acc = {k: np.zeros((N, 3), dt) for k in ("sC", "sN", "sB")}
        accm = {k: np.zeros((N, 3)) for k in ("sC", "sN", "sB")}
        sZ = np.zeros(N, dt); sA = np.zeros(N, dt); sL = np.zeros(N, dt)
        mZ = np.zeros(N); mA = np.zeros(N); mL = np.zeros(N)
    gate_ratio = np.full((7, P), np.inf)
    und_px = np.zeros(P, bool)
    ls = logit_scale(C)
    for s in range(0, P, chunk):
        sl = slice(s, min(s + chunk, P))
        x = xs[sl].astype(dt); y = ys[sl].astype(dt)
        np_ = x.shape[0]
        if prim == "disc":
            r = np.stack([Kinv[0, 1] * y + Kinv[0, 0] * x + Kinv[0, 2], Kinv[1, 1] * y + Kinv[1, 0] * x + Kinv[1, 2],
                          Kinv[2, 1] * y + Kinv[2, 0] * x + Kinv[2, 2]], 1)                       # primitives.py:203-208
            b0 = n @ r.T                                                                             # :209
            small = np.abs(b0) < 0.01                                                                # :210
            b = np.where(small, dt.type(EPS32), b0)
            with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
                t = a[:, None] / b                                                                   # :211
                vec = p[:, None, :] - r[None] * t[:, :, None]                                        # :212,:215
                d = np.sqrt((vec * vec).sum(-1))
                absrn = np.abs(r.astype(np.float64)) @ np.abs(n.astype(np.float64)).T                # (p, N)
                rn = np.sqrt((r.astype(np.float64) ** 2).sum(1))
                tb = np.abs(t.astype(np.float64)); bb = np.abs(b.astype(np.float64))
                # float32 error of the distance d: roundings of p - r t, plus |r| times the error of t = a / b (a: three products;
                # b: three products, or the exact eps that replaces a small one)
                dtt = EPS32 * (absnp[:, None] / bb + tb * (np.where(small, 0.0, absrn.T / bb) + 1.0))
                dd = EPS32 * (np.abs(p.astype(np.float64)).sum(1)[:, None] + 2 * rn[None] * tb) + rn[None] * dtt
                if alt:
                    arg = (diam - d) * cc                                                            # :217-218,:226
                    m = arg > -EXP_OVF
                    # sigmoid(arg) > 0 ends where exp(-arg) overflows: the error of arg is c times that of d, the roundings of the
                    # difference and the product, and expf's own ulp at an argument of 88.7
                    darg = cc * 2 * dd + EPS32 * (cc * (diam + d.astype(np.float64)) + 2 * np.abs(arg.astype(np.float64)))
                    edge = np.abs(arg.astype(np.float64) + EXP_OVF) / darg
                else:
                    m = d < diam                                                                     # :220,:226
                    edge = np.abs(diam - d.astype(np.float64)) / (2 * dd)
                if True:
                    # |n.ray| against 0.01: matters where the pair is covered on either side of the threshold
                    t_alt = a[:, None].astype(np.float64) / np.where(small, b0.astype(np.float64), EPS32)
                    v_alt = p[:, None, :].astype(np.float64) - r[None].astype(np.float64) * t_alt[:, :, None]
                    d_alt = np.sqrt((v_alt * v_alt).sum(-1))
                    cov_alt = ((diam - d_alt) * cc > -EXP_OVF) if alt else (d_alt < diam)
                    rb = np.abs(np.abs(b0.astype(np.float64)) - f32(0.01)) / (4 * EPS32 * absrn.T)
                    edge = np.minimum(edge, np.where(m | cov_alt, rb, np.inf))
                edge = np.where(np.isfinite(edge), edge, np.where(np.isnan(edge), 0.0, edge))
            ratio = np.minimum(ratio, edge.min(axis=1))
            und_px[sl] |= (edge < 1).any(axis=0)
            tm = np.where(m, t, 0)
            nu = np.sqrt((tm * tm).sum(0))                                                           # :227-228
            nue = nu + EPS32
            with np.errstate(over="ignore", invalid="ignore"):
                q = np.where(m, -t / nue[None] + 1, 0)                                               # :229
            l = np.maximum(q, 0) * C                                                                 # :230
        else:
            q = np.broadcast_to(q0[:, None], (N, np_))
            l = np.broadcast_to(zl[:, None], (N, np_))
            if prim == "circle":
                dx = uv[:, 0:1] - x[None]; dy = uv[:, 1:2] - y[None]
                d = np.sqrt(dx * dx + dy * dy)                                                       # :42
                if alt:
                    m = (rad[:, None] - d) > 0                                                       # :51-53,:55
                    mag = rad[:, None] + d + np.abs(uv[:, 0:1]) + np.abs(uv[:, 1:2]) + x[None] + y[None]
                    edge = np.abs(rad[:, None] - d).astype(np.float64) / (4 * EPS32 * mag.astype(np.float64))
                else:
                    arg = (rad[:, None] - d) * cc                                                    # :46-49,:55
                    m = arg > -EXP_OVF
                    # (the error of arg: the roundings of r, d, their difference and the product, and expf's own ulp at 88.7)
                    mag = rad[:, None] + d + np.abs(uv[:, 0:1]) + np.abs(uv[:, 1:2]) + x[None] + y[None]
                    edge = np.abs(arg.astype(np.float64) + EXP_OVF) / (EPS32 * (4 * cc * mag.astype(np.float64) + 2 * np.abs(arg.astype(np.float64))))
                ratio = np.minimum(ratio, edge.min(axis=1))
                und_px[sl] |= (edge < 1).any(axis=0)
            else:
                m = stamp[:, sl]
        if m.any() and N:
            qmin = min(qmin, float(q[m].min()))
        # softmax over the surfels (and the background row): masked for disc / circle_opt (:240, :156), over z * mask for the circle (:70)
        neg = dt.type(-np.inf)
        lm = np.where(m, l, neg)
        lmax = lm.max(axis=0) if N else np.full(np_, neg)
        nunc = N - m.sum(axis=0)
        if prim == "circle":
            lmax = np.where(nunc > 0, np.maximum(lmax, 0), lmax)
        if has_bg:
            lmax = np.maximum(lmax, lbg)
        fin = np.isfinite(lmax)
        lsafe = np.where(fin, lmax, 0)
        e = np.where(m, np.exp(np.where(m, l - lsafe[None], 0)), 0)
        dcov = e.sum(axis=0)
        den = dcov.copy()
        if prim == "circle":
            den = den + np.where(nunc > 0, nunc * np.exp(-lsafe), 0)
        ebg = np.exp(lbg - lsafe) if has_bg else np.zeros(np_, dt)
        den = den + ebg
        act = den > 0
        dsafe = np.where(act, den, 1)
        w = e / dsafe[None]
        wbg = ebg / dsafe
        Cs = attr.T @ w + (wbg[None] * bgv[:, sl] if has_bg else 0)
        full = act & (dcov + ebg == den)
        Ms = np.where(full, 1.0, w.sum(axis=0) + wbg)                    # the weights of a fully covered pixel sum to one exactly
        Ds = pz @ w
        Ns = mattr.T @ w
        imgs["color"][:, sl] = Cs; imgs["mask"][0, sl] = Ms; imgs["depth"][0, sl] = Ds; imgs["normals"][:, sl] = Ns
        w64 = w.astype(np.float64)
        mass["color"][:, sl] = np.abs(attr.astype(np.float64)).T @ w64 + (np.abs(wbg[None] * bgv[:, sl]) if has_bg else 0)
        mass["depth"][0, sl] = np.abs(pz.astype(np.float64)) @ w64
        mass["normals"][:, sl] = np.abs(mattr.astype(np.float64)).T @ w64
        # clamp gates: the composite's float32 error is its summation error plus the weights' error, and a weight moves with the logits'
        # rounding by at most 2 eps32 ls w (1 - w): nothing where one row holds the whole pixel (a lone surfel, the background alone)
        wmax = np.maximum(w64.max(axis=0) if N else 0.0, wbg.astype(np.float64))
        gthr = 4 * EPS32 * (1 + ls * (1 - wmax))[None]
        gate_ratio[0:3, sl] = np.abs(1 - Cs.astype(np.float64)) / (gthr * np.maximum(mass["color"][:, sl], 1e-300))
        gate_ratio[4:7, sl] = np.abs(1 - Ns.astype(np.float64)) / (gthr * np.maximum(mass["normals"][:, sl], 1e-300))
        gate_ratio[:, sl][:, ~act] = np.inf
        ncov += m.sum(axis=1)
        npc[sl] = m.sum(axis=0)
        if N:
            top[sl] = w.argmax(axis=0)
            xi = xs[sl]; yi = ys[sl]
            ext[:, 0] = np.minimum(ext[:, 0], np.where(m, xi[None], W).min(axis=1)); ext[:, 1] = np.minimum(ext[:, 1], np.where(m, yi[None], H).min(axis=1))
            ext[:, 2] = np.maximum(ext[:, 2], np.where(m, xi[None], -1).max(axis=1)); ext[:, 3] = np.maximum(ext[:, 3], np.where(m, yi[None], -1).max(axis=1))
        if want_W:
            Wd[:N, sl] = w
            if has_bg:
                Wd[N, sl] = wbg
        if not back:
            continue
        # ---- backward: clamp(max=1) passes the gradient where the composite is <= 1 (the mask's gate is always open: Ms <= 1) ----
        if gW is None:
            gCg = gC[:, sl] * (Cs <= 1); gMg = gM[sl]; gDg = gD[sl]; gNg = gN[:, sl] * (Ns <= 1)
            dW = attr @ gCg + gMg[None] + pz[:, None] * gDg[None] + mattr @ gNg
            aW = np.abs(attr.astype(np.float64)) @ np.abs(gCg) + np.abs(gMg)[None] + np.abs(pz.astype(np.float64))[:, None] * np.abs(gDg)[None] \
                + np.abs(mattr.astype(np.float64)) @ np.abs(gNg)
            S = (w * dW).sum(axis=0)
            aS = (w64 * aW).sum(axis=0)
            if has_bg:
                dbg = (gCg * bgv[:, sl]).sum(axis=0) + gMg
                S = S + wbg * dbg
                aS = aS + wbg * (np.abs(gCg * bgv[:, sl]).sum(axis=0) + np.abs(gMg))
            acc["sC"] += w @ gCg.T; accm["sC"] += w64 @ np.abs(gCg).T
            acc["sN"] += w @ gNg.T; accm["sN"] += w64 @ np.abs(gNg).T
            sZ += w @ gDg; mZ += w64 @ np.abs(gDg)
        else:
            dW = gWd[:N, sl]; aW = np.abs(dW.astype(np.float64))
            S = (w * dW).sum(axis=0); aS = (w64 * aW).sum(axis=0)
            if gWd.shape[0] > N:
                S = S + wbg * gWd[N, sl]; aS = aS + wbg * np.abs(gWd[N, sl])
            wsum[sl] = S
            mwsum[sl] = aS
        dl = w * (dW - S[None])                                          # d L / d logit on the covered entries (w = 0 elsewhere)
        adl = w64 * (aW + aS[None])
        # the clamp(min=0) gate of the logits: q = 1 - t / (nu + eps) is about 1e-7 -- below float32's rounding of the difference, so undecided --
        # exactly where a surfel is alone on its pixel; there w = 1 and dL/dw = S, so the gradient the gate would pass or block is zero.
        # q_und records the largest |dl| (relative to its mass) over the pairs whose |q| lies within 8 eps32: the gate's weighted margin.
        und_q = m & (np.abs(q) < 8 * EPS32)
        if und_q.any():
            q_und = max(q_und, float((np.abs(dl.astype(np.float64))[und_q] / np.maximum(adl[und_q], 1e-300)).max()))
        if prim == "disc":
            with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
                dq = np.where(q >= 0, dl * C, 0)
                dtt_ = np.where(m, -dq / nue[None], 0)                   # zeta = -t * mask
                da = np.where(m, dtt_ / b, 0)
                db = np.where(m & ~small, -dtt_ * t / b, 0)              # the eps overwrite passes no gradient through b (:210)
                ma = np.where(m, adl * C / nue[None] / np.abs(b), 0).astype(np.float64)
                mb = np.where(m & ~small, ma * np.abs(t), 0).astype(np.float64)
            sA += da.sum(axis=1); mA += ma.sum(axis=1)
            acc["sB"] += db @ r; accm["sB"] += mb @ np.abs(r.astype(np.float64))
        else:
            sL += np.where(m, dl, 0).sum(axis=1); mL += np.where(m, adl, 0).sum(axis=1)
    out.update(color=np.minimum(imgs["color"], 1).reshape(3, H, W), mask=np.minimum(imgs["mask"], 1).reshape(1, H, W),
               depth=imgs["depth"].reshape(1, H, W), normals=np.minimum(imgs["normals"], 1).reshape(3, H, W),
               color_pre=imgs["color"], normals_pre=imgs["normals"], mass_color=mass["color"], mass_depth=mass["depth"],
               mass_normals=mass["normals"], ncov=ncov, ext=ext, npix_cov=npc, ratio=ratio, gate_ratio=gate_ratio, und_px=und_px | (gate_ratio < 1).any(axis=0), top=top, q_min=qmin, q_und=q_und,
               logit_scale=ls)
    if want_W:
        out["W"] = Wd
    if back:
        g_p = np.zeros((N, 3), dt); g_n = np.zeros((N, 3), dt)
        m_p = np.zeros((N, 3)); m_n = np.zeros((N, 3))
        g_n += 0.5 * acc["sN"]; m_n += 0.5 * accm["sN"]
        g_p[:, 2] += sZ; m_p[:, 2] += mZ
        if prim == "disc":
            g_n += acc["sB"] + sA[:, None] * p; m_n += accm["sB"] + mA[:, None] * np.abs(p)
            g_p += sA[:, None] * n; m_p += mA[:, None] * np.abs(n)
        else:
            k = C / (float(zn) + EPS32)
            g_p[:, 2] -= np.where(q0 >= 0, sL * C, 0) / (zn + EPS32); m_p[:, 2] += np.where(q0 >= 0, mL * k, 0)
        out.update(g_p=g_p, g_n=g_n, g_attr=acc["sC"], mass_g_p=m_p, mass_g_n=m_n, mass_g_attr=accm["sC"])
        if gW is not None:
            out["wsum"] = wsum
            out["mass_wsum"] = mwsum
    return out


# The constants of the bounds, per primitive: (images and dense weights, gradient rows), in units of eps32 * logit_scale(C) * mass.  Each is
# 4 x the largest error of THIS file's arithmetic run in float32 against itself in float64 over every committed case, rounded up by a tenth
# (measured 2.229 / 3.744, 0.3763 / 0.5036, 0.4523 / 0.5844; tests/test_splat_refs_cpu.py measures it again and asserts the relation;
# profiles/splat_tests_notes.md).  The factor 4 allows for another summation order and the 1-ulp reciprocals of the kernels' gradient chain;
# the tenth keeps the CPU test independent of how another numpy build rounds the last bits of its float32 sums.
C_BOUND = {"disc": (9.8, 16.5), "circle": (1.66, 2.2), "circle_opt": (2.0, 2.6)}
FLOOR = 1e-30     # absolute: terms below float32's normal range (1.2e-38) vanish in a float32 evaluation, and several hundred may


def bound(c, mass, ls=1.0):
    """the float32 error allowed on an element of mass `mass`: c eps32 (logit scale) mass (+ the underflow floor)"""
    return c * EPS32 * ls * np.asarray(mass, np.float64) + FLOOR


def unit_error(got, ref, mass, ls=1.0):
    """|got - ref| in units of eps32 * ls * mass, elementwise; elements of zero mass must agree exactly (0 -> 0, else inf)"""
    got = np.asarray(got, np.float64); ref = np.asarray(ref, np.float64); mass = np.asarray(mass, np.float64)
    d = np.maximum(np.abs(got - ref) - FLOOR, 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        u = d / np.maximum(EPS32 * ls * mass, 1e-300)
    return np.where(mass > 0, u, np.where(d == 0, 0.0, np.inf))


# ---- projection (projection.py:7-101, rot='dcm'; the quaternion path as the Python layer calls it: the same kernel on the rotation matrix
# of the quaternion, colour mode 2 = no flip of the NOCS x, projection.py:147-149) --------------------------------------------------------

def project_ref(pose, K, points, normals, colors, mode, res_x, res_y, dtype=np.float64):
    """sdfr_project_dcm: mode 0 colours passed through, 1 NOCS (-x, y, z), 2 NOCS (x, y, z), +4: (c + 1) / 2 applied.  Returns p_cam, n_cam,
    col, uv, front (N,) bool, fidx, xyzf, fslot, and the decision ratios front_ratio (N,), uv_ratio (N,) (the clamps of uv to [-1, res])."""
    dt = np.dtype(dtype)
    A = lambda a: np.asarray(a, np.float32).astype(dt)
    pose, K, pts, nrm = A(pose).reshape(4, 4), A(K).reshape(3, 3), A(points).reshape(-1, 3), A(normals).reshape(-1, 3)
    R, t = pose[:3, :3], pose[:3, 3]
    pc = pts @ R.T + t[None]
    nc = nrm @ R.T
    if mode & 3:
        col = pts * (np.array([1, 1, 1], dt) if (mode & 3) == 2 else np.array([-1, 1, 1], dt))[None]
        if mode & 4:
            col = (col + 1) * 0.5
    else:
        col = A(colors).reshape(-1, 3)
    dot = (nc * pc).sum(1)
    front = dot < 0
    aR = np.abs(R.astype(np.float64))
    apc = np.abs(pts.astype(np.float64)) @ aR.T + np.abs(t.astype(np.float64))[None]
    anc = np.abs(nrm.astype(np.float64)) @ aR.T
    front_ratio = np.abs(dot.astype(np.float64)) / (6 * EPS32 * np.maximum((anc * apc).sum(1), 1e-300))
    h = pc @ K.T
    with np.errstate(divide="ignore", invalid="ignore"):
        un = h[:, :2] / (h[:, 2:] + EPS32)
    uv = np.stack([np.clip(un[:, 0], -1, res_x), np.clip(un[:, 1], -1, res_y)], 1)
    ah = apc @ np.abs(K.astype(np.float64)).T
    with np.errstate(divide="ignore", invalid="ignore"):
        du = 6 * EPS32 * (ah[:, :2] / np.abs(h[:, 2:].astype(np.float64)) + np.abs(un.astype(np.float64)) * ah[:, 2:] / np.abs(h[:, 2:].astype(np.float64)))
        lim = np.array([res_x, res_y], np.float64)[None]
        uv_ratio = np.minimum(np.abs(un.astype(np.float64) + 1), np.abs(un.astype(np.float64) - lim)) / du
    uv_ratio = np.where(np.isfinite(uv_ratio), uv_ratio, 0.0).min(axis=1)
    fidx = np.nonzero(front)[0]
    fslot = np.full(pts.shape[0], -1, np.int64)
    fslot[fidx] = np.arange(fidx.shape[0])
    return dict(p_cam=pc, n_cam=nc, col=col, uv=uv, front=front, fidx=fidx, xyzf=pc[fidx], fslot=fslot, front_ratio=front_ratio,
                uv_ratio=uv_ratio, mass_p_cam=apc, mass_n_cam=anc)


def project_bwd_ref(pose, points, normals, g_pc, g_nc, g_col, mode, g_xyzf=None, fslot=None, dtype=np.float64):
    """sdfr_project_dcm_bwd: g_points, g_normals, g_colors (mode 0), g_pose (12 sums, rows of [R | t]) with their masses."""
    dt = np.dtype(dtype)
    A = lambda a: np.asarray(a, np.float32).astype(dt)
    pose, pts, nrm = A(pose).reshape(4, 4), A(points).reshape(-1, 3), A(normals).reshape(-1, 3)
    N = pts.shape[0]
    R = pose[:3, :3]
    ga = A(g_pc).reshape(-1, 3).copy() if g_pc is not None else np.zeros((N, 3), dt)
    gb = A(g_nc).reshape(-1, 3) if g_nc is not None else np.zeros((N, 3), dt)
    ma = np.abs(ga).astype(np.float64)
    if g_xyzf is not None:
        gx = A(g_xyzf).reshape(-1, 3)
        fs = np.asarray(fslot).reshape(-1)
        sel = fs >= 0
        ga[sel] += gx[fs[sel]]
        ma[sel] += np.abs(gx[fs[sel]])
    g_points = ga @ R
    m_points = ma @ np.abs(R.astype(np.float64))
    g_colors = None
    if g_col is not None:
        gc = A(g_col).reshape(-1, 3)
        if mode & 3:
            c = gc * (0.5 if mode & 4 else 1.0)
            sg = np.array([1, 1, 1], dt) if (mode & 3) == 2 else np.array([-1, 1, 1], dt)
            g_points = g_points + c * sg[None]
            m_points = m_points + np.abs(c)
        else:
            g_colors = gc.copy()
    elif not (mode & 3):
        g_colors = np.zeros((N, 3), dt)
    g_normals = gb @ R
    m_normals = np.abs(gb).astype(np.float64) @ np.abs(R.astype(np.float64))
    g_pose = np.zeros((3, 4), dt); m_pose = np.zeros((3, 4))
    g_pose[:, :3] = ga.T @ pts + gb.T @ nrm
    g_pose[:, 3] = ga.sum(axis=0)
    m_pose[:, :3] = ma.T @ np.abs(pts.astype(np.float64)) + np.abs(gb).astype(np.float64).T @ np.abs(nrm.astype(np.float64))
    m_pose[:, 3] = ma.sum(axis=0)
    return dict(g_points=g_points, g_normals=g_normals, g_colors=g_colors, g_pose=g_pose, mass_g_points=m_points, mass_g_normals=m_normals,
                mass_g_pose=m_pose)


# ---- iso-surface projection (grid.py:57-67) ------------------------------------------------------------------------------------------------

def surface_project_ref(xyz, sdf, J, dtype=np.float64):
    """points = x - sdf * J / ||J||, normals = J / ||J||, NOCS = (points + 1) / 2 for the band rows given"""
    dt = np.dtype(dtype)
    x, s, j = (np.asarray(v, np.float32).astype(dt) for v in (xyz, sdf, J))
    nh = j / np.sqrt((j * j).sum(1, keepdims=True))
    pts = x - s.reshape(-1, 1) * nh
    return pts, nh, (pts + 1) / 2


def surface_project_bwd_ref(n_hat, g_points, g_nocs=None, dtype=np.float64):
    """autograd of the projection w.r.t. sdf and the grid points (the unit normal is a constant: it comes from a .grad tensor, grid.py:56-58):
    g_sdf = -<g, n_hat>, g_xyz = g, with g = g_points + g_nocs / 2"""
    dt = np.dtype(dtype)
    g = np.asarray(g_points, np.float32).astype(dt)
    if g_nocs is not None:
        g = g + np.asarray(g_nocs, np.float32).astype(dt) / 2
    nh = np.asarray(n_hat, np.float32).astype(dt)
    return -(g * nh).sum(1), g, (np.abs(g) * np.abs(nh)).sum(1)


def surface_latent_grad_ref(g_sdf, J_latent, dtype=np.float64):
    """g_latent = sum_rows g_sdf[row] * d sdf[row] / d latent, and its mass"""
    dt = np.dtype(dtype)
    g = np.asarray(g_sdf, np.float32).astype(dt).reshape(-1, 1)
    Jl = np.asarray(J_latent, np.float32).astype(dt)
    return (g * Jl).sum(0), (np.abs(g) * np.abs(Jl)).astype(np.float64).sum(0)
