"""Float64 reference of the DeepSDF decoder kernels (csrc/mlp*.hip, mlp_kernel.h), numpy only, with the per-row error masses the GPU
tests judge every output element by (profiles/decoder_tests_notes.md).

The reference is built from the float32 effective layers a decoder handle is created from and holds, per arithmetic, the weights the
kernel's image holds (sdfr_decoder_create): "f32" and "split" the exact float32 values; "f16" half(w) for the hidden layers, the last
linear and all biases in float32.  The Jacobian's backward may read another image than the forward (mask_from_f16 = 1: the float32
transposed image on the masks of a half forward).  Activations are NOT rounded: every rounding belongs to the tolerance.

All tolerances have the form c * u * mass, with mass a sum of absolute values of the terms the element is made of (so it is per row,
per entry, and sensitivity weighted: a layer's rounding is carried to the output by the exact |d y / d z_l|), u the unit roundoff of the
arithmetic and c = C_BOUND[...] a constant calibrated against THIS reference run in the working precision on the CPU (the emulations
below), never against a kernel: each constant is 4 x the largest ratio the emulation reaches over all case decoders, rows and entries
(tests/test_decoder_refs_cpu.py asserts emulation <= C_BOUND / 4).  The factor 4 covers the kernels' other k partitions.
"""
import numpy as np

U32 = 2.0 ** -24          # float32 unit roundoff
USPLIT = 2.0 ** -22       # hi/lo half pairs: the product precision mlp_split.hip states
U16 = 2.0 ** -11          # half unit roundoff
SUB16 = 2.0 ** -25        # half the spacing of half's subnormals: the float16 backward stores its in-gradients unscaled (mlp_kernel.h,
                          # store_in_grad: value() goes to store4 as it is), so small ones are rounded absolutely, not relatively
LN_EPS = 1e-5

# 4 x the largest ratio  error / (u * mass)  of the CPU emulations over all decoders and rows of tests/_decoder_cases.py (measured values
# in profiles/decoder_tests_notes.md).  c_z: unit certainty.  c_t: tanh.
C_BOUND = {
    "f32_fwd": 2.2, "f32_jac": 15.2, "f32_cz": 46.0,
    "split_fwd": 0.8, "split_cz": 13.0,                 # (the Jacobian on split masks is the float32 backward: f32_jac)
    "f16_fwd": 0.32, "f16_jac": 0.8, "f16_cz": 9.0,
    "ln_fwd": 0.75, "ln_jac": 1.25, "ln_cz": 7.4,
    "c_t": 11.25,                                       # 4 x np.tanh's float32 error (1.80 u) + 2 ulp = 4 u for the device's tanhf
}


def half(a):
    return np.asarray(a, np.float32).astype(np.float16).astype(np.float32)


class Net:
    """The layers a decoder handle is created from: [(W[out, in], b[out])] float32, the injection table [(n, off)], LayerNorm
    parameters [None | (gamma, beta)], use_tanh."""

    def __init__(self, layers, inj, ln=None, use_tanh=False):
        self.W = [np.asarray(W, np.float32) for W, _ in layers]
        self.b = [np.asarray(b, np.float32) for _, b in layers]
        self.inj = [tuple(int(v) for v in i) for i in inj]
        self.ln = list(ln) if ln is not None else [None] * len(layers)
        self.ln = [None if p is None else (np.asarray(p[0], np.float32), np.asarray(p[1], np.float32)) for p in self.ln]
        self.use_tanh = bool(use_tanh)
        self.n_lin = len(layers)
        self.n_inputs = int(self.W[0].shape[1])
        self.has_ln = any(p is not None for p in self.ln)
        width = max(max(W.shape[0] for W in self.W[:-1]), max(W.shape[1] for W in self.W))
        self.hp = 128 if width <= 128 else (256 if width <= 256 else 512)
        self.out_dims = [int(W.shape[0]) for W in self.W[:-1]]

    @classmethod
    def from_decoder(cls, dec):
        ln = []
        for l in range(dec.num_layers - 1):
            bn = getattr(dec, "bn" + str(l), None)
            ln.append(None if bn is None else (bn.weight.detach().float().numpy(), bn.bias.detach().float().numpy()))
        return cls(dec.effective_layers(), dec._inject_table(), ln, dec.use_tanh)

    def weights(self, arith):
        """float64 weights of the image `arith` reads: 'f32' / 'split' the exact values, 'f16' half(w) in the hidden layers"""
        if arith == "f16":
            return [half(W).astype(np.float64) for W in self.W[:-1]] + [self.W[-1].astype(np.float64)]
        return [W.astype(np.float64) for W in self.W]


class Result:
    pass


def _ln_fwd(lin, gamma, beta):
    mu = lin.mean(1, keepdims=True)
    var = ((lin - mu) ** 2).mean(1, keepdims=True)              # biased, as nn.LayerNorm
    rstd = 1.0 / np.sqrt(var + LN_EPS)
    xh = (lin - mu) * rstd
    return xh * gamma + beta, xh, rstd


def evaluate(net, x, arith="f32", masks=None, bwd=None, want_masses=True):
    """The reference on rows x (n, n_inputs).  masks: the ReLU decisions to use ([bool (n, out_l)] per hidden layer; default: the
    reference's own z_l > 0) -- activations, sensitivities, J and all masses are those of the piecewise-linear branch the masks select.
    bwd: the image the Jacobian's backward reads ('f32' | 'f16'; default: the forward's).

    Returns r with, per hidden layer l, lists  z (what the ReLU sees), a, xin (the layer's input, re-injected columns included), linmass
    (|W||xin| + |b|), zmass (the same carried through LayerNorm), mask, g (d y / d z_l, masked) and glin (d y / d linear output of l);
    y (pre-tanh), y1, out, gy (d out / d y), Jy = d y / d input, J = gy Jy (n, n_inputs), the forward-mode blocks A (d a_l / d input:
    (n, out_l, n_inputs)) and the masses M_fwd, M_half, MJ, MJ_half, MJ_sub."""
    x = np.asarray(x, np.float64)
    n, ni = x.shape
    Wf = net.weights(arith)
    Wb = net.weights(bwd or arith)
    b = [v.astype(np.float64) for v in net.b]
    nh = net.n_lin - 1
    r = Result()
    r.z, r.a, r.xin, r.linmass, r.zmass, r.mask = [], [], [], [], [], []
    xh_l, rstd_l, lna_l = [], [], []
    cur = x
    for l in range(nh):
        inj_n, inj_off = net.inj[l]
        if inj_n:
            cur = np.concatenate([cur, x[:, inj_off:inj_off + inj_n]], 1)
        lin = cur @ Wf[l].T + b[l]
        lm = np.abs(cur) @ np.abs(Wf[l]).T + np.abs(b[l])
        if net.ln[l] is not None:
            gam, bet = (v.astype(np.float64) for v in net.ln[l])
            z, xh, rstd = _ln_fwd(lin, gam, bet)
            # first order: d x_hat_j = rstd (d_j - mean d) - x_hat_j rstd mean(x_hat d), |mean(x_hat d)| <= sqrt(mean d^2)
            # ... plus LayerNorm's own arithmetic (mean, variance, normalise, scale and shift)
            la = np.abs(gam) * (rstd * np.abs(lin).mean(1, keepdims=True) + 2.0 * np.abs(xh)) + np.abs(z)
            zm = np.abs(gam) * rstd * (lm + lm.mean(1, keepdims=True) + np.abs(xh) * np.sqrt((lm ** 2).mean(1, keepdims=True))) + la
        else:
            z, xh, rstd, zm, la = lin, None, None, lm, None
        lna_l.append(la)
        m = (z > 0) if masks is None else np.asarray(masks[l], bool)[:, :z.shape[1]]
        r.xin.append(cur); r.z.append(z); r.linmass.append(lm); r.zmass.append(zm); r.mask.append(m)
        xh_l.append(xh); rstd_l.append(rstd)
        cur = np.where(m, z, 0.0)
        r.a.append(cur)
    inj_n, inj_off = net.inj[nh]
    if inj_n:
        cur = np.concatenate([cur, x[:, inj_off:inj_off + inj_n]], 1)
    r.xin.append(cur)
    wl, bl = Wf[nh][0], b[nh][0]
    r.y = cur @ wl + bl
    r.ymass = np.abs(cur) @ np.abs(wl) + abs(bl)
    r.y1 = np.tanh(r.y) if net.use_tanh else r.y
    r.out = np.tanh(r.y1)
    r.gy = (1.0 - r.out ** 2) * ((1.0 - r.y1 ** 2) if net.use_tanh else 1.0)

    # ---- reverse mode: d y / d input, with the backward image ----
    Jy = np.zeros((n, ni))
    r.g, r.glin = [None] * nh, [None] * nh
    h = np.broadcast_to(Wb[nh][0], (n, Wb[nh].shape[1])).copy()       # d y / d xin of the last linear
    for l in range(nh - 1, -1, -1):
        inj_n, inj_off = net.inj[l + 1]
        od = net.out_dims[l]
        if inj_n:
            Jy[:, inj_off:inj_off + inj_n] += h[:, od:od + inj_n]
        g = np.where(r.mask[l], h[:, :od], 0.0)
        r.g[l] = g
        if net.ln[l] is not None:
            gam = net.ln[l][0].astype(np.float64)
            gg = g * gam
            glin = rstd_l[l] * (gg - gg.mean(1, keepdims=True) - xh_l[l] * (gg * xh_l[l]).mean(1, keepdims=True))
        else:
            glin = g
        r.glin[l] = glin
        h = glin @ Wb[l]
    inj_n, inj_off = net.inj[0]
    Jy += h[:, :ni]
    r.Jy = Jy
    r.J = r.gy[:, None] * Jy
    if not want_masses:
        return r

    # ---- forward sensitivities with the FORWARD image (they carry the forward's roundings to y) ----
    if (bwd or arith) == arith:
        gl_f = r.glin
        g_f = r.g
    else:
        rf = evaluate(net, x, arith, masks=r.mask, want_masses=False)
        gl_f, g_f = rf.glin, rf.g
    r.M_fwd = r.ymass + np.abs(r.y)
    r.M_half = np.abs(cur) @ np.abs(wl)
    for l in range(nh):
        r.M_fwd = r.M_fwd + (np.abs(gl_f[l]) * r.linmass[l]).sum(1)
        r.M_half = r.M_half + (np.abs(gl_f[l]) * (r.linmass[l] - np.abs(b[l]))).sum(1)
        if net.ln[l] is not None:          # LayerNorm's own arithmetic, seen by d y / d z
            r.M_fwd = r.M_fwd + (np.abs(g_f[l]) * lna_l[l]).sum(1)

    # ---- forward mode: X_l = d xin_l / d input, for the Jacobian's masses ----
    eye = np.broadcast_to(np.eye(ni), (n, ni, ni))
    X = eye
    MJ = np.zeros((n, ni)); MJh = np.zeros((n, ni)); MJs = np.zeros((n, ni))
    r.A = []
    aWb = [np.abs(W) for W in Wb]
    for l in range(nh):
        inj_n, inj_off = net.inj[l]
        if inj_n:
            X = np.concatenate([X, eye[:, inj_off:inj_off + inj_n, :]], 1)
        MJ += np.einsum("nu,nuj->nj", np.abs(r.glin[l]) @ aWb[l], np.abs(X))
        dlin = np.matmul(Wb[l][None], X)                      # (n, out, ni)
        if net.ln[l] is not None:
            gam = net.ln[l][0].astype(np.float64)
            xh, rstd = xh_l[l][:, :, None], rstd_l[l][:, :, None]
            dz = gam[None, :, None] * rstd * (dlin - dlin.mean(1, keepdims=True) - xh * (xh * dlin).mean(1, keepdims=True))
            gg = np.abs(r.g[l] * gam)
            lnm = rstd_l[l] * (gg + gg.mean(1, keepdims=True) + np.abs(xh_l[l]) * (gg * np.abs(xh_l[l])).mean(1, keepdims=True))
            MJ += np.einsum("nu,nuj->nj", lnm, np.abs(dlin))
        else:
            dz = dlin
        X = np.where(r.mask[l][:, :, None], dz, 0.0)          # A_l = d a_l / d input
        r.A.append(X)
        MJh += np.einsum("nu,nuj->nj", np.abs(r.g[l]), np.abs(X))
        MJs += np.abs(X).sum(1)
    inj_n, inj_off = net.inj[nh]
    if inj_n:
        X = np.concatenate([X, eye[:, inj_off:inj_off + inj_n, :]], 1)
    MJ += np.einsum("u,nuj->nj", aWb[nh][0], np.abs(X))
    r.MJ, r.MJ_half, r.MJ_sub = MJ, MJh, MJs
    return r


# ---- tolerances -----------------------------------------------------------------------------------------------------------------

def _cls(net, arith):
    return "ln" if net.has_ln else arith


def pre_unit(net, r, arith):
    """u * mass of the pre-tanh value y per row, before the constant"""
    if arith == "f16":
        return U32 * r.M_fwd + U16 * r.M_half
    return (USPLIT if arith == "split" else U32) * r.M_fwd


def fwd_unit(net, r, arith):
    """... of `out`: the pre-tanh roundings carried through d out / d y"""
    return r.gy * pre_unit(net, r, arith)


def tanh_unit(net, r):
    """one rounding of tanh's result (two with use_tanh, the inner one carried through the outer tanh)"""
    t = U32 * np.abs(r.out)
    if net.use_tanh:
        t = t + U32 * np.abs(r.y1) * (1.0 - r.out ** 2)
    return t


def fwd_tol(net, r, arith, scale=1.0):
    """|out_kernel - out_ref| <= this, per row.  scale = 1/4: what the CPU emulation must meet."""
    return scale * (C_BOUND[_cls(net, arith) + "_fwd"] * fwd_unit(net, r, arith) + C_BOUND["c_t"] * tanh_unit(net, r))


def jac_unit(net, r, bwd):
    """u * mass of J per entry, the backward's own roundings only"""
    if bwd == "f16":
        return r.gy[:, None] * (U32 * r.MJ + U16 * r.MJ_half) + SUB16 * r.MJ_sub
    return r.gy[:, None] * (U32 * r.MJ)


def jac_out_term(net, r, out_tol):
    """the output derivative is formed from the kernel's own out (and y1 with use_tanh): |J| 2 |out| / (1 - out^2) per unit of its error"""
    with np.errstate(divide="ignore", invalid="ignore"):
        s = 2.0 * np.abs(r.out) / (1.0 - r.out ** 2)
        if net.use_tanh:
            s = s + 2.0 * np.abs(r.y1) / ((1.0 - r.y1 ** 2) * (1.0 - r.out ** 2))
        t = np.abs(r.J) * (s * out_tol)[:, None]
    # (a row saturated in float64, out = +-1 exactly, has J = 0 in the reference and in any float32 evaluation: 0 * inf -> 0)
    return np.where(np.isfinite(t), t, 0.0)


def jac_tol(net, r, fwd_arith, bwd, scale=1.0):
    cls = "ln" if net.has_ln else bwd
    return scale * C_BOUND[cls + "_jac"] * jac_unit(net, r, bwd) + jac_out_term(net, r, fwd_tol(net, r, fwd_arith, scale))


def free_units(net, r, arith):
    """[bool (n, out_l)]: units whose ReLU decision the arithmetic may take either way: |z_ref| <= c_z u zmass"""
    u = U16 if arith == "f16" else (USPLIT if arith == "split" else U32)
    c = C_BOUND[_cls(net, arith) + "_cz"]
    return [np.abs(z) <= c * u * zm for z, zm in zip(r.z, r.zmass)]


# ---- the saved ReLU masks (layout v2 of mlp_kernel.h: sdfr_mask_dword / sdfr_mask_shift), restated in Python ------------------------

def mask_shift(j):
    j = np.asarray(j)
    return ((j >> 2) & 1) * 16 + ((j & 31) >> 3) * 4 + (j & 3)


def mask_words(n, n_layers, hp):
    return ((n + 127) // 128) * n_layers * 128 * (hp // 32)


def mask_decode(ws, rows, n_layers, hp):
    """bool (len(rows), n_layers, hp) from the workspace dwords"""
    ws = np.asarray(ws).view(np.uint32).reshape(-1, n_layers, 128, hp // 32)
    rows = np.asarray(rows, np.int64)
    w = ws[rows >> 7, :, rows & 127, :]                       # (n, layers, hp / 32)
    j = np.arange(hp)
    return ((w[:, :, j >> 5] >> mask_shift(j).astype(np.uint32)) & 1).astype(bool)


def mask_encode(bits):
    """uint32 workspace of rows 0 .. n-1 from bool (n, n_layers, hp)"""
    n, nl, hp = bits.shape
    ws = np.zeros(((n + 127) // 128, nl, 128, hp // 32), np.uint32)
    rows = np.arange(n)
    j = np.arange(hp)
    sh = mask_shift(j).astype(np.uint32)
    contrib = bits.astype(np.uint32) << sh                    # (n, nl, hp)
    w = np.zeros((n, nl, hp // 32), np.uint32)
    for jj in range(hp):
        w[:, :, jj >> 5] |= contrib[:, :, jj]
    ws[rows >> 7, :, rows & 127, :] = w
    return ws.reshape(-1)


# ---- emulations: the reference's recurrence in the working precision, the worst summation order a kernel uses ----------------------

def _seq_matmul(x, W):
    """float32 x (n, k) times W (out, k) transposed, accumulated strictly in k order from 0"""
    acc = np.zeros((x.shape[0], W.shape[0]), np.float32)
    for k in range(W.shape[1]):
        acc += x[:, k:k + 1] * W[None, :, k]
    return acc


def _seq_sum(v):
    return np.cumsum(v.astype(np.float32), axis=1, dtype=np.float32)[:, -1:]


def emulate(net, x, arith="f32", bwd=None, masks=None, drop=None, bwd_masks=None):
    """y, y1, out, J (float32), the masks and the z values (a Result) of a run in the working precision.  arith: 'f32' (also LayerNorm decoders), 'f16'
    (operands rounded to half where the kernel rounds them: inputs, re-injected columns, hidden activations, half weight image),
    'split' (hi/lo pairs, main and correction accumulators).  bwd: 'f32' | 'f16' (in-gradients rounded to half between layers, half
    transposed image).  masks: use these instead of the run's own (the mask-fed Jacobian of given masks).  drop = (layer, row, k0): a planted
    defect for the tests of the judges -- that row's product of that layer skips the 16-wide K tile at k0; bwd_masks: the backward alone
    reads these masks (another planted defect: the forward and its output stay what they were)."""
    f = np.float32
    bwd = bwd or ("f16" if arith == "f16" else "f32")
    x = np.asarray(x, f)
    n, ni = x.shape
    nh = net.n_lin - 1
    W = [half(w) if arith == "f16" else w for w in net.W[:-1]] + [net.W[-1]]
    Wb = [half(w) if bwd == "f16" else w for w in net.W[:-1]] + [net.W[-1]]
    rnd = half if arith == "f16" else (lambda v: v)
    ms, zs, xhs, rss = [], [], [], []
    cur = rnd(x)
    for l in range(nh):
        inj_n, inj_off = net.inj[l]
        if inj_n:
            cur = np.concatenate([cur, rnd(x[:, inj_off:inj_off + inj_n])], 1)
        if drop is not None and drop[0] == l:
            cur = cur.copy()
            cur[drop[1], drop[2]:drop[2] + 16] = 0
        if arith == "split":
            ah, bh = half(cur), half(W[l])
            al, bl = half((cur - ah) * f(2048)), half((W[l] - bh) * f(2048))
            acc = _seq_matmul(ah, bh)
            cor = np.zeros_like(acc)
            for k in range(bh.shape[1]):
                cor += ah[:, k:k + 1] * bl[None, :, k]
                cor += al[:, k:k + 1] * bh[None, :, k]
            z = (acc + cor * f(1.0 / 2048)) + net.b[l]
        else:
            z = _seq_matmul(cur, W[l]) + net.b[l]
        if net.ln[l] is not None:
            gam, bet = net.ln[l]
            mu = _seq_sum(z) / f(z.shape[1])
            var = _seq_sum((z - mu) * (z - mu)) / f(z.shape[1])
            rs = f(1) / np.sqrt(var + f(LN_EPS))
            xh = (z - mu) * rs
            z = xh * gam + bet
            xhs.append(xh); rss.append(rs)
        else:
            xhs.append(None); rss.append(None)
        m = (z > 0) if masks is None else np.asarray(masks[l], bool)
        zs.append(z); ms.append(m)
        cur = rnd(np.where(m, z, f(0)))
    inj_n, inj_off = net.inj[nh]
    if inj_n:
        cur = np.concatenate([cur, rnd(x[:, inj_off:inj_off + inj_n])], 1)
    y = (_seq_matmul(cur, W[nh]) + net.b[nh])[:, 0]
    y1 = np.tanh(y) if net.use_tanh else y
    out = np.tanh(y1).astype(f)
    gy = (f(1) - out * out) * ((f(1) - y1 * y1) if net.use_tanh else f(1))
    rb = half if bwd == "f16" else (lambda v: v)
    J = np.zeros((n, ni), f)
    h = Wb[nh][0][None, :] * gy[:, None]
    for l in range(nh - 1, -1, -1):
        inj_n, inj_off = net.inj[l + 1]
        od = net.out_dims[l]
        if inj_n:
            J[:, inj_off:inj_off + inj_n] += h[:, od:od + inj_n]
        g = np.where((bwd_masks or ms)[l], h[:, :od], f(0))
        if net.ln[l] is not None:
            gg = g * net.ln[l][0]
            m1 = _seq_sum(gg) / f(od)
            m2 = _seq_sum(gg * xhs[l]) / f(od)
            g = rss[l] * (gg - m1 - xhs[l] * m2)
        h = _seq_matmul(rb(g), np.ascontiguousarray(Wb[l].T))
    J += h[:, :ni]
    e = Result()
    e.y, e.y1, e.out, e.J, e.mask, e.z = y, y1, out, J, ms, zs
    return e


def emulation_ratios(net, x, arith, bwd=None):
    """largest error / (u * mass) of the emulation against the reference, per quantity: what C_BOUND is calibrated from (x 4).
    'jac' is the backward's own roundings only: the part of |J_e - J_ref| that the emulation's own error of `out` explains (jac_out_term
    of that error) is taken off first, because jac_tol adds jac_out_term(fwd_tol) on top of C_BOUND[*_jac] * jac_unit -- whoever
    recalibrates must keep that split, or the output derivative's error would be counted twice."""
    e = emulate(net, x, arith, bwd)
    r0 = evaluate(net, x, arith, bwd=bwd)
    rm = evaluate(net, x, arith, masks=e.mask, bwd=bwd)
    u = U16 if arith == "f16" else (USPLIT if arith == "split" else U32)
    out = {}
    out["fwd"] = float((np.abs(e.y - r0.y) / pre_unit(net, r0, arith)).max())
    out["cz"] = max(float((np.abs(z - z0) / (u * zm)).max()) for z, z0, zm in zip(e.z, r0.z, r0.zmass))
    t = Result()
    t.y1 = np.tanh(e.y.astype(np.float64)) if net.use_tanh else e.y.astype(np.float64)
    t.out = np.tanh(t.y1)
    nz = np.abs(t.out) > 0
    out["tanh"] = float((np.abs(e.out - t.out)[nz] / tanh_unit(net, t)[nz]).max()) if nz.any() else 0.0
    own = jac_out_term(net, rm, np.abs(e.out - rm.out) * 1.01 + 1e-300)
    out["jac"] = float(_ratio(np.maximum(np.abs(e.J - rm.J) - own, 0.0), jac_unit(net, rm, bwd or ("f16" if arith == "f16" else "f32"))).max())
    out["free"] = float(np.mean(np.concatenate([f.ravel() for f in free_units(net, r0, arith)])))
    return out, e, r0, rm


# ---- judges: what the GPU tests (and the CPU dry runs on the emulations) assert ----------------------------------------------------

def _ratio(err, tol):
    """err / tol; 0 / 0 = 0; a non-finite error (a NaN or inf in the kernel's output) is inf, never NaN: no reduction may skip it"""
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(tol > 0, err / tol, np.where(err == 0, 0.0, np.inf))
    return np.where(np.isfinite(err), r, np.inf)


def judge_forward(net, r, out, arith, scale=1.0):
    """per row |out - out_ref| / tolerance (<= 1 passes)"""
    return _ratio(np.abs(np.asarray(out, np.float64) - r.out), fwd_tol(net, r, arith, scale))


def judge_masks(net, r, bits, arith):
    """bits: bool (n, layers, hp) decoded from the workspace.  Returns (certain units whose bit is not z_ref > 0, share of free units)"""
    free = free_units(net, r, arith)
    bad = sum(int(((bits[:, l, :z.shape[1]] != (z > 0)) & ~f).sum()) for l, (z, f) in enumerate(zip(r.z, free)))
    return bad, float(np.mean(np.concatenate([f.ravel() for f in free])))


def judge_jac_masks(net, x, masks, J, fwd_arith, bwd, scale=1.0):
    """the mask-fed Jacobian: per entry |J - J_ref(masks)| / tolerance, the reference evaluated with the KERNEL's masks"""
    rm = evaluate(net, x, fwd_arith, masks=masks, bwd=bwd)
    return _ratio(np.abs(np.asarray(J, np.float64) - rm.J), jac_tol(net, rm, fwd_arith, bwd, scale))


def judge_jac_recompute(net, x, r0, J, arith="f32", scale=1.0, max_free=3):
    """the recomputing Jacobian: a row with k <= 3 free units must match one of the 2^k reference Jacobians; rows with more are left out.
    Returns (per-row ratio, bool mask of the rows left out): the caller reduces with .max() over the rows kept -- a non-finite J is inf
    there, and a row is left out by the REFERENCE's count of free units alone, never by what the kernel wrote."""
    J = np.asarray(J, np.float64)
    free = free_units(net, r0, arith)
    k = sum(f.sum(1) for f in free)
    ratio = _ratio(np.abs(J - r0.J), jac_tol(net, r0, arith, "f32", scale)).max(1)
    for i in np.nonzero((k > 0) & (k <= max_free) & (ratio > 1))[0]:
        where = [(l, int(j)) for l, f in enumerate(free) for j in np.nonzero(f[i])[0]]
        nc = 1 << len(where)
        masks = [np.repeat(m[i:i + 1], nc, 0) for m in r0.mask]
        for c in range(nc):
            for b, (l, j) in enumerate(where):
                masks[l][c, j] = bool((c >> b) & 1)
        xs = np.repeat(np.asarray(x)[i:i + 1], nc, 0)
        rc = evaluate(net, xs, arith, masks=masks, bwd="f32")
        ratio[i] = _ratio(np.abs(J[i:i + 1] - rc.J), jac_tol(net, rc, arith, "f32", scale)).max(1).min()
    return ratio, k > max_free
