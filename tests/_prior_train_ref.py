"""Float64 numpy restatement of the decoder's training kernels (csrc/mlp_train.hip, train_cells.h): the forward with a GIVEN keep mask,
the backward with a GIVEN local-derivative pattern, the dropout hash, the chunked summation order of dW, and the per-element error masses
the GPU tests judge every output by (profiles/prior_train_notes.md).  The float32 emulations the constants are calibrated on are here too;
nothing is calibrated against a kernel.  Nets are tests/_decoder_ref.Net.
"""
import numpy as np

from tests._decoder_ref import C_BOUND as DEC_C, U32, Net, _ratio, _seq_matmul  # noqa: F401

CHUNK = 1024
HEADER = 16
GOLDEN = 0x9E3779B97F4A7C15
M64 = (1 << 64) - 1

# 4 x the largest ratio error / (u mass) of the float32 emulation below over the cases of tests/_prior_train_cases.py (measured values in
# profiles/prior_train_notes.md; tests/test_prior_train_cpu.py asserts emulation <= C / 4 and that C is not looser than 4 x measured, rounded up)
C = {"c_fwd": 1.23, "c_dx": 0.92, "c_dw": 3.37, "c_z": 32.8, "c_t": DEC_C["c_t"]}
FREE_CAP = 1e-3


class R:
    pass


# ---- the dropout hash (train_cells.h) -----------------------------------------------------------------------------------------------

def mix64(z):
    z = np.asarray(z, np.uint64)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def drop_word(seed, layer, rows, features):
    """uint32 (len(rows), len(features)): the 24-bit word of every unit"""
    with np.errstate(over="ignore"):
        key = (np.asarray(rows, np.uint64)[:, None] << np.uint64(14)) | np.uint64(int(layer) << 10) | np.asarray(features, np.uint64)[None, :]
        h = mix64(np.uint64(int(seed) & M64) ^ mix64(key * np.uint64(GOLDEN) + np.uint64(1)))
    return (h >> np.uint64(40)).astype(np.uint32)


def drop_threshold(p):
    return int(np.rint(float(np.float32(p)) * 16777216.0))


def keep_mask(seed, layer, n, width, p, row0=0):
    """bool (n, width); p = 0 keeps all without a hash"""
    if p <= 0:
        return np.ones((n, width), bool)
    return drop_word(seed, layer, np.arange(row0, row0 + n), np.arange(width)) >= np.uint32(drop_threshold(p))


def keep_masks(net, seed, n, p, drop_layers):
    return [keep_mask(seed, l, n, net.out_dims[l], p if (drop_layers >> l) & 1 else 0.0) for l in range(net.n_lin - 1)]


def scales(net, p, drop_layers):
    """float32 1 / (1 - p) of the layers that drop, 1 of the others, as float64 values"""
    s = float(np.float32(1.0) / (np.float32(1.0) - np.float32(p))) if p > 0 else 1.0
    return [s if (p > 0 and (drop_layers >> l) & 1) else 1.0 for l in range(net.n_lin - 1)]


# ---- workspace layout (include/sdfr.h) ----------------------------------------------------------------------------------------------

def layout(net, n):
    in_dim = [int(W.shape[1]) for W in net.W]
    out_dim = [int(W.shape[0]) for W in net.W]
    L = R()
    at = HEADER
    L.x0 = at
    at += n * in_dim[0]
    L.act = []
    for l in range(net.n_lin - 1):
        L.act.append(at)
        at += n * in_dim[l + 1]
    L.tail = at
    at += 2 * n
    mo = max(out_dim)
    L.delta = (at, at + n * mo)
    at += 2 * n * mo
    L.ginj = [0] * net.n_lin
    for l in range(1, net.n_lin):
        L.ginj[l] = at
        at += n * net.inj[l][0]
    L.part = at
    L.chunks = (n + CHUNK - 1) // CHUNK
    at += L.chunks * max(o * i + o for o, i in zip(out_dim, in_dim))
    L.total = at
    L.in_dim, L.out_dim = in_dim, out_dim
    return L


# ---- float64 forward / backward ------------------------------------------------------------------------------------------------------

def forward(net, x, keep=None, scale=None):
    """keep: [bool (n, out_l)] per hidden layer (None: all kept); scale: [float] per hidden layer (None: 1).  Returns r with lists z (the
    pre-activations), a (after ReLU, dropout and its scale), xin (every layer's input, re-injected columns included), linmass, and y, y1,
    out (= sdf), gy."""
    x = np.asarray(x, np.float64)
    nh = net.n_lin - 1
    W = [w.astype(np.float64) for w in net.W]
    b = [v.astype(np.float64) for v in net.b]
    r = R()
    r.z, r.a, r.xin, r.linmass, r.relu = [], [], [], [], []
    r.keep = [np.ones((x.shape[0], net.out_dims[l]), bool) if keep is None else np.asarray(keep[l], bool) for l in range(nh)]
    r.scale = [1.0] * nh if scale is None else [float(s) for s in scale]
    cur = x
    for l in range(nh + 1):
        inj_n, inj_off = net.inj[l]
        if inj_n:
            cur = np.concatenate([cur, x[:, inj_off:inj_off + inj_n]], 1)
        r.xin.append(cur)
        z = cur @ W[l].T + b[l]
        r.linmass.append(np.abs(cur) @ np.abs(W[l]).T + np.abs(b[l]))
        if l == nh:
            break
        r.z.append(z)
        r.relu.append(z > 0)
        cur = np.where((z > 0) & r.keep[l], z * r.scale[l], 0.0)
        r.a.append(cur)
    r.y = z[:, 0]
    r.y1 = np.tanh(r.y) if net.use_tanh else r.y
    r.out = np.tanh(r.y1)
    r.gy = (1.0 - r.out ** 2) * ((1.0 - r.y1 ** 2) if net.use_tanh else 1.0)
    r.x = x
    return r


def local_derivative(r):
    """the reference's own pattern: scale where the unit is alive and kept, else 0"""
    return [np.where(m & k, s, 0.0) for m, k, s in zip(r.relu, r.keep, r.scale)]


def backward(net, r, g_sdf, deriv=None, tail=None, want_masses=True):
    """deriv: [float (n, out_l)] the local derivative of every hidden activation (None: the reference's own); tail = (y1, out) the values
    the output derivative is formed from (None: the reference's own).  Returns b with g_inputs (n, n_inputs), dW [ (out, in) ], db [ (out,) ],
    d [ (n, out_l) ] and, with want_masses, M_fwd (n,), zmass, M_gin, M_dW, M_db."""
    nh = net.n_lin - 1
    W = [w.astype(np.float64) for w in net.W]
    aW = [np.abs(w) for w in W]
    deriv = local_derivative(r) if deriv is None else [np.asarray(d, np.float64) for d in deriv]
    y1, out = (r.y1, r.out) if tail is None else (np.asarray(tail[0], np.float64), np.asarray(tail[1], np.float64))
    gy = (1.0 - out ** 2) * ((1.0 - y1 ** 2) if net.use_tanh else 1.0)
    g_sdf = np.asarray(g_sdf, np.float64).reshape(-1)
    n, ni = r.x.shape
    b = R()
    b.dW, b.db, b.d = [None] * (nh + 1), [None] * (nh + 1), [None] * (nh + 1)
    b.M_dW, b.M_db = [None] * (nh + 1), [None] * (nh + 1)

    # forward error masses of the activations (first order, absolute weights): what the kernel's stored xin may differ by, per u
    Ma = [np.zeros_like(r.x)]                                           # of xin_0
    cur = Ma[0]
    for l in range(nh):
        mz = r.linmass[l] + cur @ aW[l].T
        ma = np.abs(deriv[l]) * (mz + np.abs(r.z[l]))
        inj_next = net.inj[l + 1][0]
        cur = np.concatenate([ma, np.zeros((n, inj_next))], 1) if inj_next else ma
        Ma.append(cur)

    d = (g_sdf * gy)[:, None]
    Md = np.abs(d) * 3.0                                                # 1 - o o, (* 1 - y1 y1), * g
    ginj, Mginj, el = {}, {}, {}
    for l in range(nh, -1, -1):
        b.d[l] = d
        b.dW[l] = d.T @ r.xin[l]
        b.db[l] = d.sum(0)
        if want_masses:
            b.M_dW[l] = (np.abs(d) + Md).T @ np.abs(r.xin[l]) + np.abs(d).T @ Ma[l]
            b.M_db[l] = (np.abs(d) + Md).sum(0)
        H = d @ W[l]
        MH = (np.abs(d) + Md) @ aW[l]
        el[l] = np.abs(d) @ aW[l] + np.abs(H)
        if l == 0:
            break
        od = net.out_dims[l - 1]
        inj_n, inj_off = net.inj[l]
        if inj_n:
            ginj[l], Mginj[l] = H[:, od:od + inj_n], MH[:, od:od + inj_n]
        d = H[:, :od] * deriv[l - 1]
        Md = np.abs(deriv[l - 1]) * MH[:, :od] + np.abs(d)
    g = H[:, :ni].copy()
    for l in sorted(ginj):
        inj_n, inj_off = net.inj[l]
        g[:, inj_off:inj_off + inj_n] += ginj[l]
    # the roundings of every product h_l = d_l W_l (|d_l| |W_l| + |h_l| per element of xin_l) carried to input column j by the exact
    # |d xin_l / d input_j| on this branch (forward mode, as MJ of tests/_decoder_ref.py), plus d's own three roundings and the final sums
    Mg = 4.0 * np.abs(g)
    if want_masses:
        eye = np.broadcast_to(np.eye(ni), (n, ni, ni))
        X = eye
        for l in range(nh + 1):
            inj_n, inj_off = net.inj[l]
            if inj_n:
                X = np.concatenate([X, eye[:, inj_off:inj_off + inj_n, :]], 1)
            Mg = Mg + np.einsum("nu,nuj->nj", el[l], np.abs(X))
            if l < nh:
                X = deriv[l][:, :, None] * np.matmul(W[l][None], X)
    b.g_inputs, b.M_gin = g, Mg
    if want_masses:
        # M_fwd of profiles/decoder_tests_notes.md: the roundings of every layer carried to y by the exact |d y / d z_l|, on this branch
        h = W[nh][0][None, :].repeat(n, 0)
        M = r.linmass[nh][:, 0] + np.abs(r.y)
        for l in range(nh - 1, -1, -1):
            gz = h[:, :net.out_dims[l]] * deriv[l]
            extra = np.abs(r.z[l]) if r.scale[l] != 1.0 else 0.0
            M = M + (np.abs(gz) * (r.linmass[l] + extra)).sum(1)
            h = gz @ W[l]
        b.M_fwd = M
        b.zmass = r.linmass[:nh]
    return b


def fwd_tol(net, r, b, scale=1.0):
    t = U32 * np.abs(r.out)
    if net.use_tanh:
        t = t + U32 * np.abs(r.y1) * (1.0 - r.out ** 2)
    return scale * (C["c_fwd"] * r.gy * U32 * b.M_fwd + C["c_t"] * t)


def free_units(r):
    """[bool (n, out_l)]: |z_ref| <= c_z u linmass -- the float32 pre-activation may fall on either side of zero"""
    return [np.abs(z) <= C["c_z"] * U32 * m for z, m in zip(r.z, r.linmass[:len(r.z)])]


# ---- float32 emulation: strictly sequential k for the forward and dX, chunk order for dW -------------------------------------------

def _seq_rows(d, xin):
    """float32 d^T xin and column sums of d: rows in order inside chunks of CHUNK, chunk sums added in chunk order from 0"""
    f = np.float32
    n = d.shape[0]
    dw = np.zeros((d.shape[1], xin.shape[1]), f)
    db = np.zeros((d.shape[1],), f)
    for c0 in range(0, n, CHUNK):
        pw = np.zeros_like(dw)
        pb = np.zeros_like(db)
        for i in range(c0, min(n, c0 + CHUNK)):
            pw += d[i][:, None] * xin[i][None, :]
            pb += d[i]
        dw += pw
        db += pb
    return dw, db


def emulate(net, x, g_sdf, keep=None, scale=None):
    """the recurrence in float32.  Returns e with sdf, y1, a (the stored activations), z, g_inputs, dW, db."""
    f = np.float32
    x = np.asarray(x, f)
    n, ni = x.shape
    nh = net.n_lin - 1
    sc = [f(1)] * nh if scale is None else [f(s) for s in scale]
    e = R()
    e.z, e.a, xin = [], [], []
    cur = x
    for l in range(nh + 1):
        inj_n, inj_off = net.inj[l]
        if inj_n:
            cur = np.concatenate([cur, x[:, inj_off:inj_off + inj_n]], 1)
        xin.append(cur)
        z = _seq_matmul(cur, net.W[l]) + net.b[l]
        if l == nh:
            break
        e.z.append(z)
        a = np.where(z > 0, z, f(0))
        if keep is not None and sc[l] != f(1):
            a = np.where(keep[l], a * sc[l], f(0))
        elif keep is not None:
            a = np.where(keep[l], a, f(0))
        cur = a.astype(f)
        e.a.append(cur)
    y = z[:, 0]
    e.y = y
    e.y1 = (np.tanh(y) if net.use_tanh else y).astype(f)
    e.sdf = np.tanh(e.y1).astype(f)
    gy = f(1) - e.sdf * e.sdf
    if net.use_tanh:
        gy = gy * (f(1) - e.y1 * e.y1)
    d = (np.asarray(g_sdf, f).reshape(-1) * gy)[:, None].astype(f)
    e.dW, e.db = [None] * (nh + 1), [None] * (nh + 1)
    ginj = {}
    for l in range(nh, -1, -1):
        e.dW[l], e.db[l] = _seq_rows(d, xin[l])
        H = _seq_matmul(d, np.ascontiguousarray(net.W[l].T))
        if l == 0:
            break
        od = net.out_dims[l - 1]
        inj_n, inj_off = net.inj[l]
        if inj_n:
            ginj[l] = H[:, od:od + inj_n]
        d = np.where(e.a[l - 1] > 0, H[:, :od] * sc[l - 1], f(0)).astype(f)
    g = H[:, :ni].copy()
    for l in sorted(ginj):
        inj_n, inj_off = net.inj[l]
        g[:, inj_off:inj_off + inj_n] += ginj[l]
    e.g_inputs = g
    return e


def deriv_from_acts(acts, scale):
    """the local-derivative pattern the kernels' backward applies: scale where the stored activation is > 0"""
    return [np.where(np.asarray(a) > 0, float(s), 0.0) for a, s in zip(acts, scale)]


def judge(net, x, g_sdf, keep, scale, sdf, y1, acts, g_inputs, dW, db, q=1.0):
    """What the GPU tests assert, on any implementation's outputs (the emulation's in the CPU tests, with q = 1/4): a dict of the largest
    ratios error / tolerance (<= 1 passes) and the counts of the unit checks."""
    r = forward(net, x, keep, scale)
    b0 = backward(net, r, g_sdf)
    out = {}
    out["fwd"] = float(_ratio(np.abs(np.asarray(sdf, np.float64) - r.out), fwd_tol(net, r, b0, q)).max())
    free = free_units(r)
    bad = wrong_drop = wrong_scale = 0
    for l, (a, fr) in enumerate(zip(acts, free)):
        a = np.asarray(a)
        alive = r.relu[l] & r.keep[l]
        bad += int((((a > 0) != alive) & ~fr & r.keep[l]).sum())
        wrong_drop += int((a[~r.keep[l]] != 0).sum())
    out["bad_units"] = bad
    out["wrong_drop"] = wrong_drop
    out["free_share"] = float(np.mean(np.concatenate([(f & k).ravel() for f, k in zip(free, r.keep)]))) if free else 0.0
    bm = backward(net, r, g_sdf, deriv=deriv_from_acts(acts, scale), tail=(y1, sdf))
    out["dx"] = float(_ratio(np.abs(np.asarray(g_inputs, np.float64) - bm.g_inputs), q * C["c_dx"] * U32 * bm.M_gin).max())
    out["dw"] = max(float(_ratio(np.abs(np.asarray(w, np.float64) - rw), q * C["c_dw"] * U32 * mw).max()) for w, rw, mw in zip(dW, bm.dW, bm.M_dW))
    out["db"] = max(float(_ratio(np.abs(np.asarray(v, np.float64) - rv), q * C["c_dw"] * U32 * mv).max()) for v, rv, mv in zip(db, bm.db, bm.M_db))
    out["cz"] = max(float((np.abs(np.asarray(a, np.float64) / s - np.where(r.keep[l], np.maximum(r.z[l], 0.0), 0.0)) / (U32 * r.linmass[l])).max())
                    for l, (a, s) in enumerate(zip(acts, scale))) if acts else 0.0
    return out, r, bm


# ---- the weight-norm fold and float64 nets (golden G23, the autograd Function's test) -----------------------------------------------

class Net64:
    """tests/_decoder_ref.Net's attributes with float64 weights (the fold's result is not a float32 value)"""

    def __init__(self, layers, inj, use_tanh=False):
        self.W = [np.asarray(W, np.float64) for W, _ in layers]
        self.b = [np.asarray(b, np.float64) for _, b in layers]
        self.inj = [tuple(int(v) for v in i) for i in inj]
        self.use_tanh = bool(use_tanh)
        self.n_lin = len(layers)
        self.n_inputs = int(self.W[0].shape[1])
        self.out_dims = [int(W.shape[0]) for W in self.W[:-1]]


def fold(v, g):
    """W = v (g / ||v||_row), nn.utils.weight_norm's"""
    v, g = np.asarray(v, np.float64), np.asarray(g, np.float64).reshape(-1, 1)
    return v * (g / np.linalg.norm(v, axis=1, keepdims=True))


def fold_backward(v, g, dW):
    """(dv, dg [out][1]) from dW"""
    v, g = np.asarray(v, np.float64), np.asarray(g, np.float64).reshape(-1, 1)
    nv = np.linalg.norm(v, axis=1, keepdims=True)
    s = (dW * v).sum(1, keepdims=True)
    return dW * (g / nv) - v * (s * g / nv ** 3), s / nv


def clamped_l1(pred, target, clamp=0.1):
    """loss and d loss / d pred of mean |clamp(pred) - clamp(target)|"""
    pred, target = np.asarray(pred, np.float64), np.asarray(target, np.float64)
    diff = np.clip(pred, -clamp, clamp) - np.clip(target, -clamp, clamp)
    inside = (pred > -clamp) & (pred < clamp)
    return float(np.abs(diff).mean()), np.where(inside, np.sign(diff), 0.0) / pred.shape[0]
