"""Float64 restatement of the sphere tracer's kernels (csrc/trace.hip), one function per stage.  TEST INFRASTRUCTURE ONLY: plain numpy, no
device code, written from the kernels' header comments and include/sdfr.h.

Every float the kernels compute is carried here as a pair (v, e): v the float64 value on the float32 inputs, e a first-order bound of what a
float32 evaluation of the same expression may differ from it by.  e is built up operation by operation (class Ap): an operation adds
u |result| (u = eps32 / 2, one rounding) to the errors its operands hand on through the operation's partial derivatives -- the bound
c eps32 mass of the other reference modules with the count c and the mass kept per term by the arithmetic itself, so that the longest
path of a value (ray 6 roundings, slab entry 8, hit point 10, ...) never has to be counted by hand.  An operation whose operands are exact
and whose float64 result is a float32 number adds nothing: such values (a direction component that is exactly 0, an axis-aligned ray of
length exactly 1) must come back BIT FOR BIT.  A fused multiply-add has one rounding where the bound charges two: the bound holds for
either code generation.  Every comparison the kernels branch on is returned with its RATIO = |lhs - rhs| / (e_lhs + e_rhs): a decision with
ratio > 1 cannot fall the other way in float32 (`decided`), the others may legitimately go either way and are exempt from the comparison.

tests/test_trace_refs_cpu.py ties the restatement to the oracle (oracle/sdf_oracle.py) and to torch float64 autograd."""
import numpy as np

F = np.float32
U = 2.0 ** -24
EPS32 = 2.0 * U
FLT_MAX = float(np.finfo(F).max)
T_PAR = float(F(1e-12))          # trace_slab's parallel-ray threshold, as the float32 literal
T_GATE = float(F(0.1))           # trace_polish's grazing gate, as the float32 literal
NV = 20                          # partial sums of the backward: 9 rotation, 3 translation, 8 latent entries


def _rep(v):
    """float64 values that are float32 numbers"""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(v, np.float64).astype(F).astype(np.float64) == v


class Ap:
    """value + first-order float32 error bound, elementwise"""
    __slots__ = ("v", "e")

    def __init__(self, v, e=0.0):
        self.v = np.asarray(v, np.float64)
        self.e = np.asarray(e, np.float64) + np.zeros_like(self.v)

    @staticmethod
    def of(x):
        return x if isinstance(x, Ap) else Ap(x)

    @staticmethod
    def _round(v, carried):
        """the error of a float32 operation with float64 result v whose operands carried `carried`"""
        exact = (carried == 0) & _rep(v)
        with np.errstate(invalid="ignore"):
            return Ap(v, np.where(exact, 0.0, carried + U * np.abs(v)))

    def __add__(self, o):
        o = Ap.of(o)
        return Ap._round(self.v + o.v, self.e + o.e)

    __radd__ = __add__

    def __sub__(self, o):
        o = Ap.of(o)
        return Ap._round(self.v - o.v, self.e + o.e)

    def __rsub__(self, o):
        return Ap.of(o) - self

    def __mul__(self, o):
        o = Ap.of(o)
        with np.errstate(invalid="ignore", over="ignore"):
            return Ap._round(self.v * o.v, np.abs(self.v) * o.e + np.abs(o.v) * self.e)

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = Ap.of(o)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            q = self.v / o.v
            return Ap._round(q, np.where((self.e == 0) & (o.e == 0), 0.0, (self.e + np.abs(q) * o.e) / np.abs(o.v)))

    def __rtruediv__(self, o):
        return Ap.of(o) / self

    def __neg__(self):
        return Ap(-self.v, self.e)

    def __abs__(self):
        return Ap(np.abs(self.v), self.e)

    def sqrt(self):
        with np.errstate(divide="ignore", invalid="ignore"):
            s = np.sqrt(self.v)
            return Ap._round(s, np.where(self.e == 0, 0.0, self.e / (2.0 * s)))

    def __getitem__(self, k):
        return Ap(self.v[k], self.e[k])

    @property
    def tol(self):
        return self.e


def ap_where(c, a, b):
    a, b = Ap.of(a), Ap.of(b)
    return Ap(np.where(c, a.v, b.v), np.where(c, a.e, b.e))


def ap_max(a, b):
    """fmaxf: the error of the operand that wins; of the larger of the two where the intervals overlap"""
    a, b = Ap.of(a), Ap.of(b)
    e = np.where(a.v - a.e > b.v + b.e, a.e, np.where(b.v - b.e > a.v + a.e, b.e, np.maximum(a.e, b.e)))
    return Ap(np.maximum(a.v, b.v), e)


def ap_min(a, b):
    return -ap_max(-Ap.of(a), -Ap.of(b))


def ratio(a, b):
    """how far the comparison of a with b is from its threshold, in units of the two error bounds (inf: exact operands)"""
    a, b = Ap.of(a), Ap.of(b)
    with np.errstate(divide="ignore", invalid="ignore"):
        m, t = np.abs(a.v - b.v), a.e + b.e
        r = np.where(t > 0, m / t, np.inf)
    return np.where(np.isnan(r), np.inf, r)               # NaN operands: the comparison is false in any arithmetic


def unit(got, ref):
    """|got - ref.v| / ref.e elementwise; where the bound is 0 the bits must agree (0 or inf)"""
    got = np.asarray(got, np.float64)
    d = np.abs(got - ref.v)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(ref.e > 0, d / ref.e, np.where(d == 0, 0.0, np.inf))


# ---- rays and the slab test -------------------------------------------------------------------------------------------------------------------

def ray(pose, Kinv, x, y):
    """the pixel ray in object space: r = K^-1 [x, y, 1] (camera frame), d = R^T r, o = -R^T t, |d|.  Returns dict of Ap: r, d, o (lists of 3), dn"""
    P = np.asarray(pose, np.float64).reshape(4, 4)
    Ki = np.asarray(Kinv, np.float64).reshape(3, 3)
    X, Y = Ap(np.asarray(x, np.float64)), Ap(np.asarray(y, np.float64))
    r = [(Ap(Ki[i, 0]) * X + Ap(Ki[i, 1]) * Y) + Ap(Ki[i, 2]) for i in range(3)]
    d = [(Ap(P[0, j]) * r[0] + Ap(P[1, j]) * r[1]) + Ap(P[2, j]) * r[2] for j in range(3)]
    o = [-((Ap(P[0, j]) * Ap(P[0, 3]) + Ap(P[1, j]) * Ap(P[1, 3])) + Ap(P[2, j]) * Ap(P[2, 3])) for j in range(3)]
    o = [Ap(np.broadcast_to(c.v, X.v.shape), np.broadcast_to(c.e, X.v.shape)) for c in o]
    dn = ((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]).sqrt()
    return dict(r=r, d=d, o=o, dn=dn)


def point(rays, lam):
    """o + lam d"""
    lam = Ap.of(lam)
    return [rays["o"][j] + lam * rays["d"][j] for j in range(3)]


def slab(rays, bound, near):
    """entry (>= near) and exit parameter of the rays against the cube [-bound, bound]^3.  An axis the ray runs parallel to (|d_a| < 1e-12)
    only asks whether the origin lies inside the slab.  Returns l0, l1 (Ap), active (bool), ratio (the closest of the ray's decisions)."""
    o, d = rays["o"], rays["d"]
    shape = d[0].v.shape
    b = float(F(bound))
    l0, l1 = Ap(np.full(shape, float(F(near)))), Ap(np.full(shape, FLT_MAX))
    active = np.ones(shape, bool)
    rt = np.full(shape, np.inf)
    for a in range(3):
        par = np.abs(d[a].v) < T_PAR
        rt = np.minimum(rt, ratio(abs(d[a]), T_PAR))
        inside = np.abs(o[a].v) <= b
        active &= np.where(par, inside, True)
        rt = np.where(par, np.minimum(rt, ratio(abs(o[a]), b)), rt)
        ta, tb = (Ap(-b) - o[a]) / d[a], (Ap(b) - o[a]) / d[a]
        l0 = ap_where(par, l0, ap_max(l0, ap_min(ta, tb)))
        l1 = ap_where(par, l1, ap_min(l1, ap_max(ta, tb)))
    with np.errstate(invalid="ignore"):
        active &= l0.v < l1.v
    rt = np.minimum(rt, ratio(l0, l1))
    return l0, l1, active, rt


def pixels(W, H):
    p = np.arange(W * H)
    return (p % W).astype(np.float64), (p // W).astype(np.float64)


def setup_crop(pose, Kinv, W, H, bound, near, cone=None, cone_block=0):
    """sdfr_trace_setup of one crop, every pixel in row-major order: rays, l0 (where the march starts: max(entry, near), or the block's cone
    start if that lies beyond), l1 (`far`), active, ratio.  cone: the crop's float32 cone starts (-1: the block's rays are misses)."""
    x, y = pixels(W, H)
    rays = ray(pose, Kinv, x, y)
    l0, l1, active, rt = slab(rays, bound, near)
    if cone is not None:
        nbx = (W + cone_block - 1) // cone_block
        c = np.asarray(cone, F)[(y.astype(int) // cone_block) * nbx + x.astype(int) // cone_block].astype(np.float64)
        culled = c < 0                                           # (an exact test of an input)
        l0c = ap_max(l0, Ap(c))
        act2 = ~culled & (l0c.v < l1.v)
        rt = np.where(active & ~culled, np.minimum(rt, ratio(l0c, l1)), np.where(culled, np.inf, rt))
        l0 = ap_where(culled, l0, l0c)
        active = active & act2
    return dict(rays=rays, l0=l0, l1=l1, active=active, ratio=rt, x=x, y=y)


# ---- the step rule ----------------------------------------------------------------------------------------------------------------------------

def advance(st, v, dn, eps, far, qmax=1.0):
    """The plain step rule on float32 states st (n, 4) = (lam, rho, q, -) and float32 decoder values v.  Hit: |v| < eps (exact; the state is
    kept).  Otherwise rho' = |v|, q' = clamp(|v| / rho, 0.5, qmax) (1 if rho = 0: one float32 division, bit for bit), lam' = lam + v / |d|;
    miss unless lam' < far and v is a number.  Returns what (1 hit, 0 marching, -1 miss), lam' (Ap), rho', q' (float32), ratio of lam' < far."""
    st = np.asarray(st, F)
    v = np.asarray(v, F)
    r = np.abs(v)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        hit = r < F(eps)
        q = np.where(st[:, 1] > 0, np.minimum(np.maximum(r / st[:, 1], F(0.5)), F(qmax)), F(1)).astype(F)
        # fminf / fmaxf return the other operand for a NaN
        qn = r / st[:, 1]
        q = np.where((st[:, 1] > 0) & np.isnan(qn), F(0.5), q).astype(F)
        l2 = Ap(st[:, 0].astype(np.float64)) + Ap(v.astype(np.float64)) / dn
        far = Ap.of(np.asarray(far, np.float64))
        ok = (l2.v < far.v) & ~np.isnan(v)
    what = np.where(hit, 1, np.where(ok, 0, -1))
    rt = np.where(hit | np.isnan(v), np.inf, ratio(l2, far))
    return what, l2, r, q, rt


# ---- hit list, polish, images, points ---------------------------------------------------------------------------------------------------------

def hits_crop(hit_lam, W, H, PS):
    """which pixels of a crop's slot are hits: hit_lam > 0 (NaN is not) on the crop's own W x H pixels"""
    h = np.zeros(PS, bool)
    with np.errstate(invalid="ignore"):
        h[:W * H] = np.asarray(hit_lam, F)[:W * H] > 0
    return h


def polish(rays, lam0, f0, J, L):
    """One Newton step along the ray, lam_s = lam0 - f0 / (g . d), for rays that are not grazing: |g . d| > 0.1 |g| |d| (g = J[L:L+3]); grazing
    rays keep lam0 and get c = 0 instead of c = 1 / (g . d).  n = g / max(|g|, 1e-12).  Returns dict lam_s, c, n (list), ok, ratio, gd, gnorm."""
    g = [Ap(np.asarray(J, np.float64)[:, L + j]) for j in range(3)]
    d = rays["d"]
    gd = (g[0] * d[0] + g[1] * d[1]) + g[2] * d[2]
    gn = ((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]).sqrt()
    rhs = (Ap(T_GATE) * gn) * rays["dn"]
    ok = np.abs(gd.v) > rhs.v
    rt = ratio(abs(gd), rhs)
    lam0, f0 = Ap(np.asarray(lam0, np.float64)), Ap(np.asarray(f0, np.float64))
    safe = ap_where(ok, gd, Ap(np.ones_like(gd.v)))
    lam_s = ap_where(ok, lam0 - f0 / safe, lam0)
    c = ap_where(ok, Ap(1.0) / safe, Ap(np.zeros_like(gd.v)))
    inv = Ap(1.0) / ap_max(gn, Ap(T_PAR))
    n = [g[j] * inv for j in range(3)]
    return dict(lam_s=lam_s, c=c, n=n, ok=ok, ratio=rt, gd=gd, gnorm=gn, g=g)


def images(pose, rays, pol):
    """depth = lam_s r_z, colour = ((-x, y, z) + 1) / 2 of the polished point, normals = (R n + 1) / 2.  Returns dict of Ap lists."""
    P = np.asarray(pose, np.float64).reshape(4, 4)
    xs = point(rays, pol["lam_s"])
    half = lambda a: (a + Ap(1.0)) / Ap(2.0)
    color = [half(-xs[0]), half(xs[1]), half(xs[2])]
    n = pol["n"]
    normals = [half((Ap(P[i, 0]) * n[0] + Ap(P[i, 1]) * n[1]) + Ap(P[i, 2]) * n[2]) for i in range(3)]
    depth = pol["lam_s"] * rays["r"][2]
    return dict(color=color, normals=normals, depth=depth, xs=xs)


def points_crop(hit, lam_s, rays, ecap):
    """pixel-order compaction of a crop's hits: pt_slot (rank, -1 beyond ecap or no hit), the true count, and xyz = lam_s r of the kept rows"""
    hit = np.asarray(hit, bool)
    rank = np.cumsum(hit) - 1
    slot = np.where(hit & (rank < ecap), rank, -1).astype(np.int32)
    keep = np.nonzero(slot >= 0)[0]
    l = Ap(np.asarray(lam_s, np.float64)[keep])
    xyz = [l * rays["r"][j][keep] for j in range(3)]
    return slot, int(hit.sum()), keep, xyz


# ---- backward ---------------------------------------------------------------------------------------------------------------------------------

def backward_terms(pose, rays, pol, J, L, g_color=None, g_depth=None, g_normals=None, g_pt=None, surfel=False):
    """What every hit pixel adds to d L / d R (entries 0..8, row-major), d L / d t (9..11) and d L / d z (12..12+L), given the upstream gradients
    of its colour (n, 3), depth (n,), normal (n, 3) and camera-frame point (n, 3) (None: absent).

    surfel = False, the image-space derivative at the fixed pixel: the hit parameter is the implicit function
        lam(theta) = lam_s - c [ g . (o(theta) + lam_s d(theta) - x_s) + g_z . (z(theta) - z_s) ],  x = o + lam d,  o = -R^T t,  d = R^T r,
    the camera-frame point lam r moves along its ray only, n_cam = R n with n constant.
    surfel = True: the hit is a material point x_s that moves rigidly with the pose and along its normal with the latent,
        d x_s = -n (g_z . dz) / |g|;  p_cam = R x_s + t, depth = its z, colour = x_s's own coordinates, n_cam = R n.
    Returns a list of NV Ap (entries 12 + L .. are zero)."""
    P = np.asarray(pose, np.float64).reshape(4, 4)
    n_pix = rays["dn"].v.shape
    zero = Ap(np.zeros(n_pix))
    J = np.asarray(J, np.float64)
    gxs = [zero] * 3 if g_color is None else [-(Ap(g_color[:, 0]) / Ap(2.0)), Ap(g_color[:, 1]) / Ap(2.0), Ap(g_color[:, 2]) / Ap(2.0)]
    gnc = [zero] * 3 if g_normals is None else [Ap(g_normals[:, j]) / Ap(2.0) for j in range(3)]
    ge = [zero] * 3 if g_pt is None else [Ap(g_pt[:, j]) for j in range(3)]
    r, d, g, nh, lam_s = rays["r"], rays["d"], pol["g"], pol["n"], pol["lam_s"]
    out = [zero] * NV
    if not surfel:
        gl = ((gxs[0] * d[0] + gxs[1] * d[1]) + gxs[2] * d[2]) + ((ge[0] * r[0] + ge[1] * r[1]) + ge[2] * r[2])
        if g_depth is not None:
            gl = gl + Ap(g_depth) * r[2]
        k = pol["c"] * gl
        gw = [gxs[j] - k * g[j] for j in range(3)]
        gdd = [lam_s * gw[j] for j in range(3)]
        for i in range(3):
            for j in range(3):
                out[i * 3 + j] = (Ap(-P[i, 3]) * gw[j] + r[i] * gdd[j]) + gnc[i] * nh[j]
            out[9 + i] = -((Ap(P[i, 0]) * gw[0] + Ap(P[i, 1]) * gw[1]) + Ap(P[i, 2]) * gw[2])
    else:
        if g_depth is not None:
            ge = [ge[0], ge[1], ge[2] + Ap(g_depth)]
        xs = point(rays, lam_s)
        for i in range(3):
            for j in range(3):
                out[i * 3 + j] = ge[i] * xs[j] + gnc[i] * nh[j]
            out[9 + i] = ge[i]
        go = [((Ap(P[0, j]) * ge[0] + Ap(P[1, j]) * ge[1]) + Ap(P[2, j]) * ge[2]) + gxs[j] for j in range(3)]
        k = ((go[0] * nh[0] + go[1] * nh[1]) + go[2] * nh[2]) / ap_max(pol["gnorm"], Ap(T_PAR))
    for c in range(L):
        out[12 + c] = (-k) * Ap(J[:, c])
    return out


def backward_sum(terms, n_slot):
    """the crop's sums.  The kernels add the pixels' terms in a tree of 8 levels per 256-pixel block, then the block partials: a serial run of
    ceil(blocks / 256) per thread and another tree of 8 levels -- every level one rounding of a partial sum that the sum of the |terms| bounds."""
    nblk = (n_slot + 255) // 256
    depth = 8 + 8 + (nblk + 255) // 256
    tot, err = np.zeros(NV), np.zeros(NV)
    for i, t in enumerate(terms):
        tot[i] = t.v.sum()
        err[i] = t.e.sum() + depth * U * np.abs(t.v).sum()
    return Ap(tot, err)


# ---- one speculative pass -------------------------------------------------------------------------------------------------------------------------

def _and_ratio(conds):
    """ratio of a conjunction [(bool, ratio)]: true -- every term must hold, the closest one counts; false -- one false term suffices, the clearest"""
    truth = np.logical_and.reduce([c for c, _ in conds])
    r_true = np.minimum.reduce([r for _, r in conds])
    r_false = np.maximum.reduce([np.where(c, 0.0, r) for c, r in conds])
    return truth, np.where(truth, r_true, r_false)


def spec_pass(st, rays, far, K, sigma, eps, qmax, value):
    """One pass of K samples per ray from the float32 states st (n, 4) = (lam, rho, q, -): p_0 = lam, p_j = p_{j-1} + sigma q^j rho / |d|;
    sample j counts only while every sample before it was accepted and it lies inside its predecessor's safe sphere,
    (p_j - p_{j-1}) |d| <= |v_{j-1}|, with v_{j-1} > 0 and p_j > p_{j-1}.  The first accepted sample with |v| < eps is the hit (lam = its
    position).  Otherwise the ray goes on from the last accepted sample j*: rho' = |v_j*|, q' = clamp(|v_j*| / (the radius before it), 0.5,
    qmax) (1 when that radius is 0), lam' = p_j* + v_j* / |d|, a miss unless lam' < far.  K = 1 is the plain step rule.
    value(points): the decoder at the points (list of 3 Ap) as an Ap whose bound includes the decoder's own tolerance.
    Returns dict: hit, keep (bool), J (index of the last accepted sample), pj, vj, rho, q, lam (Ap), ratio (the closest decision met)."""
    if isinstance(st, tuple):                                  # (lam, rho, q) as Ap: a state that carries a bound of its own (march below)
        lam, rho, q = st
        st = np.zeros((lam.v.shape[0], 4))
    else:
        st = np.asarray(st, F).astype(np.float64)
        lam, rho, q = Ap(st[:, 0]), Ap(st[:, 1]), Ap(st[:, 2])
    dn = rays["dn"]
    P = [lam]
    qp = q
    for j in range(1, K):
        P.append(P[-1] + ((Ap(float(F(sigma))) * qp) * rho) / dn)
        qp = qp * q
    V = [value(point(rays, p)) for p in P]
    e = float(F(eps))
    vj, rj, pj, prev = V[0], abs(V[0]), P[0], rho
    done = rj.v < e
    ishit = done.copy()
    rt = ratio(rj, e)
    J = np.zeros(st.shape[0], np.int64)
    neg_end = np.zeros(st.shape[0], bool)                      # the prefix ended because the sample before was not outside the surface
    for j in range(1, K):
        rp = abs(V[j - 1])
        gap = (P[j] - P[j - 1]) * dn
        cov, r_cov = _and_ratio([(gap.v <= rp.v, ratio(gap, rp)), (V[j - 1].v > 0, ratio(V[j - 1], 0.0)), (P[j].v > P[j - 1].v, ratio(P[j], P[j - 1]))])
        rt = np.where(done, rt, np.minimum(rt, r_cov))
        neg_end |= ~done & ~cov & (V[j - 1].v <= 0)
        take = cov & ~done
        done = done | ~cov
        prev, vj, rj, pj = ap_where(take, rp, prev), ap_where(take, V[j], vj), ap_where(take, abs(V[j]), rj), ap_where(take, P[j], pj)
        J = np.where(take, j, J)
        hj = take & (np.abs(V[j].v) < e)
        rt = np.where(take, np.minimum(rt, ratio(abs(V[j]), e)), rt)
        ishit |= hj
        done = done | hj
    has_prev = prev.v > 0
    qn = ap_where(has_prev, ap_min(ap_max(rj / ap_where(has_prev, prev, Ap(np.ones_like(prev.v))), Ap(0.5)), Ap(float(F(qmax)))), Ap(np.ones_like(prev.v)))
    l2 = pj + vj / dn
    far = Ap.of(np.asarray(far, np.float64))
    keep = ~ishit & (l2.v < far.v)
    rt = np.where(ishit, rt, np.minimum(rt, np.minimum(ratio(l2, far), ratio(prev, 0.0))))
    return dict(hit=ishit, keep=keep, J=J, pj=pj, vj=vj, rho=rj, q=qn, lam=l2, ratio=rt, neg_end=neg_end)


# ---- the cone phase -------------------------------------------------------------------------------------------------------------------------------

def cone_setup(pose, Kinv, W, H, block, bound, near):
    """One cone per block x block pixel tile (clipped by the image border): the ray through the centre of the tile's pixels, delta = the largest
    |d_corner - d_centre| over its four corner pixels, near_b / far_b = the smallest entry / the largest exit over its pixel rays that enter
    the cube (keep: any does), first advance guess a0 = 0.1 (far_b - near_b).  ratio: the closest slab decision of any of the tile's pixels."""
    nbx, nby = (W + block - 1) // block, (H + block - 1) // block
    k = np.arange(nbx * nby)
    x0, y0 = (k % nbx) * block, (k // nbx) * block
    x1, y1 = np.minimum(x0 + block - 1, W - 1), np.minimum(y0 + block - 1, H - 1)
    rc = ray(pose, Kinv, 0.5 * (x0 + x1), 0.5 * (y0 + y1))
    delta = Ap(np.zeros(k.size))
    for cx, cy in ((x0, y0), (x1, y0), (x0, y1), (x1, y1)):
        rk = ray(pose, Kinv, cx.astype(np.float64), cy.astype(np.float64))
        e = [rk["d"][j] - rc["d"][j] for j in range(3)]
        delta = ap_max(delta, ((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]).sqrt())
    near_b, far_b = Ap(np.full(k.size, FLT_MAX)), Ap(np.zeros(k.size))
    keep = np.zeros(k.size, bool)
    rt = np.full(k.size, np.inf)
    for j in range(block):
        for i in range(block):
            px, py = x0 + i, y0 + j
            ins = (px <= x1) & (py <= y1)
            rk = ray(pose, Kinv, px.astype(np.float64), py.astype(np.float64))
            l0, l1, act, r = slab(rk, bound, near)
            a = act & ins
            near_b, far_b = ap_where(a, ap_min(near_b, l0), near_b), ap_where(a, ap_max(far_b, l1), far_b)
            keep |= a
            rt = np.where(ins, np.minimum(rt, r), rt)
    a0 = Ap(float(F(0.1))) * (far_b - near_b)
    return dict(rays=rc, delta=delta, near=near_b, far=far_b, keep=keep, a0=a0, ratio=rt, x0=x0, y0=y0, x1=x1, y1=y1)


def cone_pass(cs, K, sigma, eps, bound, value):
    """The first (and, with cone_steps = 1, last) pass of K samples of the kept cones: p_0 = near_b, p_j = p_{j-1} + sigma q^j a_prev (q = 1,
    a_prev = a0).  A sample counts only inside the range its predecessor proved free, p_{j-1} < p_j <= p_{j-1} + a_{j-1}.  v = the decoder at
    the centre point CLAMPED into the cube, and sqrt(cd^2 + max(v, 0)^2) where the point lies outside it by cd > 0.  free = v - p delta:
    free <= eps -> the tile's rays start at p (kind 0); else a = free / (|d_c| + delta) and p + a >= far_b -> culled, -1 (kind 1); else the cone
    advances to p + a.  Cones still marching at the end of the pass start where they got to (kind 2).
    Returns start (Ap), kind, ratio -- over the kept cones of cs (index arrays follow cs['keep'])."""
    sel = np.nonzero(cs["keep"])[0]
    rays = dict(o=[c[sel] for c in cs["rays"]["o"]], d=[c[sel] for c in cs["rays"]["d"]])
    delta, far_b, aprev = cs["delta"][sel], cs["far"][sel], cs["a0"][sel]
    den = cs["rays"]["dn"][sel] + delta
    n = sel.size
    b = float(F(bound))
    P = [cs["near"][sel]]
    qp = Ap(np.ones(n))
    for j in range(1, K):
        P.append(P[-1] + (Ap(float(F(sigma))) * qp) * aprev)
        qp = qp * Ap(np.ones(n))
    out, kind = Ap(np.full(n, np.nan)), np.full(n, -1)
    done = np.zeros(n, bool)
    rt = cs["ratio"][sel].copy()
    lam_new, a_prevj = P[0], aprev
    e = float(F(eps))
    clamped = np.zeros(n, bool)                                # a counted sample lay outside the cube
    for j in range(K):
        if j > 0:
            gap = P[j] - P[j - 1]
            valid, r_v = _and_ratio([(P[j].v > P[j - 1].v, ratio(P[j], P[j - 1])), (gap.v <= a_prevj.v, ratio(gap, a_prevj))])
            rt = np.where(done, rt, np.minimum(rt, r_v))
            done = done | ~valid                                   # the prediction left the proved range: the pass ends at the previous sample
        x = point(rays, P[j])
        cl, ex = [], []
        r_cl = np.full(n, np.inf)
        for a in range(3):
            outside = np.abs(x[a].v) > b
            r_cl = np.minimum(r_cl, ratio(abs(x[a]), b))
            edge = np.where(x[a].v > 0, b, -b)
            cl.append(ap_where(outside, Ap(edge), x[a]))
            ex.append(ap_where(outside, x[a] - Ap(edge), Ap(np.zeros(n))))   # inside the cube x - clamp(x) is exactly 0
        cd = ((ex[0] * ex[0] + ex[1] * ex[1]) + ex[2] * ex[2]).sqrt()
        v = value(cl)
        vp = ap_max(v, Ap(0.0))
        v = ap_where(cd.v > 0, ((cd * cd) + (vp * vp)).sqrt(), v)
        free = v - P[j] * delta
        act = ~done
        clamped |= act & (cd.v > 0)
        go = free.v > e
        rt = np.where(act, np.minimum(rt, np.minimum(ratio(free, e), r_cl)), rt)
        stop = act & ~go
        a_ = free / den
        adv = P[j] + a_
        cul = act & go & ~(adv.v < far_b.v)
        rt = np.where(act & go, np.minimum(rt, ratio(adv, far_b)), rt)
        ok = act & go & ~cul
        out = ap_where(stop, P[j], ap_where(cul, Ap(np.full(n, -1.0)), out))
        kind = np.where(stop, 0, np.where(cul, 1, kind))
        lam_new, a_prevj = ap_where(ok, adv, lam_new), ap_where(ok, a_, a_prevj)
        done = done | stop | cul
    alive = kind < 0
    out = ap_where(alive, lam_new, out)
    kind = np.where(alive, 2, kind)
    return dict(sel=sel, start=out, kind=kind, ratio=rt, clamped=clamped)


# ---- a whole march ----------------------------------------------------------------------------------------------------------------------------------

def pass_samples(levels, s):
    """samples per ray of the pass with index s: the schedule [(first pass index, samples)], a function of s alone; 1 before the first level"""
    k = 1
    for a, b in levels:
        if s >= a:
            k = int(b)
    return k


def march(l0, rays, far, steps, levels, sigma, eps, qmax, value_of, c_acc):
    """`steps` passes from the set-up state (l0, 0, 1), pass s with pass_samples(levels, s) samples per ray (spec_pass; 1 sample: the plain step
    rule).  Rays that still march when the passes run out are unresolved.
    The bound of lam is ACCUMULATED, not propagated: with a decoder of slope <= 1 a step does not amplify an error of lam
    (|1 + f'(x) . d / |d|| <= 1), so the errors of the passes add.  Every pass is run twice: from the state taken as exact, which gives the pass's
    own one-step bound e_s of lam', and from the state carrying c_acc * (e_0 + ... + e_{s-1}), which gives the pass's decisions their ratios and
    rho', q' their bounds.  c_acc is calibrated on a float32 emulation of the whole march (tests/test_trace_refs_cpu.py).
    value_of(idx): the `value` callback of spec_pass for the rays idx.
    Returns dict: hit, unresolved (bool), hit_lam (Ap, bound c_acc * acc), acc (the sum of one-step bounds behind hit_lam, or behind the last
    lam of a ray that did not hit), ratio (the closest decision over all passes), evals, max_evals (what one ray can cost)."""
    l0 = Ap.of(l0)
    n = l0.v.shape[0]
    lam, acc = l0.v.copy(), l0.e.copy()
    rho, q = Ap(np.zeros(n)), Ap(np.ones(n))
    active = np.ones(n, bool)
    hit = np.zeros(n, bool)
    hit_v, hit_acc = np.zeros(n), np.zeros(n)
    rt = np.full(n, np.inf)
    evals = max_evals = 0
    far = np.asarray(far, np.float64)
    for s in range(steps):
        idx = np.nonzero(active)[0]
        k = pass_samples(levels, s)
        max_evals += k
        if idx.size == 0:
            continue
        evals += idx.size * k
        sub = dict(o=[c[idx] for c in rays["o"]], d=[c[idx] for c in rays["d"]], dn=rays["dn"][idx])
        val = value_of(idx)
        own = spec_pass((Ap(lam[idx]), Ap(rho.v[idx]), Ap(q.v[idx])), sub, far[idx], k, sigma, eps, qmax, val)
        res = spec_pass((Ap(lam[idx], c_acc * acc[idx]), rho[idx], q[idx]), sub, far[idx], k, sigma, eps, qmax, val)
        rt[idx] = np.minimum(rt[idx], res["ratio"])
        h = res["hit"]
        hit[idx[h]] = True
        hit_v[idx[h]] = res["pj"].v[h]
        hit_acc[idx[h]] = acc[idx[h]] + own["pj"].e[h]
        keep = res["keep"]
        lam[idx] = np.where(keep, res["lam"].v, lam[idx])
        acc[idx] = acc[idx] + np.where(np.isfinite(own["lam"].e), own["lam"].e, 0.0)
        rho.v[idx], rho.e[idx] = res["rho"].v, res["rho"].e
        q.v[idx], q.e[idx] = res["q"].v, res["q"].e
        active[idx] = keep
    acc_out = np.where(hit, hit_acc, acc)
    return dict(hit=hit, unresolved=active.copy(), hit_lam=Ap(hit_v, c_acc * hit_acc), acc=acc_out, ratio=rt, evals=evals, max_evals=max_evals)
