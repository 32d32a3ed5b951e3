"""Float64 numpy restatement of the CSS network's output head and latent head (networks/resnet_css.py:194-196, :203-249 of the reference),
with the tolerance a float32 implementation is held to.  The tolerances are derived from the arithmetic, not from any implementation:

  delta      bound on a logit's rounding error: a 64-term dot product plus the bias, (64 + 2) * 2^-24 * max_k(sum_j |w_kj| |x_j| + |b_k|)
             per pixel (the usual n u sum |terms| bound, taken over the classes so one number serves a pixel).
  uvw_sm     E = sum_k k p_k with p = softmax(100 logit).  dE/dlogit_k = 100 p_k (k - E), so to first order |dE| <= 100 delta S with
             S = sum_k p_k |k - E|; the factor 2 covers the second order while 100 delta << 1.  255 * 2^-22 (four ulp of the largest
             colour) covers exp, the sums and the division.                    tol = 2 * 100 * delta * S + 255 * 2^-22
  mask       the raw logits: delta_mask.
  mask_sm    p = softmax(100 mask)[1], dp/d(m1 - m0) = 100 p (1 - p), each logit off by delta_mask:
                                                                                tol = 2 * 100 * delta_mask * p (1 - p) + 2^-22
  u, v, w    log_softmax moves by at most 2 delta (the logit and the log-sum-exp, a weighted mean of logits), plus 2^-20 relative for exp,
             log and the sum.                                                   tol = 2 * delta + 2^-20 * |value|
  masked     uvw_sm * (m1 > m0): the comparison can flip where |m1 - m0| <= 2 delta_mask; those pixels are left out (`unsure`), and a
             case may leave out at most 0.5 % of its pixels.  Elsewhere the tolerance is uvw_sm's.
  latent     v_c = mean_p(sum_k w_ck x_kp + b_c): 256 + 2 terms per pixel and h w pixels, delta_lat_c = (258 + h w) * 2^-24 *
             mean_p(sum_k |w_ck| |x_kp| + |b_c|); the unit vector v / |v| moves by at most |delta_lat| / |v|, doubled for the second
             order, plus 2^-22 for the norm and the division.                   tol = 2 |delta_lat| / |v| + 2^-22
"""
import numpy as np

U24 = 2.0 ** -24
HARD = 100.0
MAX_UNSURE = 0.005


def _f64(a):
    return np.asarray(a, dtype=np.float64)


def _w2(w):
    w = _f64(w)
    return w.reshape(w.shape[0], w.shape[1])


def _logits(x, w, b):
    """1x1 convolution in float64 and its rounding bound: ([B][K][H][W], [B][1][H][W])"""
    x, w, b = _f64(x), _w2(w), _f64(b)
    lg = np.einsum('kc,bchw->bkhw', w, x) + b[None, :, None, None]
    mag = np.einsum('kc,bchw->bkhw', np.abs(w), np.abs(x)) + np.abs(b)[None, :, None, None]
    return lg, (w.shape[1] + 2) * U24 * mag.max(axis=1, keepdims=True)


def _softmax(z):
    z = z - z.max(axis=1, keepdims=True)
    e = np.exp(z)
    return e / e.sum(axis=1, keepdims=True)


def head(x_u, x_v, x_w, x_mask, weights):
    """weights: {'u': (W, b), 'v': ..., 'w': ..., 'mask': ...}.  Returns (out, tol, unsure): float64 outputs under the reference's keys, a
    tolerance array per key (broadcastable to the output) and the bool [B][1][H][W] map of pixels left out of the uvw_sm_masked comparison."""
    out, tol = {}, {}
    cols, tols = [], []
    k = np.arange(256, dtype=np.float64)[None, :, None, None]
    for name, x in (('u', x_u), ('v', x_v), ('w', x_w)):
        lg, d = _logits(x, *weights[name])
        p = _softmax(HARD * lg)
        E = (k * p).sum(axis=1, keepdims=True)
        S = (p * np.abs(k - E)).sum(axis=1, keepdims=True)
        cols.append(E)
        tols.append(2 * HARD * d * S + 255 * 2.0 ** -22)
        z = lg - lg.max(axis=1, keepdims=True)
        out[name] = z - np.log(np.exp(z).sum(axis=1, keepdims=True))
        tol[name] = 2 * d + 2.0 ** -20 * np.abs(out[name])
    out['uvw_sm'], tol['uvw_sm'] = np.concatenate(cols, axis=1), np.concatenate(tols, axis=1)
    m, dm = _logits(x_mask, *weights['mask'])
    out['mask'], tol['mask'] = m, np.broadcast_to(dm, m.shape)
    p1 = _softmax(HARD * m)[:, 1:2]
    out['mask_sm'], tol['mask_sm'] = p1, 2 * HARD * dm * p1 * (1 - p1) + 2.0 ** -22
    gap = m[:, 1:2] - m[:, 0:1]
    out['uvw_sm_masked'], tol['uvw_sm_masked'] = out['uvw_sm'] * (gap > 0), tol['uvw_sm']
    unsure = np.abs(gap) <= 2 * dm
    return out, tol, unsure


def latent(x4, w, b):
    """(latent [B][3] float64, tol [B][1])"""
    x, w, b = _f64(x4), _w2(w), _f64(b)
    hw = x.shape[2] * x.shape[3]
    v = np.einsum('kc,bchw->bkhw', w, x).reshape(x.shape[0], 3, hw).mean(axis=2) + b[None]
    mag = np.einsum('kc,bchw->bkhw', np.abs(w), np.abs(x)).reshape(x.shape[0], 3, hw).mean(axis=2) + np.abs(b)[None]
    d = (w.shape[1] + 2 + hw) * U24 * mag
    n = np.linalg.norm(v, axis=1, keepdims=True)
    return v * (1.0 / (n + 1e-8)), 2 * np.linalg.norm(d, axis=1, keepdims=True) / n + 2.0 ** -22


def compare(got, out, tol, unsure, keys=None, label=""):
    """Print and assert every key of `got` (numpy arrays) against the restatement; returns {key: (max error, max error / tolerance)}."""
    res = {}
    share = float(unsure.mean())
    print("%s pixels left out of uvw_sm_masked: %d of %d (%.3f %%)" % (label, int(unsure.sum()), unsure.size, 100 * share))
    for key in (keys or sorted(got)):
        g = np.asarray(got[key], dtype=np.float64)
        assert g.shape == out[key].shape, (key, g.shape, out[key].shape)
        assert np.isfinite(g).all(), key
        err = np.abs(g - out[key])
        t = np.broadcast_to(tol[key], err.shape)
        if key == 'uvw_sm_masked':
            keep = np.broadcast_to(~unsure, err.shape)
            err, t = err[keep], t[keep]
        ratio = float((err / t).max()) if err.size else 0.0
        res[key] = (float(err.max()) if err.size else 0.0, ratio)
        print("%s %-14s max error %.3e, largest error / tolerance %.3f (smallest tolerance %.3e)" % (label, key, res[key][0], ratio,
                                                                                                  float(t.min()) if t.size else 0.0))
    assert share <= MAX_UNSURE, "too many pixels with an undecided mask: %.3f %%" % (100 * share)
    for key, (_, ratio) in res.items():
        assert ratio <= 1.0, (key, ratio)
    return res
