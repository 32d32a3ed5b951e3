"""Float64 numpy restatement of the CSS head's training losses and their gradients (pipelines/train_css.py:71-80 of the reference) with the
tolerance a float32 implementation is held to.  With N = B H W, m = (mask_gt != 0), t_h = uvw_gt[:, h] m and z_h = W_h x_h + b_h:

  colour heads  log_softmax is idempotent and log_softmax(z) * m is all zeros where m = 0, so
                  loss_h = (1/N) [ sum_{m=1} (logsumexp(z_h) - z_h[t_h]) + (N - n_fg) ln 256 ],  g_h = dloss_h/dz_h = m (softmax(z_h) - onehot(t_h)) / N
  mask head     loss_mask = 2 CE(z_mask, m),  g_mask = 2 (softmax(z_mask) - onehot(m)) / N
  latent        loss = mean over B * 3 of (lat - gt)^2, lat = v f, f = 1 / (|v| + 1e-8), v = W_lat mean_p(x4) + b_lat; the reference DETACHES
                the length (project_vecs_onto_sphere), so dv = 2 (lat - gt) / (3 B) f with no term through the norm
  dX = W^T g per pixel, dW = sum_pix g (x) x, db = sum_pix g

Tolerances, derived from the arithmetic and never from an implementation (delta is _css_ref's per-pixel bound on a logit):
  g        log p_c = z_c - lse moves by at most 2 delta (the logit and the log-sum-exp, a weighted mean of logits): a softmax entry moves by
           2 delta p, plus 2^-21 p for exp and the sum; the subtraction of the one-hot and the product with 1/N (itself rounded) add three
           roundings of the result:                                dg = m s (2 delta + 2^-21) p / N + 3 * 2^-24 |g|      (s = 2 for the mask head)
           float32 has no numbers between 0 and 2^-149 and expf may return 0 below 2^-126: every g carries TINY = 2^-126 more (absolute), and
           so does every float32 result (|W| TINY per class in dX, |x| TINY per pixel in dW)
  dX       sum_c |W| dg + (256 + 2) * 2^-24 * sum_c |W| |g|  (2 + 2 classes for the mask head); exactly 0 where m = 0 for the colour heads
  dW, db   sum_pix dg |x| + (N + 2) * 2^-24 * sum_pix |g| |x|: the any-order bound over N pixels (|x| = 1 for db)
  losses   a pixel's term lse - z[t] moves by 2 delta, plus 2^-22 (|lse| + |z[t]|) for exp, log and the float32 roundings of the two; the mean
           over N terms in any order adds (N + 2) * 2^-24 * mean |term|
  latent   tl = _css_ref.latent's bound on |lat|'s error (it covers v's rounding relative to |v|, hence also f's relative error);
           loss: mean(2 |lat - gt| tl + tl^2) + 8 * 2^-24 loss
           dv:   tdv = 2 / (3 B) f tl (1 + |lat - gt|) + 2^-22 |dv|
           dx4 = W^T dv / (h w):  (sum_j |W_jc| tdv_j + 5 * 2^-24 sum_j |W_jc| |dv_j|) / (h w)
           dW  = sum_b dv_b (x) xbar_b:  sum_b (tdv |xbar| + |dv| (h w + 1) 2^-24 mean_p |x|) + (B + 2) 2^-24 sum_b |dv| |xbar|
           db  = sum_b dv_b:  sum_b tdv + (B + 2) 2^-24 sum_b |dv|
"""
import numpy as np

from tests import _css_ref as R

U24 = R.U24
HEADS = ("u", "v", "w", "mask")
LN256 = float(np.log(256.0))
TINY = 2.0 ** -126


def _one_head(x, w, b, target, m, n_class, scale):
    """target int [B][H][W], m float [B][H][W] weight of the pixel's gradient (0 / 1); returns values and tolerances of loss, dx, dw, db"""
    x = R._f64(x)
    w2 = R._w2(w)
    lg, d = R._logits(x, w, b)
    B, _, H, W = x.shape
    N = B * H * W
    zmax = lg.max(axis=1, keepdims=True)
    lse = zmax + np.log(np.exp(lg - zmax).sum(axis=1, keepdims=True))
    p = np.exp(lg - lse)
    oh = (np.arange(n_class)[None, :, None, None] == target[:, None]).astype(np.float64)
    mm = m[:, None].astype(np.float64)
    g = scale * mm * (p - oh) / N
    dg = scale * mm * (2 * d + 2.0 ** -21) * p / N + 3 * U24 * np.abs(g) + mm * TINY
    zt = (lg * oh).sum(axis=1, keepdims=True)
    term = mm * (lse - zt) + (1 - mm) * np.log(float(n_class))
    tterm = mm * (2 * d + 2.0 ** -22 * (np.abs(lse) + np.abs(zt)))
    out = {"loss": scale * term.sum() / N, "dx": np.einsum("ck,bchw->bkhw", w2, g), "dw": np.einsum("bchw,bkhw->ck", g, x), "db": g.sum(axis=(0, 2, 3))}
    aw, ax, ag = np.abs(w2), np.abs(x), np.abs(g)
    tol = {"loss": scale * (tterm.sum() / N + (N + 2) * U24 * np.abs(term).sum() / N),
           "dx": np.einsum("ck,bchw->bkhw", aw, dg) + (n_class + 2) * U24 * np.einsum("ck,bchw->bkhw", aw, ag) + mm * TINY,
           "dw": np.einsum("bchw,bkhw->ck", dg, ax) + (N + 2) * U24 * np.einsum("bchw,bkhw->ck", ag, ax) + TINY,
           "db": dg.sum(axis=(0, 2, 3)) + (N + 2) * U24 * ag.sum(axis=(0, 2, 3)) + TINY}
    return out, tol


def head_loss(x_u, x_v, x_w, x_mask, weights, uvw_gt, mask_gt):
    """Returns (out, tol): {'loss_u', 'dx_u', 'dw_u', 'db_u', ... for u, v, w, mask} in float64 and a tolerance of the same shape per key."""
    m = (np.asarray(mask_gt) != 0)
    uvw = np.asarray(uvw_gt).astype(np.int64)
    out, tol = {}, {}
    for i, (h, x) in enumerate((("u", x_u), ("v", x_v), ("w", x_w))):
        o, t = _one_head(x, *weights[h], uvw[:, i] * m, m.astype(np.float64), 256, 1.0)
        for k in o:
            out[k + "_" + h], tol[k + "_" + h] = o[k], t[k]
    o, t = _one_head(x_mask, *weights["mask"], m.astype(np.int64), np.ones(m.shape), 2, 2.0)
    for k in o:
        out[k + "_mask"], tol[k + "_mask"] = o[k], t[k]
    return out, tol


def latent_loss(x4, w, b, latent_gt):
    """(out, tol) with keys 'loss_lat', 'dx_lat' [B][256][h][w], 'dw_lat' [3][256], 'db_lat' [3]"""
    x, w2, b, gt = R._f64(x4), R._w2(w), R._f64(b), R._f64(latent_gt)
    B, C, h, wd = x.shape
    hw = h * wd
    lat, tl = R.latent(x4, w, b)                                      # [B][3], [B][1]
    xbar = x.reshape(B, C, hw).mean(axis=2)
    axbar = np.abs(x).reshape(B, C, hw).mean(axis=2)
    v = xbar @ w2.T + b[None]
    f = 1.0 / (np.linalg.norm(v, axis=1, keepdims=True) + 1e-8)
    d = lat - gt
    loss = (d * d).mean()
    dv = 2 * d / (3 * B) * f
    tdv = 2 / (3 * B) * f * tl * (1 + np.abs(d)) + 2.0 ** -22 * np.abs(dv)
    out = {"loss_lat": loss, "dx_lat": np.broadcast_to(((dv @ w2) / hw)[:, :, None, None], x.shape).copy(), "dw_lat": dv.T @ xbar,
           "db_lat": dv.sum(axis=0)}
    aw, adv = np.abs(w2), np.abs(dv)
    tol = {"loss_lat": (2 * np.abs(d) * tl + tl * tl).mean() + 8 * U24 * loss,
           "dx_lat": np.broadcast_to(((tdv @ aw + 5 * U24 * (adv @ aw)) / hw)[:, :, None, None], x.shape).copy(),
           "dw_lat": tdv.T @ np.abs(xbar) + adv.T @ ((hw + 1) * U24 * axbar) + (B + 2) * U24 * (adv.T @ np.abs(xbar)),
           "db_lat": tdv.sum(axis=0) + (B + 2) * U24 * adv.sum(axis=0)}
    return out, tol


def compare(got, out, tol, keys=None, label=""):
    """Print and assert every key of `got` against the restatement; returns {key: (max error, largest error / tolerance)}."""
    res = {}
    for key in (keys or sorted(got)):
        g = np.asarray(got[key], dtype=np.float64).reshape(np.shape(out[key]))
        assert np.isfinite(g).all(), key
        err = np.abs(g - out[key])
        t = np.broadcast_to(tol[key], err.shape)
        bad = (t == 0) & (err > 0)
        ratio = float(np.where(t > 0, err / np.where(t > 0, t, 1.0), 0.0).max()) if err.size else 0.0
        if bad.any():
            ratio = float("inf")
        res[key] = (float(err.max()) if err.size else 0.0, ratio)
        print("%s %-10s max error %.3e, largest error / tolerance %.3f (largest value %.3e)" % (label, key, res[key][0], ratio,
                                                                                                 float(np.abs(out[key]).max()) if err.size else 0.0))
    for key, (_, ratio) in res.items():
        assert ratio <= 1.0, (key, ratio)
    return res
