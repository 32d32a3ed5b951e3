"""Numpy restatements of what Pillow 12 computes for the calls torchvision's PIL backend makes in the reference's datasets/crops.py, for the
tests of csrc/augment.hip.  All images are uint8 [h][w][3] arrays.

  brightness, contrast, saturation   ImageEnhance.* = Image.blend(degenerate, image, f): float32 a + f (b - a), truncated / clipped
  rgb_to_hsv, hsv_to_rgb, hue        Image.convert('HSV') / convert('RGB') around H += uint8(hue * 255)
  jitter                             the four in a given order
  rotation_matrix                    the host arithmetic of Image.rotate(angle, expand=True)
  rotate_bilinear, rotate_nearest    Image.transform(AFFINE): the generic float64 bilinear path, the 16.16 fixed-point nearest path
  resize_bilinear, resize_nearest    ImagingResample (two 8-bit passes, 22-bit coefficients) and ImagingScaleAffine
  augment                            the whole chain of one sample: jitter, rotate, resize, crop, resize; labels and mask

Nothing here imports the product: the CPU tests pin these functions to PIL itself and to golden G22, the GPU tests pin the kernels to them.
"""
import math

import numpy as np

OUT = 128
MEAN = np.array([0.485, 0.456, 0.406], np.float32)
STD = np.array([0.229, 0.224, 0.225], np.float32)
PRECISION_BITS = 22
OPS = ("brightness", "contrast", "saturation", "hue")


# ---- colour -------------------------------------------------------------------------------------------------------------------------------
def luma(img):
    """convert('L'): (19595 R + 38470 G + 7471 B + 0x8000) >> 16"""
    i = img.astype(np.int64)
    return ((19595 * i[..., 0] + 38470 * i[..., 1] + 7471 * i[..., 2] + 0x8000) >> 16).astype(np.uint8)


def blend(a, b, f):
    """Image.blend(a, b, f) of two uint8 arrays: t = a + f (b - a) in float32"""
    f = np.float32(f)
    af = a.astype(np.float32)
    t = af + f * (b.astype(np.float32) - af)
    if 0.0 <= f <= 1.0:
        return t.astype(np.int32).astype(np.uint8)
    return np.where(t <= 0, 0, np.where(t >= 255, 255, t.astype(np.int32))).astype(np.uint8)


def brightness(img, f):
    return blend(np.zeros_like(img), img, f)


def contrast(img, f):
    L = luma(img)
    s, n = int(L.astype(np.int64).sum()), L.size
    mean = (2 * s + n) // (2 * n)                       # int(sum / n + 0.5)
    return blend(np.full_like(img, mean), img, f)


def saturation(img, f):
    return blend(np.repeat(luma(img)[..., None], 3, -1), img, f)


def rgb_to_hsv(img):
    """convert('HSV'): float32 quotients, the hue sextant and h / 6 + 1 in float64 from a float32 h, truncation"""
    r, g, b = (img[..., k].astype(np.int32) for k in range(3))
    maxc, minc = np.maximum(r, np.maximum(g, b)), np.minimum(r, np.minimum(g, b))
    grey = maxc == minc
    with np.errstate(all="ignore"):
        cr = (maxc - minc).astype(np.float32)
        s = cr / maxc.astype(np.float32)
        rc, gc, bc = ((maxc - c).astype(np.float32) / cr for c in (r, g, b))
        h = np.where(r == maxc, (bc - gc).astype(np.float64),
                     np.where(g == maxc, 2.0 + rc.astype(np.float64) - bc.astype(np.float64),
                              4.0 + gc.astype(np.float64) - rc.astype(np.float64))).astype(np.float32)
        h = np.fmod(h.astype(np.float64) / 6.0 + 1.0, 1.0).astype(np.float32)
        uh = np.clip((h.astype(np.float64) * 255.0).astype(np.int32), 0, 255)
        us = np.clip((s.astype(np.float64) * 255.0).astype(np.int32), 0, 255)
    uh, us = np.where(grey, 0, uh), np.where(grey, 0, us)
    return np.stack((uh, us, maxc), -1).astype(np.uint8)


def hsv_to_rgb(hsv):
    """convert('RGB') of an HSV image: float32 h * 6 / 255 split into sextant and remainder, p / q / t rounded half up from float64"""
    h, s, v = (hsv[..., k].astype(np.int32) for k in range(3))
    hf = h.astype(np.float32).astype(np.float64) * 6.0 / 255.0
    i = np.floor(hf).astype(np.int32)
    f = (hf - i.astype(np.float32).astype(np.float64)).astype(np.float32).astype(np.float64)
    fs = (s.astype(np.float64) / 255.0).astype(np.float32).astype(np.float64)
    vf = v.astype(np.float64)

    def rnd(x):
        return np.clip(np.floor(x + 0.5).astype(np.int32), 0, 255)
    p, q, t = rnd(vf * (1.0 - fs)), rnd(vf * (1.0 - fs * f)), rnd(vf * (1.0 - fs * (1.0 - f)))
    k = i % 6
    r = np.choose(k, (v, q, p, p, t, v))
    g = np.choose(k, (t, v, v, q, p, p))
    b = np.choose(k, (p, p, t, v, v, q))
    grey = s == 0
    return np.stack((np.where(grey, v, r), np.where(grey, v, g), np.where(grey, v, b)), -1).astype(np.uint8)


def hue_shift(f):
    """np.array(f * 255).astype(np.uint8): truncation toward zero, then the byte"""
    return int(f * 255) & 255


def hue(img, f):
    if f == 0:
        return img.copy()
    hsv = rgb_to_hsv(img)
    hsv[..., 0] = (hsv[..., 0].astype(np.int32) + hue_shift(f)) & 255
    return hsv_to_rgb(hsv)


def jitter(img, factors, order):
    """factors: (brightness, contrast, saturation, hue); order: a permutation of 0 ... 3, the operations in the order applied"""
    fn = (brightness, contrast, saturation, hue)
    for k in order:
        img = fn[int(k)](img, factors[int(k)])
    return img


# ---- rotation -----------------------------------------------------------------------------------------------------------------------------
def rotation_matrix(w, h, angle):
    """Image.rotate(angle, expand=True): (matrix of 6 float64, nw, nh), or (None, w, h) for the copy shortcut"""
    angle = angle % 360.0
    if angle == 0:
        return None, w, h
    if angle in (90, 180, 270):
        raise ValueError("rotation by %g degrees is Pillow's transpose shortcut, which is not restated" % angle)
    a = -math.radians(angle)
    m = [round(math.cos(a), 15), round(math.sin(a), 15), 0.0, round(-math.sin(a), 15), round(math.cos(a), 15), 0.0]

    def tf(x, y):
        return m[0] * x + m[1] * y + m[2], m[3] * x + m[4] * y + m[5]
    cx, cy = w / 2, h / 2
    m[2], m[5] = tf(-cx - 0, -cy - 0)
    m[2] += cx
    m[5] += cy
    xs, ys = zip(*(tf(x, y) for x, y in ((0, 0), (w, 0), (w, h), (0, h))))
    nw = math.ceil(max(xs)) - math.floor(min(xs))
    nh = math.ceil(max(ys)) - math.floor(min(ys))
    m[2], m[5] = tf(-(nw - w) / 2.0, -(nh - h) / 2.0)
    return m, nw, nh


def rotate_bilinear(img, angle):
    m, nw, nh = rotation_matrix(img.shape[1], img.shape[0], angle)
    if m is None:
        return img.copy()
    h, w = img.shape[:2]
    xi, yi = np.arange(nw, dtype=np.float64)[None, :] + 0.5, np.arange(nh, dtype=np.float64)[:, None] + 0.5
    xin = m[0] * xi + m[1] * yi + m[2]
    yin = m[3] * xi + m[4] * yi + m[5]
    inside = (xin >= 0.0) & (xin < w) & (yin >= 0.0) & (yin < h)
    xs, ys = xin - 0.5, yin - 0.5
    x, y = np.floor(xs).astype(np.int64), np.floor(ys).astype(np.int64)       # FLOOR: floor below zero, truncation above
    dx, dy = (xs - x)[..., None], (ys - y)[..., None]
    x0, x1 = np.clip(x, 0, w - 1), np.clip(x + 1, 0, w - 1)
    src = img.astype(np.float64)
    yc = np.clip(y, 0, h - 1)
    a, b = src[yc, x0], src[yc, x1]
    v1 = a + (b - a) * dx
    lower = (y + 1 >= 0) & (y + 1 < h)
    y1 = np.clip(y + 1, 0, h - 1)
    a, b = src[y1, x0], src[y1, x1]
    v2 = np.where(lower[..., None], a + (b - a) * dx, v1)
    out = (v1 + (v2 - v1) * dy).astype(np.int64).astype(np.uint8)
    return np.where(inside[..., None], out, 0).astype(np.uint8)


def fix16(v):
    return int(math.floor(v * 65536.0 + 0.5))


def rotate_nearest(img, angle):
    m, nw, nh = rotation_matrix(img.shape[1], img.shape[0], angle)
    if m is None:
        return img.copy()
    h, w = img.shape[:2]
    a0, a1, a3, a4 = fix16(m[0]), fix16(m[1]), fix16(m[3]), fix16(m[4])
    a2 = fix16(m[2] + m[0] * 0.5 + m[1] * 0.5)
    a5 = fix16(m[5] + m[3] * 0.5 + m[4] * 0.5)
    x, y = np.arange(nw, dtype=np.int64)[None, :], np.arange(nh, dtype=np.int64)[:, None]
    xin = (a2 + a1 * y + a0 * x) >> 16
    yin = (a5 + a4 * y + a3 * x) >> 16
    inside = (xin >= 0) & (xin < w) & (yin >= 0) & (yin < h)
    out = img[np.clip(yin, 0, h - 1), np.clip(xin, 0, w - 1)]
    return np.where(inside[..., None], out, 0).astype(np.uint8)


# ---- resize -------------------------------------------------------------------------------------------------------------------------------
def _coeffs(inS, outS):
    scale = float(inS) / float(outS)
    fs = max(scale, 1.0)
    support = 1.0 * fs
    ss = 1.0 / fs
    out = []
    for xx in range(outS):
        c = (xx + 0.5) * scale
        xmin = max(int(c - support + 0.5), 0)
        xmax = min(int(c + support + 0.5), inS)
        k = []
        ww = 0.0
        for x in range(xmax - xmin):
            wgt = max(0.0, 1.0 - abs((x + xmin - c + 0.5) * ss))
            k.append(wgt)
            ww += wgt
        kk = np.array([int(0.5 + (v / ww if ww != 0.0 else v) * (1 << PRECISION_BITS)) for v in k], np.int64)
        out.append((xmin, kk))
    return out


def _pass(img, outS):
    res = np.empty((img.shape[0], outS, img.shape[2]), np.uint8)
    src = img.astype(np.int64)
    for xx, (xmin, kk) in enumerate(_coeffs(img.shape[1], outS)):
        acc = (1 << (PRECISION_BITS - 1)) + np.tensordot(src[:, xmin:xmin + len(kk)], kk, axes=([1], [0]))
        res[:, xx] = np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)
    return res


def resize_bilinear(img, size=OUT):
    """resize((size, size), BILINEAR): the horizontal pass over all rows, then the vertical pass over its uint8 result"""
    hp = _pass(np.ascontiguousarray(img), size)
    return _pass(hp.transpose(1, 0, 2), size).transpose(1, 0, 2)


def nearest_index(inS, outS):
    """ImagingScaleAffine's source index per output index: the coordinate starts at scale / 2 and grows by one float64 addition per step"""
    step = float(inS) / float(outS)
    o = 0.0 + step * 0.5
    idx = np.empty(outS, np.int64)
    for x in range(outS):
        idx[x] = -1 if o < 0.0 else int(o)
        o += step
    return idx                                           # (always inside [0, inS) for these sizes; the tests check it)


def resize_nearest(img, size=OUT):
    return np.ascontiguousarray(img[nearest_index(img.shape[0], size)][:, nearest_index(img.shape[1], size)])


# ---- the chain ----------------------------------------------------------------------------------------------------------------------------
def augment(rgb, uvw, factors, order, angle, box, stages=False):
    """One sample.  box = (i, j, h, w) inside the 128 x 128 intermediate.  Returns (rgb u8 [128][128][3], uvw u8 [128][128][3]); with stages a
    dict of every intermediate image as well."""
    i, j, bh, bw = (int(v) for v in box)
    jit = jitter(rgb, factors, order)
    rot = rotate_bilinear(jit, angle)
    mid = resize_bilinear(rot)
    fin = resize_bilinear(mid[i:i + bh, j:j + bw])
    urot = rotate_nearest(uvw, angle)
    umid = resize_nearest(urot)
    ufin = resize_nearest(umid[i:i + bh, j:j + bw])
    if stages:
        return fin, ufin, dict(jitter=jit, rotated=rot, mid=mid, uvw_rotated=urot, uvw_mid=umid)
    return fin, ufin


def to_tensor(u8):
    """ToTensor + Normalize of a uint8 [128][128][3] image: float32 [3][128][128], each operation rounded separately"""
    x = u8.transpose(2, 0, 1).astype(np.float32) / np.float32(255.0)
    return ((x - MEAN[:, None, None]) / STD[:, None, None]).astype(np.float32)


def mask_of(uvw_u8):
    return (uvw_u8.astype(np.int32).sum(-1) > 0).astype(np.uint8)
