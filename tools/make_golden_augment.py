"""Golden G22 (tests/golden/g22_augment.npz): the augmentation of the CSS training crops, from Pillow itself.

Runs the Pillow calls that torchvision's PIL backend makes for the transforms of the reference's datasets/crops.py, with EXPLICIT parameters
(no random stream is involved), and records inputs and results.  Only DATA is committed: small synthetic sources, the parameter rows, and
per case the uint8 image after the colour jitter, after the rotation, and final, and the final UVW labels.

  ColorJitter           ImageEnhance.Brightness / Contrast / Color(.enhance(f)) and, for hue, convert('HSV'), np_h += np.uint8(f * 255),
                        merge, convert('RGB') (functional_pil.adjust_hue; skipped for f = 0), in the case's order
  RandomRotation        img.rotate(angle, BILINEAR | NEAREST, expand=True)
  Resize((128, 128))    img.resize((128, 128), BILINEAR | NEAREST)
  RandomResizedCrop     img.crop((j, i, j + w, i + h)).resize((128, 128), BILINEAR | NEAREST)

torchvision is not installed where this file is made: that mapping is written from its PIL backend and not tested against it.
The float32 tensors are not stored; the tests recompute them from the final bytes with torch on the CPU.

Cases: the sizes 3 x 5, 17 x 128, 128 x 17, 128 x 128, 129 x 64 and 200 x 150 (w x h) once each and 61 x 47 five times; between them every factor row, order, angle and box below; factors at 0.6, 1.0, 1.4 and inside; hue at -0.2, 0,
0.2; angles 0, 1e-3, +-10 and inside; boxes that are the whole intermediate, touch each edge, and have the smallest area (0.5 * 128^2 at the
extreme ratios); eight different jitter orders (all 24 are covered against Pillow directly in tests/test_augment_cpu.py).
"""
import itertools
import os

import numpy as np
import PIL
from PIL import Image, ImageEnhance

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "..", "tests", "golden", "g22_augment.npz")
S = 128


def source(rng, w, h, k):
    """an RGB image of flat random blocks, one ramp channel and sparse noise (the file has to stay small) and a UVW label image: an ellipse of NOCS-like labels, the values 1
    and 255 among them, on a black background"""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    blocks = rng.integers(0, 256, ((h + 4) // 5, (w + 4) // 5, 3)).astype(np.float64)      # flat 5 x 5 blocks: edges for the filters, small file
    base = np.repeat(np.repeat(blocks, 5, 0), 5, 1)[:h, :w]
    base[..., 2] = 255 * (x + y) / max(w + h - 2, 1) + 0 * k
    rgb = np.clip(base + 40.0 * rng.normal(0, 1, base.shape) * (rng.random(base.shape) < 0.04), 0, 255).astype(np.uint8)
    inside = ((x - (w - 1) / 2) / (0.42 * w + 0.5)) ** 2 + ((y - (h - 1) / 2) / (0.42 * h + 0.5)) ** 2 <= 1.0
    uvw = np.stack([1 + 254 * x / max(w - 1, 1), 1 + 254 * y / max(h - 1, 1), 255 - 254 * (x + y) / max(w + h - 2, 1)], -1).astype(np.uint8)
    uvw[::4, ::3] = (1, 0, 0)
    uvw[1::4, 1::3] = (0, 0, 255)
    uvw[~inside] = 0
    return rgb, uvw


def pil_jitter(im, factors, order):
    for op in order:
        f = float(factors[op])
        if op == 0:
            im = ImageEnhance.Brightness(im).enhance(f)
        elif op == 1:
            im = ImageEnhance.Contrast(im).enhance(f)
        elif op == 2:
            im = ImageEnhance.Color(im).enhance(f)
        elif f != 0:
            h, s, v = im.convert("HSV").split()
            np_h = np.array(h, dtype=np.uint8)
            with np.errstate(over="ignore"):
                np_h += np.array(f * 255).astype(np.int64).astype(np.uint8)
            im = Image.merge("HSV", (Image.fromarray(np_h), s, v)).convert("RGB")
    return im


def pil_geometry(im, angle, box, resample):
    i, j, h, w = box
    rot = im.rotate(angle, resample, expand=True)
    mid = rot.resize((S, S), resample)
    return rot, mid.crop((j, i, j + w, i + h)).resize((S, S), resample)


def main():
    rng = np.random.default_rng(22)
    sizes = [(3, 5), (17, 128), (128, 17), (128, 128), (129, 64), (200, 150)]
    factors = [(0.6, 1.4, 1.0, -0.2), (1.4, 0.6, 0.6, 0.2), (1.0, 1.0, 1.4, 0.0), (0.83, 1.21, 0.77, 0.11), (1.4, 1.4, 1.4, -0.07),
               (0.6, 0.6, 0.6, 0.2), (1.17, 0.95, 1.33, -0.2), (0.71, 1.4, 0.6, 0.05)]
    angles = [0.0, 1e-3, 10.0, -10.0, 3.7, -6.25, 10.0, -1e-3]
    boxes = [(0, 0, 128, 128), (0, 0, 105, 78), (23, 50, 105, 78), (50, 0, 78, 105), (0, 23, 78, 105), (19, 19, 91, 91), (5, 9, 110, 97),
             (38, 0, 90, 128)]
    perms = list(itertools.permutations(range(4)))
    orders = [perms[k] for k in (0, 23, 9, 14, 5, 18, 7, 16)]
    cases = []
    k = 0
    for k, (w, h) in enumerate(sizes):                   # every size once
        cases.append(((w, h), factors[k], orders[k], angles[(k + 2) % 8], boxes[(k * 3 + 1) % 8]))
    for q in range(3, 8):                                # the remaining parameter rows on a small source
        cases.append(((61, 47), factors[q], orders[(q + 3) % 8], angles[(q + 5) % 8], boxes[q]))
    out = {"n": np.int32(len(cases)), "pillow_version": np.array(PIL.__version__)}
    params = np.zeros((len(cases), 13), np.float64)
    for c, ((w, h), fac, order, angle, box) in enumerate(cases):
        rgb, uvw = source(rng, w, h, c)
        params[c] = list(fac) + list(order) + [angle] + list(box)
        jit = pil_jitter(Image.fromarray(rgb), fac, order)
        rot, fin = pil_geometry(jit, angle, box, Image.BILINEAR)
        _, ufin = pil_geometry(Image.fromarray(uvw), angle, box, Image.NEAREST)
        out["rgb_%d" % c], out["uvw_%d" % c] = rgb, uvw
        out["jitter_%d" % c], out["rotated_%d" % c] = np.asarray(jit), np.asarray(rot)
        out["final_%d" % c], out["uvw_final_%d" % c] = np.asarray(fin), np.asarray(ufin)
    out["params"] = params
    np.savez_compressed(OUT, **out)
    print("wrote %s: %d cases, %d bytes" % (OUT, len(cases), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
