"""The augmentation of the CSS training crops, without a GPU: the numpy restatement (tests/_augment_ref.py) against Pillow itself stage by
stage, golden G22 against the restatement, the host side of sdflabel_amd.augment (parameter draws, Image.rotate's matrix, no CPU fallback)
and the dataset / loader plumbing."""
import itertools
import os
import re

import numpy as np
import pytest
import torch

from tests import _augment_ref as R

PILImage = pytest.importorskip("PIL.Image")
from PIL import ImageEnhance  # noqa: E402

from sdflabel_amd import _lib, augment  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(3, 5), (17, 128), (128, 17), (128, 128), (129, 64), (200, 150)]          # (w, h)
ANGLES = [0.0, 1e-3, 10.0, -10.0]
# (i, j, h, w): the whole intermediate; each edge touched; the smallest area of RandomResizedCrop (0.5 * 128^2) at both extreme ratios
BOXES = [(0, 0, 128, 128), (0, 0, 105, 78), (23, 50, 105, 78), (50, 0, 78, 105), (0, 23, 78, 105), (38, 0, 90, 128), (0, 9, 128, 97)]


def _image(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _pil_hue(im, f):
    """functional_pil.adjust_hue"""
    h, s, v = im.convert("HSV").split()
    np_h = np.array(h, dtype=np.uint8)
    np_h += np.array(f * 255).astype(np.int64).astype(np.uint8)
    return PILImage.merge("HSV", (PILImage.fromarray(np_h), s, v)).convert("RGB")


def _pil_op(im, op, f):
    if op == 3:
        return im if f == 0 else _pil_hue(im, f)
    return (ImageEnhance.Brightness, ImageEnhance.Contrast, ImageEnhance.Color)[op](im).enhance(f)


@pytest.mark.parametrize("size", SIZES)
def test_blend_operations_equal_pillow(size):
    img = _image(*size, seed=1)
    im = PILImage.fromarray(img)
    for f in (0.6, 1.0, 1.4, 0.0, 0.73, 1.27):
        assert np.array_equal(np.asarray(ImageEnhance.Brightness(im).enhance(f)), R.brightness(img, f)), f
        assert np.array_equal(np.asarray(ImageEnhance.Contrast(im).enhance(f)), R.contrast(img, f)), f
        assert np.array_equal(np.asarray(ImageEnhance.Color(im).enhance(f)), R.saturation(img, f)), f


def test_brightness_over_all_bytes():
    ramp = np.repeat(np.arange(256, dtype=np.uint8)[None, :, None], 3, 2)
    im = PILImage.fromarray(ramp)
    for f in np.linspace(0.6, 1.4, 81):
        assert np.array_equal(np.asarray(ImageEnhance.Brightness(im).enhance(float(f))), R.brightness(ramp, float(f))), f


def test_hue_conversions_equal_pillow_on_all_colours():
    """convert('HSV') on all 2^24 RGB colours and convert('RGB') on all 2^24 HSV triples: every byte equal (the H byte included: the
    restatement keeps the float32 / float64 rounding order of Pillow's C, so no colour differs)"""
    g, b = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    differing = 0
    for r0 in range(0, 256, 16):
        arr = np.empty((16, 256, 256, 3), np.uint8)
        arr[..., 0] = np.arange(r0, r0 + 16, dtype=np.uint8)[:, None, None]
        arr[..., 1], arr[..., 2] = g, b
        arr = arr.reshape(16 * 256, 256, 3)
        differing += int((np.asarray(PILImage.fromarray(arr).convert("HSV")) != R.rgb_to_hsv(arr)).any(-1).sum())
        back = np.asarray(PILImage.frombytes("HSV", (256, 16 * 256), arr.tobytes()).convert("RGB"))
        differing += int((back != R.hsv_to_rgb(arr)).any(-1).sum())
    assert differing == 0


@pytest.mark.parametrize("f", [-0.2, 0.0, 0.2, 0.11, -0.07, 0.5, -0.5])
def test_hue_step_equals_pillow(f):
    img = _image(129, 64, seed=2)
    assert np.array_equal(np.asarray(_pil_op(PILImage.fromarray(img), 3, f)), R.hue(img, f))


def test_all_24_jitter_orders_equal_pillow():
    img = _image(17, 128, seed=3)
    rows = [(0.6, 1.4, 1.0, -0.2), (1.4, 0.6, 0.6, 0.2), (1.0, 1.0, 1.4, 0.0)]
    for n, order in enumerate(itertools.permutations(range(4))):
        fac = rows[n % 3]
        im = PILImage.fromarray(img)
        for op in order:
            im = _pil_op(im, op, fac[op])
        assert np.array_equal(np.asarray(im), R.jitter(img, fac, order)), order


@pytest.mark.parametrize("size", SIZES)
def test_rotations_equal_pillow(size):
    img = _image(*size, seed=4)
    im = PILImage.fromarray(img)
    for angle in ANGLES + [3.7, -6.25, 359.5]:
        for resample, fn in ((PILImage.BILINEAR, R.rotate_bilinear), (PILImage.NEAREST, R.rotate_nearest)):
            ref = np.asarray(im.rotate(angle, resample, expand=True))
            got = fn(img, angle)
            assert got.shape == ref.shape and np.array_equal(got, ref), (angle, resample)


@pytest.mark.parametrize("size", SIZES)
def test_resizes_equal_pillow(size):
    img = _image(*size, seed=5)
    im = PILImage.fromarray(img)
    assert np.array_equal(np.asarray(im.resize((128, 128), PILImage.BILINEAR)), R.resize_bilinear(img))
    assert np.array_equal(np.asarray(im.resize((128, 128), PILImage.NEAREST)), R.resize_nearest(img))


def test_nearest_resize_equals_pillow_for_every_input_length():
    """ImagingScaleAffine's accumulated float64 coordinate, for every input length a rotated source or a crop box can have"""
    for n in range(1, 301):
        img = _image((n * 7) % 300 + 1, n, seed=n)
        assert np.array_equal(np.asarray(PILImage.fromarray(img).resize((128, 128), PILImage.NEAREST)), R.resize_nearest(img)), n
        idx = R.nearest_index(n, 128)
        assert idx.min() >= 0 and idx.max() < n


@pytest.mark.parametrize("box", BOXES)
def test_crop_and_resize_equal_pillow(box):
    i, j, h, w = box
    img = _image(128, 128, seed=6)
    im = PILImage.fromarray(img).crop((j, i, j + w, i + h))
    assert np.array_equal(np.asarray(im.resize((128, 128), PILImage.BILINEAR)), R.resize_bilinear(img[i:i + h, j:j + w]))
    assert np.array_equal(np.asarray(im.resize((128, 128), PILImage.NEAREST)), R.resize_nearest(img[i:i + h, j:j + w]))


@pytest.mark.parametrize("size", SIZES)
def test_whole_chain_equals_pillow(size):
    rgb, uvw = _image(*size, seed=7), _image(*size, seed=8)
    uvw[uvw[..., 0] < 128] = 0
    for n, angle in enumerate(ANGLES):
        fac, order, box = (0.6 + 0.2 * n, 1.4 - 0.2 * n, 1.0 + 0.1 * n, (-0.2, 0.0, 0.2, 0.11)[n]), (n, (n + 2) % 4, (n + 1) % 4, (n + 3) % 4), BOXES[n + 1]
        i, j, h, w = box
        im = PILImage.fromarray(rgb)
        for op in order:
            im = _pil_op(im, op, fac[op])
        fin = im.rotate(angle, PILImage.BILINEAR, expand=True).resize((128, 128), PILImage.BILINEAR).crop((j, i, j + w, i + h)) \
            .resize((128, 128), PILImage.BILINEAR)
        ufin = PILImage.fromarray(uvw).rotate(angle, PILImage.NEAREST, expand=True).resize((128, 128), PILImage.NEAREST) \
            .crop((j, i, j + w, i + h)).resize((128, 128), PILImage.NEAREST)
        got, ugot = R.augment(rgb, uvw, fac, order, angle, box)
        assert np.array_equal(got, np.asarray(fin)) and np.array_equal(ugot, np.asarray(ufin)), angle


def test_golden_g22_equals_the_restatement():
    g = np.load(os.path.join(ROOT, "tests", "golden", "g22_augment.npz"))
    assert int(g["n"]) >= 10
    seen = set()
    for c in range(int(g["n"])):
        p = g["params"][c]
        fin, ufin, st = R.augment(g["rgb_%d" % c], g["uvw_%d" % c], p[0:4], p[4:8], p[8], p[9:13], stages=True)
        for name, got in (("jitter", st["jitter"]), ("rotated", st["rotated"]), ("final", fin), ("uvw_final", ufin)):
            ref = g["%s_%d" % (name, c)]
            assert got.shape == ref.shape and np.array_equal(got, ref), (c, name)
        seen.add(g["rgb_%d" % c].shape[:2])
    assert {(h, w) for w, h in SIZES} <= seen


def test_to_tensor_equals_torch():
    u8 = _image(128, 128, seed=9)
    x = torch.from_numpy(u8).permute(2, 0, 1).float() / 255.0
    ref = (x - torch.tensor(R.MEAN)[:, None, None]) / torch.tensor(R.STD)[:, None, None]
    assert np.array_equal(R.to_tensor(u8).view(np.int32), ref.numpy().view(np.int32))


# ---- the host side of the product ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("size", SIZES)
def test_rotation_matrix_equals_the_restatement(size):
    for angle in ANGLES + [3.7, 359.5, 360.0, -360.0]:
        m, nw, nh = augment.rotation_matrix(size[0], size[1], angle)
        rm, rw, rh = R.rotation_matrix(size[0], size[1], angle)
        assert (m is None) == (rm is None) and (nw, nh) == (rw, rh)
        assert m is None or m == rm
        assert PILImage.new("RGB", size).rotate(angle, expand=True).size == (nw, nh)


def test_draw_params_ranges_and_boxes():
    gen = torch.Generator().manual_seed(5)
    p = augment.draw_params([(200, 150)] * 2000, gen)
    assert p.shape == (2000, 13) and p.dtype == np.float64
    assert (p[:, 0:3] >= 0.6).all() and (p[:, 0:3] <= 1.4).all()
    assert (np.abs(p[:, 3]) <= 0.2).all() and (np.abs(p[:, 8]) <= 10.0).all()
    assert (np.sort(p[:, 4:8], axis=1) == np.arange(4)).all()
    assert len({tuple(r) for r in p[:, 4:8].tolist()}) == 24                        # every order occurs
    i, j, h, w = p[:, 9], p[:, 10], p[:, 11], p[:, 12]
    assert np.array_equal(p[:, 9:13], np.trunc(p[:, 9:13]))
    assert (i >= 0).all() and (j >= 0).all() and (h >= 1).all() and (w >= 1).all() and (i + h <= 128).all() and (j + w <= 128).all()
    area, ratio = h * w / 128.0 ** 2, w / h
    assert area.min() >= 0.5 - 0.02 and area.max() <= 1.0 and area.std() > 0.1      # (w and h are rounded: 0.02 covers one pixel each way)
    assert ratio.min() >= 0.75 - 0.02 and ratio.max() <= 4.0 / 3.0 + 0.02
    for col in (0, 1, 2, 3, 8):                                                     # uniform draws: the mean of 2000 lies within 5 sigma
        lo, hi = ((0.6, 1.4), (0.6, 1.4), (0.6, 1.4), (-0.2, 0.2), None, None, None, None, (-10.0, 10.0))[col]
        assert abs(p[:, col].mean() - (lo + hi) / 2) < 5 * (hi - lo) / np.sqrt(12 * 2000)
    again = augment.draw_params([(200, 150)] * 2000, torch.Generator().manual_seed(5))
    assert np.array_equal(p, again)
    assert not np.array_equal(p[:1000], augment.draw_params([(3, 5)] * 1000, torch.Generator().manual_seed(6)))


def test_no_cpu_fallback_and_the_abi():
    header = open(os.path.join(ROOT, "include", "sdfr.h")).read()
    assert "sdfr_augment" in _lib.EXPORTS and re.search(r"\bint sdfr_augment\(", header)
    assert int(re.search(r"#define SDFR_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION >= 409
    assert int(re.search(r"#define SDFR_AUG_PARAMS (\d+)", header).group(1)) == augment._ROW
    for name, value in (("ORDER", augment._ORDER), ("MATRIX", augment._MATRIX), ("BOX_I", augment._BOX)):
        assert int(re.search(r"#define SDFR_AUG_%s (\d+)" % name, header).group(1)) == value
    if not torch.cuda.is_available():
        img = _image(5, 3, seed=1)
        with pytest.raises(_lib.SdfrError):
            augment.augment_many([img], [img], augment.draw_params([(5, 3)], torch.Generator().manual_seed(0)))


def test_ingest_and_augment_share_the_resample_code():
    """one statement of Pillow's coefficients: both translation units include csrc/css_resample.h and neither restates it"""
    csrc = os.path.join(ROOT, "sdflabel_amd", "csrc")
    for name in ("ingest.hip", "augment.hip"):
        text = open(os.path.join(csrc, name)).read()
        assert '#include "css_resample.h"' in text and "precompute_coeffs" not in text.replace("css_resample.h", "")
    assert "css_coef_row" in open(os.path.join(csrc, "css_resample.h")).read()
    assert "-ffp-contract=off -c \"$HERE/augment.hip\"" in open(os.path.join(csrc, "build.sh")).read()


def _write_dataset(path, n, seed=0):
    import json
    rng = np.random.default_rng(seed)
    gt = {}
    for k in range(n):
        w, h = int(rng.integers(20, 60)), int(rng.integers(20, 60))
        PILImage.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(os.path.join(path, "%05d_rgb.png" % k))
        uvw = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        uvw[: h // 3] = 0
        PILImage.fromarray(uvw).save(os.path.join(path, "%05d_uvw.png" % k))
        gt[str(k)] = [{"latent": rng.normal(size=3).tolist(), "extrinsics": np.eye(4).reshape(-1).tolist(),
                       "intrinsics": (np.eye(3) * (k + 1)).reshape(-1).tolist()}]
    with open(os.path.join(path, "crops.json"), "w") as f:
        json.dump(gt, f)


def test_crops_dataset_reads_the_reference_layout(tmp_path, monkeypatch):
    from sdflabel_amd.datasets.crops import Crops, DeviceCropLoader
    _write_dataset(str(tmp_path), 5)
    ds = Crops(str(tmp_path))
    assert len(ds) == 5
    s = ds[3]
    assert set(s) == {"rgb", "uvw", "latent", "crop_size", "intrinsics", "pose"}
    assert s["rgb"].dtype == np.uint8 and s["rgb"].shape == s["uvw"].shape and s["rgb"].shape[2] == 3
    assert np.array_equal(s["rgb"], np.asarray(PILImage.open(os.path.join(str(tmp_path), "00003_rgb.png")).convert("RGB")))
    assert s["crop_size"].tolist() == [s["rgb"].shape[1], s["rgb"].shape[0]] and s["crop_size"].dtype == torch.int64
    assert s["latent"].dtype == torch.float32 and tuple(s["intrinsics"].shape) == (3, 3) and tuple(s["pose"].shape) == (4, 4)
    assert float(s["intrinsics"][0, 0]) == 4.0
    loader = DeviceCropLoader(ds, batch_size=2, shuffle=False)
    assert len(loader) == 3 and loader.dataset is ds
    monkeypatch.syspath_prepend(os.path.join(ROOT, "sdflabel_amd", "compat"))
    import importlib
    import sys
    monkeypatch.delitem(sys.modules, "datasets", raising=False)
    monkeypatch.delitem(sys.modules, "datasets.crops", raising=False)
    mod = importlib.import_module("datasets.crops")
    assert mod.Crops is Crops and mod.DeviceCropLoader is DeviceCropLoader
    monkeypatch.delitem(sys.modules, "datasets", raising=False)
    monkeypatch.delitem(sys.modules, "datasets.crops", raising=False)


def test_train_css_refuses_an_unknown_augment():
    import configparser
    from sdflabel_amd.pipelines.train_css import train_css
    with pytest.raises(ValueError):
        train_css(configparser.ConfigParser(), augment="host")
    with pytest.raises(ValueError):
        train_css(configparser.ConfigParser(), trainloader=[], augment="device")
