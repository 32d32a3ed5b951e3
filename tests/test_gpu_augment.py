"""The augmentation of the CSS training crops on the GPU (csrc/augment.hip, sdflabel_amd/augment.py, datasets/crops.py) against golden G22 --
recorded from Pillow itself by tools/make_golden_augment.py -- and against the numpy restatement of tests/_augment_ref.py, which
tests/test_augment_cpu.py pins to Pillow and to the same golden.  Everything is exact: bytes and float bits are compared for equality, so
there is no tolerance to choose."""
import os
import warnings

import numpy as np
import pytest
import torch

from sdflabel_amd import augment
from tests import _augment_ref as R
from tests._util import gold

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def g():
    return gold("g22_augment.npz")


def sources(g, cases):
    return [g["rgb_%d" % c] for c in cases], [g["uvw_%d" % c] for c in cases], g["params"][list(cases)]


@pytest.fixture(scope="module")
def whole(g):
    """all of G22 as one batch, run once"""
    rgb_l, uvw_l, p = sources(g, range(int(g["n"])))
    rgb, uvw, mask, st = augment.augment_many(rgb_l, uvw_l, p, device=DEV, return_stages=True)
    return rgb.cpu(), uvw.cpu(), mask.cpu(), st["rgb_u8"].cpu(), [j.cpu() for j in st["jitter"]]


def bits(t):
    return t.contiguous().view(torch.int32)


def test_golden_g22_byte_for_byte(g, whole):
    rgb, uvw, mask, rgb_u8, jit = whole
    mean, std = torch.tensor(R.MEAN)[:, None, None], torch.tensor(R.STD)[:, None, None]
    for c in range(int(g["n"])):
        for name, got, ref in (("jitter", jit[c].numpy(), g["jitter_%d" % c]), ("final", rgb_u8[c].numpy(), g["final_%d" % c]),
                               ("uvw", uvw[c].permute(1, 2, 0).numpy(), g["uvw_final_%d" % c])):
            print("case %d %s: %d differing bytes of %d" % (c, name, int((got != ref).sum()), ref.size))
            assert got.shape == ref.shape and np.array_equal(got, ref), (c, name)
        x = torch.from_numpy(g["final_%d" % c]).permute(2, 0, 1).float() / 255.0             # ToTensor, Normalize: torch on the CPU
        assert torch.equal(bits(rgb[c]), bits((x - mean) / std)), c
        assert np.array_equal(mask[c].numpy(), R.mask_of(g["uvw_final_%d" % c])), c


def test_a_sample_has_the_same_bits_alone_and_anywhere_in_a_batch(g, whole):
    c = 5                                                                                    # the 200 x 150 source
    others = [0, 1, 2, 3, 4, 6]
    for cases in ([c], [c] + others, others + [c], others[:3] + [c] + others[3:]):
        out = augment.augment_many(*sources(g, cases), device=DEV, return_stages=True)
        k = cases.index(c)
        assert torch.equal(bits(out[0][k].cpu()), bits(whole[0][c])), cases
        assert torch.equal(out[1][k].cpu(), whole[1][c]) and torch.equal(out[2][k].cpu(), whole[2][c]), cases
        assert torch.equal(out[3]["rgb_u8"][k].cpu(), whole[3][c]) and torch.equal(out[3]["jitter"][k].cpu(), whole[4][c]), cases


def test_two_runs_are_identical_and_nothing_synchronises(g, whole):
    rgb_l, uvw_l, p = sources(g, range(int(g["n"])))
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            out = augment.augment_many(rgb_l, uvw_l, p, device=DEV)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert sum("synchroniz" in str(x.message).lower() for x in w) == 0
    assert torch.equal(bits(out[0].cpu()), bits(whole[0])) and torch.equal(out[1].cpu(), whole[1]) and torch.equal(out[2].cpu(), whole[2])


def test_masks_and_labels(g):
    rgb_src = g["rgb_5"]
    h, w = rgb_src.shape[:2]
    black = np.zeros((h, w, 3), np.uint8)
    one, top = black.copy(), black.copy()
    one[..., 0], top[..., 2] = 1, 255
    ident = [1.0, 1.0, 1.0, 0.0, 0, 1, 2, 3, 0.0, 0, 0, 128, 128]                            # no rotation, the whole intermediate
    turned = [1.0, 1.0, 1.0, 0.0, 0, 1, 2, 3, 10.0, 0, 0, 128, 128]
    white = np.full((h, w, 3), 255, np.uint8)
    rgb, uvw, mask, st = augment.augment_many([rgb_src, rgb_src, rgb_src, white, white], [black, one, top, top, top],
                                              [turned, ident, ident, turned, [1.0, 1.0, 1.0, 0.0, 0, 1, 2, 3, -10.0, 0, 0, 128, 128]],
                                              device=DEV, return_stages=True)
    uvw, mask, u8 = uvw.cpu().numpy(), mask.cpu().numpy(), st["rgb_u8"].cpu().numpy()
    assert mask.dtype == np.uint8 and not mask[0].any() and not uvw[0].any()                 # all-black labels: an empty mask
    assert (uvw[1, 0] == 1).all() and not uvw[1, 1:].any() and (mask[1] == 1).all()          # label 1 survives everywhere
    assert (uvw[2, 2] == 255).all() and not uvw[2, :2].any() and (mask[2] == 1).all()        # label 255 survives
    for s in (3, 4):                                                                         # +-10 degrees: the corners lie outside the source
        for y, x in ((0, 0), (0, 127), (127, 0), (127, 127)):
            assert not u8[s, y, x].any() and not uvw[s, :, y, x].any() and mask[s, y, x] == 0, (s, y, x)
        assert (u8[s, 64, 64] == 255).all() and uvw[s, 2, 64, 64] == 255 and mask[s, 64, 64] == 1
        ref, uref = R.augment(white, top, turned[0:4], [0, 1, 2, 3], 10.0 if s == 3 else -10.0, (0, 0, 128, 128))
        assert np.array_equal(u8[s], ref) and np.array_equal(uvw[s].transpose(1, 2, 0), uref)
        assert np.array_equal(mask[s], R.mask_of(uref))


def test_bad_arguments_are_refused(g):
    rgb_l, uvw_l, p = sources(g, [0])
    for col, value in ((9, 1.0), (12, 129.0), (11, 0.0), (10, 0.5), (4, 1.0), (3, 0.7), (8, 90.0)):      # box outside / empty / fractional,
        q = p.copy()                                                                                    # order no permutation, hue, transpose
        q[0, 9:13] = (0, 0, 128, 128)
        q[0, col] = value
        with pytest.raises(ValueError):
            augment.augment_many(rgb_l, uvw_l, q, device=DEV)
    with pytest.raises(ValueError):
        augment.augment_many(rgb_l, [uvw_l[0][:-1]], p, device=DEV)
    with pytest.raises(ValueError):
        augment.augment_many([rgb_l[0].astype(np.float32)], uvw_l, p, device=DEV)
    empty = augment.augment_many([], [], np.zeros((0, 13)), device=DEV)
    assert tuple(empty[0].shape) == (0, 3, 128, 128) and tuple(empty[2].shape) == (0, 128, 128)


def _write_dataset(path, n):
    import json
    from PIL import Image
    rng = np.random.default_rng(3)
    gt = {}
    for k in range(n):
        w, h = int(rng.integers(30, 70)), int(rng.integers(30, 70))
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(os.path.join(path, "%05d_rgb.png" % k))
        uvw = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        uvw[: h // 3] = 0
        Image.fromarray(uvw).save(os.path.join(path, "%05d_uvw.png" % k))
        gt[str(k)] = [{"latent": rng.normal(size=3).tolist(), "extrinsics": np.eye(4).reshape(-1).tolist(),
                       "intrinsics": np.eye(3).reshape(-1).tolist()}]
    with open(os.path.join(path, "crops.json"), "w") as f:
        json.dump(gt, f)


def test_loader_feeds_train_step(tmp_path):
    pytest.importorskip("PIL")
    import copy
    from sdflabel_amd.datasets.crops import Crops, DeviceCropLoader
    from sdflabel_amd.networks.resnet_css import setup_css
    from sdflabel_amd.pipelines.train_css import train_step
    _write_dataset(str(tmp_path), 3)
    ds = Crops(str(tmp_path))
    loader = DeviceCropLoader(ds, batch_size=2, shuffle=True, generator=torch.Generator().manual_seed(7), device=DEV)
    batches = list(loader)
    assert len(loader) == 2 and [len(b["rgb"]) for b in batches] == [2, 1]
    b = batches[0]
    assert b["rgb"].is_cuda and b["rgb"].dtype == torch.float32 and tuple(b["rgb"].shape) == (2, 3, 128, 128)
    assert b["uvw"].dtype == torch.uint8 and tuple(b["uvw"].shape) == (2, 3, 128, 128)
    assert b["mask"].dtype == torch.uint8 and tuple(b["mask"].shape) == (2, 128, 128)
    assert torch.equal(b["mask"], (b["uvw"].int().sum(1) > 0).to(torch.uint8)) and 0 < int(b["mask"].sum()) < b["mask"].numel()
    assert tuple(b["latent"].shape) == (2, 3) and tuple(b["crop_size"].shape) == (2, 2) and tuple(b["pose"].shape) == (2, 4, 4)
    again = next(iter(DeviceCropLoader(ds, batch_size=2, shuffle=True, generator=torch.Generator().manual_seed(7), device=DEV)))
    assert torch.equal(bits(again["rgb"]), bits(b["rgb"])) and torch.equal(again["uvw"], b["uvw"])      # the generator is the only randomness
    torch.manual_seed(1)
    net = setup_css(mode="train").to(DEV)
    twin = copy.deepcopy(net)
    got = train_step(net, torch.optim.Adam(net.parameters(), lr=1e-4), b)
    direct = {"rgb": b["rgb"].clone(), "uvw": b["uvw"].long(), "mask": b["mask"].long(), "latent": b["latent"].clone()}
    ref = train_step(twin, torch.optim.Adam(twin.parameters(), lr=1e-4), direct)
    for k in ("loss", "uvw", "mask", "latent"):
        print("%s: %.9g from the loader's batch, %.9g from the tensors" % (k, float(got[k]), float(ref[k])))
        assert torch.isfinite(got[k]).all() and torch.equal(got[k], ref[k]), k


def test_train_css_builds_the_device_loader(tmp_path, monkeypatch):
    pytest.importorskip("PIL")
    import configparser
    from sdflabel_amd.datasets import crops as C
    from sdflabel_amd.pipelines.train_css import train_css
    _write_dataset(str(tmp_path), 3)
    built = []

    class Spy(C.DeviceCropLoader):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            built.append(self)
    monkeypatch.setattr(C, "DeviceCropLoader", Spy)
    cfgp = configparser.ConfigParser()
    cfgp.read_dict({"input": {"data_path": str(tmp_path)}, "train": {"batch_size": "2", "epochs": "0"}, "log": {"dir": str(tmp_path / "log")}})
    net = train_css(cfgp, augment="device")
    assert isinstance(net, torch.nn.Module)
    assert len(built) == 1 and isinstance(built[0].dataset, C.Crops) and built[0].batch_size == 2 and built[0].shuffle and len(built[0].dataset) == 3
