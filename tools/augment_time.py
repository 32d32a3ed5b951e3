"""GPU timing of the training-crop augmentation (sdflabel_amd.augment) for 16 and 32 sources of about 200 x 150 pixels.

launches     sdfr_augment's four kernels on a batch that is already on the device (augment.run_batch): device events around windows of INNER
             calls, median of REPS windows after WARM warm-up windows.  This is the device time of the augmentation.
call         augment_many from host images (checks, Image.rotate's matrices, two uploads, the launches): a host clock around calls that end in
             a synchronise, and the kernel launches, copies and host synchronisations of one call (torch.profiler, sync debug mode).
train_step   one optimisation step of the CSS network (pipelines.train_css.train_step) fed by DeviceCropLoader over an in-memory dataset of the
             same sources -- parameter draw, augmentation and step -- against the same step on batches made beforehand; host clock, the two
             sides alternating, each ending in a synchronise.
pillow       the same twelve Pillow operations per sample on ONE CPU thread of the machine this runs on (decoding excluded), if Pillow can be
             imported there; otherwise the JSON says so and quotes the 7.9 ms per sample of the issue that asked for this tool, measured on
             another machine's CPU and not verified here.
No ratio is asserted anywhere.

usage: python tools/augment_time.py OUT_DIR          (writes OUT_DIR/augment_time.json)
"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from frame_time import count_launches, count_syncs  # noqa: E402
from sdflabel_amd import augment  # noqa: E402
from sdflabel_amd.datasets.crops import DeviceCropLoader  # noqa: E402
from sdflabel_amd.networks.resnet_css import setup_css  # noqa: E402
from sdflabel_amd.pipelines.train_css import train_step  # noqa: E402

DEV = "cuda:0"
WARM, REPS, INNER = 2, 9, 10
STEP_WARM, STEP_REPS = 3, 9


def stat(v):
    return {"median_ms": round(float(np.median(v)), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}


def make_sources(n, seed):
    """n RGB / UVW pairs of about 200 x 150 pixels: random bytes, labels inside an ellipse"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        w, h = int(rng.integers(180, 221)), int(rng.integers(135, 166))
        y, x = np.mgrid[0:h, 0:w]
        uvw = rng.integers(1, 256, (h, w, 3), dtype=np.uint8)
        uvw[((x - w / 2) / (0.45 * w)) ** 2 + ((y - h / 2) / (0.45 * h)) ** 2 > 1] = 0
        out.append((rng.integers(0, 256, (h, w, 3), dtype=np.uint8), uvw))
    return out


class MemoryCrops:
    """the dataset interface of sdflabel_amd.datasets.crops.Crops over images held in memory (decoding is not part of any figure here)"""

    def __init__(self, sources):
        self.sources = sources

    def __len__(self):
        return len(self.sources)

    def __getitem__(self, idx):
        rgb, uvw = self.sources[idx]
        return {"rgb": rgb, "uvw": uvw, "latent": torch.tensor([0.3, -0.5, 0.8]), "crop_size": torch.tensor([rgb.shape[1], rgb.shape[0]]),
                "intrinsics": torch.eye(3), "pose": torch.eye(4)}


def event_windows(fn):
    def window():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(INNER):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / INNER
    for _ in range(WARM):
        window()
    return stat([window() for _ in range(REPS)])


def host_clock(fns, warm, reps):
    """the functions alternate; each call ends in a synchronise"""
    for _ in range(warm):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for fn, t in zip(fns, ts):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            t.append((time.perf_counter() - t0) * 1e3)
    return [stat(t) for t in ts]


def pillow_one_thread(sources, params):
    """the Pillow calls of torchvision's PIL backend for the reference's transforms, per sample, on one thread"""
    try:
        from PIL import Image, ImageEnhance
    except ImportError:
        return {"measured": False, "reason": "Pillow cannot be imported on this machine",
                "quoted_ms_per_sample": 7.9, "quoted_from": "the issue that asked for this tool: another machine's CPU, one thread, 200 x 150 "
                "sources, decoding excluded; NOT verified here"}
    torch.set_num_threads(1)
    enh = (ImageEnhance.Brightness, ImageEnhance.Contrast, ImageEnhance.Color)

    def one(rgb, uvw, p):
        im = Image.fromarray(rgb)
        for op in p[4:8].astype(int):
            if op < 3:
                im = enh[op](im).enhance(float(p[op]))
            elif p[3] != 0:
                h, s, v = im.convert("HSV").split()
                np_h = np.array(h, dtype=np.uint8)
                np_h += np.array(p[3] * 255).astype(np.int64).astype(np.uint8)
                im = Image.merge("HSV", (Image.fromarray(np_h), s, v)).convert("RGB")
        i, j, bh, bw = (int(v) for v in p[9:13])
        res = []
        for img, rs in ((im, Image.BILINEAR), (Image.fromarray(uvw), Image.NEAREST)):
            res.append(np.asarray(img.rotate(float(p[8]), rs, expand=True).resize((128, 128), rs).crop((j, i, j + bw, i + bh))
                                  .resize((128, 128), rs)))
        return res
    per = []
    for _ in range(5):
        t0 = time.perf_counter()
        for (rgb, uvw), p in zip(sources, params):
            one(rgb, uvw, p)
        per.append((time.perf_counter() - t0) * 1e3 / len(sources))
    import PIL
    return {"measured": True, "pillow_version": PIL.__version__, "ms_per_sample_one_thread": stat(per), "samples": len(sources),
            "note": "this machine's CPU, one thread, decoding excluded; the float tensors and the mask are not made"}


def main():
    out_dir = sys.argv[1] if len(sys.argv) > 1 else "."
    os.makedirs(out_dir, exist_ok=True)
    assert torch.cuda.is_available(), "augment_time.py measures on the GPU only"
    res = {"config": "sources of 180-220 x 135-165 random bytes; launches: device events around windows of %d calls, median of %d windows after "
                     "%d warm-up windows; call and train_step: host clock around work that ends in a synchronise, sides alternating, median "
                     "of %d after %d warm-up rounds" % (INNER, REPS, WARM, STEP_REPS, STEP_WARM), "sizes": {}}
    torch.manual_seed(1)
    net = setup_css(mode="train").to(DEV)
    opt = torch.optim.Adam(net.parameters(), lr=1e-4)
    for B in (16, 32):
        src = make_sources(B, seed=B)
        rgb_l, uvw_l = [s[0] for s in src], [s[1] for s in src]
        params = augment.draw_params([(r.shape[1], r.shape[0]) for r in rgb_l], torch.Generator().manual_seed(B))
        batch = augment.pack_batch(rgb_l, uvw_l, params, torch.device(DEV))
        launches = event_windows(lambda: augment.run_batch(batch))
        call = lambda: augment.augment_many(rgb_l, uvw_l, params, device=DEV)                                   # noqa: E731
        k, c = count_launches(call)
        call_ms, = host_clock([call], STEP_WARM, STEP_REPS)
        # one training step: loader-fed (draw + augmentation + step) against batches made beforehand
        ds = MemoryCrops(src)
        gen = torch.Generator().manual_seed(3)
        ready = [next(iter(DeviceCropLoader(ds, batch_size=B, shuffle=True, generator=gen, device=DEV))) for _ in range(4)]
        state = {"n": 0}

        def fed():
            train_step(net, opt, next(iter(DeviceCropLoader(ds, batch_size=B, shuffle=True, generator=gen, device=DEV))))

        def premade():
            state["n"] += 1
            train_step(net, opt, ready[state["n"] % len(ready)])
        t_fed, t_pre = host_clock([fed, premade], STEP_WARM, STEP_REPS)
        res["sizes"]["B%d" % B] = {"source_pixels": int(batch["pixels"]), "launches_device_ms": launches, "augment_many_call_ms": call_ms,
                                   "kernel_launches": k, "copies": c, "host_synchronisations": count_syncs(call),
                                   "train_step_loader_fed_ms": t_fed, "train_step_premade_batches_ms": t_pre,
                                   "loader_cost_per_step_ms": round(t_fed["median_ms"] - t_pre["median_ms"], 4)}
        print("B=%d" % B, json.dumps(res["sizes"]["B%d" % B]))
        if B == 32:
            res["pillow_cpu"] = pillow_one_thread(src, params)
            print("pillow", json.dumps(res["pillow_cpu"]))
    json.dump(res, open(os.path.join(out_dir, "augment_time.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
