"""bootstrap_crops -- a CSS training folder of synthetic renderings of the shape prior: the step the loop of the method starts from (fit
decoder -> synthetic crops -> CSS network -> refinement -> verified autolabels -> training data of the next CSS network).

    from sdflabel_amd.pipelines.synth_crops import bootstrap_crops
    bootstrap_crops(dsdf, latents, folder, 10000, K, (1242, 375), seed=0)
    train_css(cfgp, augment='device')                  # with the config's crops path set to the folder

The folder is what datasets.crops.Crops and train_css read.  No operating point is claimed for any of the draws' ranges (synth.draw_scenes).
"""
import numpy as np
import torch

from .. import synth
from ..export import Crop, CropWriter


def bootstrap_crops(dsdf, latents, path, n_crops, K, image_size, seed=0, batch_scenes=8, min_visible=0.0, resolution=64, z_min=0.1,
                    min_pixels=16, backgrounds=None, max_batches=None, **draw):
    """Write n_crops synthetic crops into the folder `path` (created, or appended to) through export.CropWriter.

    Scenes seed's 0, 1, 2, ... are drawn batch_scenes at a time (synth.draw_scenes(**draw); a scene depends on (seed, its index) only, so
    the folder does not depend on batch_scenes) and rendered by synth.scenes_many.  A crop is written when it is usable (flag bit 1 clear,
    at least one visible pixel) and its visible share -- visible over covered pixels inside its box -- is at least min_visible; min_visible
    is the caller's parameter and the default filters nothing.  Every entry carries {'synthetic': True, 'scene', 'object', 'yaw', 'visible',
    'covered', 'box'} beside the raw latent decoded, the crop's intrinsics and the label's cam_T.
    Per batch: scenes_many's host reads, and ONE more for the counts and bytes of all its crops.  max_batches: give up after that many
    batches (None: 16 + 4 n_crops / batch_scenes) -- scenes whose objects all hide each other write nothing.  Returns the number written."""
    n_crops, batch_scenes = int(n_crops), int(batch_scenes)
    if n_crops < 1 or batch_scenes < 1:
        raise ValueError("bootstrap_crops: n_crops and batch_scenes must be positive")
    n_latents = int(latents.shape[0])
    gen = torch.Generator().manual_seed(int(seed))
    if backgrounds is not None:
        draw.setdefault('n_backgrounds', int(backgrounds.shape[0]))
    limit = int(max_batches) if max_batches is not None else 16 + 4 * n_crops // batch_scenes
    written, first = 0, 0
    with CropWriter(path) as writer:
        for _ in range(limit):
            scenes = synth.draw_scenes(gen, batch_scenes, n_latents, K, image_size, first_scene=first, z_min=z_min, **draw)
            first += batch_scenes
            crops, _ = synth.scenes_many(dsdf, latents, scenes, K, image_size, resolution=resolution, z_min=z_min, min_pixels=min_pixels,
                                         backgrounds=backgrounds)
            if not crops:
                continue
            dev = crops[0].uvw.device
            parts, sizes = [], []
            for c in crops:
                part = [torch.stack([c.counts[0], c.counts[1], c.counts[2], c.flags.to(torch.int32)]).contiguous().view(torch.uint8),
                        c.latent.detach().to(dev, torch.float32).reshape(-1).contiguous().view(torch.uint8), c.uvw.reshape(-1), c.rgb.reshape(-1)]
                parts += part
                sizes.append([int(p.numel()) for p in part])
            host = torch.cat(parts).cpu().numpy()                            # the one further host read of the batch
            o = 0
            for c, sz in zip(crops, sizes):
                counts = host[o:o + sz[0]].view(np.int32)
                lat = host[o + sz[0]:o + sz[0] + sz[1]].view(np.float32)
                shape = tuple(c.uvw.shape)
                uvw = host[o + sz[0] + sz[1]:o + sum(sz[:3])].reshape(shape)
                rgb = host[o + sum(sz[:3]):o + sum(sz)].reshape(shape)
                o += sum(sz)
                n, covered, visible, flags = (int(x) for x in counts)
                if n == 0 or visible == 0 or (flags & 2) or not float(visible) / float(covered) >= float(min_visible):
                    continue
                writer.add(Crop(uvw, rgb, c.box, c.window, counts, flags), lat, c.intrinsics, c.extrinsics, synthetic=True, scene=int(c.scene),
                           object=int(c.object), yaw=float(c.yaw), visible=visible, covered=covered, box=[int(x) for x in c.box])
                written += 1
                if written == n_crops:
                    return written
    raise RuntimeError("bootstrap_crops: %d of %d crops after %d batches of %d scenes (min_visible = %g leaves too few)"
                       % (written, n_crops, limit, batch_scenes, float(min_visible)))
