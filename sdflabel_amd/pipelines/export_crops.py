"""export_frame -- a frame's verified autolabels as samples of a CSS training folder: the step that closes the loop of the method (CSS
network -> refinement -> verified autolabels -> training data of the next CSS network).

    from sdflabel_amd.export import CropWriter
    from sdflabel_amd.pipelines.export_crops import export_frame
    est, kept, stages = refine_frame(..., return_stages=True, verify=True, crops=True)
    with CropWriter(folder) as writer:
        export_frame(stages, writer)

The folder is what datasets.crops.Crops and train_css read.  Walking a dataset is the caller's loop.
"""
import numpy as np
import torch

from ..export import Crop


def export_frame(stages, writer, only_ok=True, min_visible=0.0):
    """Write the crops of refine_frame's / refine_sample's stages (crops=...) into `writer` (export.CropWriter).

    An annotation is written when its crop is usable (a non-empty box, flag bit 1 clear, at least one visible pixel), its verdict
    stages['verify'][j]['ok'] holds (only_ok=True; without stages['verify'] that raises) and its visible share -- the visible pixels of
    the crop over its covered pixels, i.e. how much of the rendered shape the frame's other annotations leave in sight inside the box -- is
    at least min_visible.  min_visible is the caller's parameter: NO OPERATING POINT IS CLAIMED for it, nothing here or in the method's
    published description fixes one, and the default 0.0 filters nothing.
    ONE host read: the counts, latents and bytes of all crops travel in one buffer.  Returns the indices into stages['crops'] written, in
    order; the writer's entries carry 'visible', 'covered' and the box as further fields."""
    crops = stages.get('crops')
    if crops is None:
        raise ValueError("export_frame: the stages hold no 'crops' (refine_frame(..., return_stages=True, crops=True))")
    verdicts = stages.get('verify')
    if only_ok and verdicts is None:
        raise ValueError("export_frame: only_ok=True needs stages['verify'] (refine_frame(..., verify=True)); pass only_ok=False to write unverified labels")
    if verdicts is not None and len(verdicts) != len(crops):
        raise ValueError("export_frame: %d verdicts for %d crops" % (len(verdicts), len(crops)))
    if not crops:
        return []
    for c in crops:
        if c.rgb is None or c.latent is None or c.intrinsics is None or c.extrinsics is None:
            raise ValueError("export_frame: a crop lacks rgb, latent, intrinsics or extrinsics")
    dev = crops[0].uvw.device
    parts, sizes = [], []
    for c in crops:
        lat = torch.as_tensor(c.latent).detach().to(dev, torch.float32).reshape(-1).contiguous()
        part = [torch.stack([c.counts[0], c.counts[1], c.counts[2], c.flags.to(torch.int32)]).contiguous().view(torch.uint8), lat.view(torch.uint8),
                c.uvw.reshape(-1), c.rgb.reshape(-1)]
        parts += part
        sizes.append([int(p.numel()) for p in part])
    host = torch.cat(parts).cpu().numpy()                                    # the one host read
    written, o = [], 0
    for j, (c, sz) in enumerate(zip(crops, sizes)):
        counts = host[o:o + sz[0]].view(np.int32)
        lat = host[o + sz[0]:o + sz[0] + sz[1]].view(np.float32)
        shape = tuple(c.uvw.shape)
        uvw = host[o + sz[0] + sz[1]:o + sz[0] + sz[1] + sz[2]].reshape(shape)
        rgb = host[o + sum(sz[:3]):o + sum(sz)].reshape(shape)
        o += sum(sz)
        n, covered, visible, flags = (int(x) for x in counts)
        if n == 0 or visible == 0 or (flags & 2):
            continue
        if only_ok and not verdicts[j]['ok']:
            continue
        if not float(visible) / float(covered) >= float(min_visible):
            continue
        writer.add(Crop(uvw, rgb, c.box, c.window, counts, flags), lat, c.intrinsics, c.extrinsics, box=[int(x) for x in c.box],
                   covered=covered, visible=visible)
        written.append(j)
    return written
