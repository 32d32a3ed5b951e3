"""GPU timing of the training-crop export (sdflabel_amd/export.py) beside the verification on the same inputs.

crops_many   launches, copies, host synchronisations and device time (device events round the call) of export.crops_many, with the
             occlusion on and off; the raster it contains is verify's own
verify_many  the same figures of verify.verify_many on the same meshes, boxes and clouds (host clock: it ends with its one host read)
writer       CropWriter.add per crop: the download and the two PNG encodings (host clock), into a temporary folder
cases        B = 1 / 16 annotations: verify_time.py's shapes (the synthetic decoder in its float16 mode, meshed at R = 64, 3 - 30 m in front of
             a KITTI-sized camera, 1242 x 375, f = 720), each with its projected box as the label and a constant colour crop
Medians of REPS repetitions after WARM warm-up runs.

usage: python tools/export_time.py OUT_DIR          (writes OUT_DIR/export_time.json)
"""
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import sdflabel_amd  # noqa: E402
from sdflabel_amd import export as E  # noqa: E402
from sdflabel_amd import mesh as M  # noqa: E402
from sdflabel_amd import verify as V  # noqa: E402
from sdflabel_amd.fixtures import ASSET  # noqa: E402
from tests import _verify_ref as VR  # noqa: E402
from tools.frame_time import count_launches, count_syncs  # noqa: E402
from tools.verify_time import DEV, NPTS, REPS, WARM, F, H, K, W, event_ms, host_ms, problem  # noqa: E402


def main():
    out_dir = sys.argv[1] if len(sys.argv) > 1 else "."
    os.makedirs(out_dir, exist_ok=True)
    dec = sdflabel_amd.setup_dsdf(ASSET + ".pt", precision=torch.float16)[0].to(DEV)
    res = {"config": "deepsdf_synth (8 x 512, latent 3) in its float16 mode; meshes at R = 64; image %d x %d, f = %g; %d points per annotation; "
                     "device events on the current stream for crops_many, host clock for verify_many and the writer; WARM %d, REPS %d, medians"
                     % (W, H, F, NPTS, WARM, REPS),
           "cases": {}}
    size = (W, H)
    for B in (1, 16):
        params = problem(B)
        meshes = [m.to_camera() for m in M.meshes_many(dec, params, resolution=64)]
        boxes, clouds, colors = [], [], []
        rng = np.random.default_rng(B)
        for m in meshes:
            v = m.vertices_numpy()
            u, w = VR.project(F, K[0, 2], v[:, 0], v[:, 2]), VR.project(F, K[1, 2], v[:, 1], v[:, 2])
            boxes.append([float(np.floor(u.min())), float(np.floor(w.min())), float(np.ceil(u.max())), float(np.ceil(w.max()))])
            clouds.append(m.vertices[torch.from_numpy(rng.choice(len(v), NPTS, replace=len(v) < NPTS)).to(DEV)].contiguous())
            colors.append(torch.full((int(boxes[-1][3] - boxes[-1][1]), int(boxes[-1][2] - boxes[-1][0]), 3), 0.5, device=DEV))
        crops = lambda occ=True: E.crops_many(meshes, K, boxes, size, colors=colors, occlusion=occ)          # noqa: E731
        verify = lambda: V.verify_many(dec, params, meshes, clouds, K, boxes, size)                          # noqa: E731
        got = crops()
        verify()
        kl, cp = count_launches(crops)
        vkl, vcp = count_launches(verify)
        counts = torch.stack([c.counts for c in got]).cpu().numpy()
        entry = {"crops_many_ms": round(event_ms(crops), 4), "crops_many_occlusion_off_ms": round(event_ms(lambda: crops(False)), 4),
                 "crops_many_host_ms": round(host_ms(crops), 4),
                 "kernel_launches": kl, "copies": cp, "host_synchronisations": count_syncs(crops),
                 "verify_many_ms": round(host_ms(verify), 4), "verify_many_kernel_launches": vkl, "verify_many_copies": vcp,
                 "verify_many_host_synchronisations": count_syncs(verify),
                 "triangles": int(sum(len(m) for m in meshes)), "window_pixels": int(sum((c.window[2] - c.window[0]) * (c.window[3] - c.window[1]) for c in got)),
                 "box_pixels": int(counts[:, 0].sum()), "covered": int(counts[:, 1].sum()), "visible": int(counts[:, 2].sum())}
        with tempfile.TemporaryDirectory() as tmp:
            usable = [(c, p) for c, p in zip(got, params) if c.uvw.numel()]
            ts = []
            with E.CropWriter(tmp) as writer:
                for _ in range(3):
                    for c, p in usable:
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        writer.add(c, p["latent"], K, np.eye(4))
                        ts.append((time.perf_counter() - t0) * 1e3)
            entry["writer_add_ms_per_crop"] = round(float(np.median(ts)), 4)
            entry["writer_crops"] = len(usable)
        res["cases"]["B%d" % B] = entry
        print("B=%d" % B, json.dumps(entry), flush=True)
    json.dump(res, open(os.path.join(out_dir, "export_time.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
