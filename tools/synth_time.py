"""GPU timing of the synthetic bootstrap crops (sdflabel_amd/synth.py) beside the training-crop export on the same meshes and boxes.

launches     device time of the two new entry points, sdfr_synth_owner and sdfr_synth_shade, on the buffers of a scenes_many call (device
             events round each call)
scenes_many  the whole call with the meshes at hand (host clock: it contains its one host read), its launches, copies and host
             synchronisations; the same with the meshes made inside (mesh.meshes_many's launches and host reads added)
crops_many   export.crops_many on the same camera-frame meshes and crop boxes, for comparison (device events)
restatement  tests/_synth_ref.render of one scene (numpy, host clock, one run)
bootstrap    crops per second of pipelines.synth_crops.bootstrap_crops into a temporary folder (host clock, PNG encoding included)
cases        1 scene x 1 object and 8 scenes x 2 objects of synth.draw_scenes' defaults: the synthetic decoder in its float16 mode meshed at
             R = 64, a KITTI-sized camera (1242 x 375, f = 720)
Medians of REPS repetitions after WARM warm-up runs.

usage: python tools/synth_time.py OUT_DIR          (writes OUT_DIR/synth_time.json)
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
from sdflabel_amd import synth  # noqa: E402
from sdflabel_amd.fixtures import ASSET  # noqa: E402
from sdflabel_amd.pipelines.synth_crops import bootstrap_crops  # noqa: E402
from tests import _synth_ref as SR  # noqa: E402
from tools.frame_time import count_launches, count_syncs  # noqa: E402
from tools.verify_time import DEV, REPS, WARM, F, H, K, W, event_ms, host_ms, problem  # noqa: E402


def scenes_with(n_scenes, n_objects, n_latents):
    """the first n_scenes scenes of seed 0 that hold exactly n_objects objects"""
    out, first = [], 0
    while len(out) < n_scenes:
        out += [s for s in synth.draw_scenes(torch.Generator().manual_seed(0), 16, n_latents, K, (W, H), first_scene=first, max_objects=3)
                if len(s["objects"]) == n_objects]
        first += 16
    return out[:n_scenes]


def main():
    out_dir = sys.argv[1] if len(sys.argv) > 1 else "."
    os.makedirs(out_dir, exist_ok=True)
    dec = sdflabel_amd.setup_dsdf(ASSET + ".pt", precision=torch.float16)[0].to(DEV)
    latents = torch.stack([p["latent"] for p in problem(16)])
    size = (W, H)
    res = {"config": "deepsdf_synth (8 x 512, latent 3) in its float16 mode; meshes at R = 64; image %d x %d, f = %g; draw_scenes' default ranges, "
                     "seed 0; device events on the current stream for single entry points and crops_many, host clock for scenes_many, the "
                     "restatement and bootstrap_crops; WARM %d, REPS %d, medians" % (W, H, F, WARM, REPS),
           "cases": {}}
    for n_scenes, n_objects in ((1, 1), (8, 2)):
        scenes = scenes_with(n_scenes, n_objects, len(latents))
        meshes = synth.scene_meshes(dec, latents, scenes, resolution=64)
        launches = {}
        render = lambda: synth.scenes_many(dec, latents, scenes, K, size, resolution=64, meshes=meshes)          # noqa: E731
        whole = lambda: synth.scenes_many(dec, latents, scenes, K, size, resolution=64)                          # noqa: E731
        crops, report = synth.scenes_many(dec, latents, scenes, K, size, resolution=64, meshes=meshes, _launches=launches)
        kl, cp = count_launches(render)
        wkl, wcp = count_launches(whole)
        counts = torch.stack([c.counts for c in crops]).cpu().numpy()
        kept = [i for i, (si, oi, _) in enumerate(synth._objects(scenes)) if (scenes[si]["index"], oi) in report["kept"]]
        cam = [meshes[0][i] for i in kept]
        boxes = [list(c.box) for c in crops]
        export = lambda: E.crops_many(cam, K, boxes, size)                                                      # noqa: E731
        export()
        entry = {"scenes": n_scenes, "objects": n_scenes * n_objects, "crops": len(crops),
                 "sdfr_synth_owner_ms": round(event_ms(launches["owner"]), 4), "sdfr_synth_shade_ms": round(event_ms(launches["shade"]), 4),
                 "scenes_many_ms": round(host_ms(render), 4), "kernel_launches": kl, "copies": cp, "host_synchronisations": count_syncs(render),
                 "scenes_many_with_meshes_made_inside_ms": round(host_ms(whole), 4), "with_meshes_kernel_launches": wkl, "with_meshes_copies": wcp,
                 "with_meshes_host_synchronisations": count_syncs(whole),
                 "crops_many_same_meshes_and_boxes_ms": round(event_ms(export), 4), "crops_many_host_ms": round(host_ms(export), 4),
                 "triangles": int(sum(len(m) for m in meshes[0])), "window_pixels": int(launches["window_pixels"]),
                 "box_pixels": int(launches["box_pixels"]), "covered": int(counts[:, 1].sum()), "visible": int(counts[:, 2].sum())}
        if n_scenes == 1:
            objs = [o for s in scenes for o in s["objects"]]
            m = meshes[0]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            SR.render([(x.vertices_numpy(), x.faces_numpy()) for x in m], [x.normals_numpy() for x in m], (F, F, K[0, 2], K[1, 2]),
                      [c.window for c in crops], [c.box for c in crops], size,
                      np.array([o["albedo"] + [o["ks"], o["shin"]] for o in objs], np.float64),
                      np.array([s["light"] + [s["ambient"], s["kd"]] for s in scenes], np.float64), np.array([s["ramp"] for s in scenes], np.int32),
                      [0] * len(objs))
            entry["numpy_restatement_one_scene_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        res["cases"]["%dx%d" % (n_scenes, n_objects)] = entry
        print("%d x %d" % (n_scenes, n_objects), json.dumps(entry), flush=True)
    with tempfile.TemporaryDirectory() as tmp:
        n = 48
        bootstrap_crops(dec, latents, os.path.join(tmp, "warm"), 8, K, size, seed=1, batch_scenes=8)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        bootstrap_crops(dec, latents, os.path.join(tmp, "crops"), n, K, size, seed=0, batch_scenes=8)
        dt = time.perf_counter() - t0
        res["bootstrap_crops"] = {"crops": n, "batch_scenes": 8, "seconds": round(dt, 3), "crops_per_second": round(n / dt, 2),
                                  "note": "host clock, one run: drawing, meshing at R = 64, rendering, the downloads and the PNG encoding"}
        print("bootstrap_crops", json.dumps(res["bootstrap_crops"]), flush=True)
    json.dump(res, open(os.path.join(out_dir, "synth_time.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
