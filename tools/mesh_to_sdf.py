"""Triangle meshes in, DeepSDF training samples out: for every PLY / OBJ file an .npz with `pos` and `neg` rows x y z sdf
(sdflabel_amd/sdf_samples.py: fit_frame, normalize, draw_sdf_samples, SdfSamples.save).

usage: python tools/mesh_to_sdf.py [--out DIR] [--n 500000] [--frame unit_sphere|unit_cube|none] [--buffer 1.03] [--seed 0] [--unsigned]
                                   [--batch 8] MESH [MESH ...]

--frame      how a model is brought into the lattice frame before sampling (none: the file's coordinates are used as they are)
--unsigned   the unsigned distance, for open meshes (everything lands in `pos`)
The sampling shares and widths are draw_sdf_samples' defaults: DeepSDF's as recalled, not checked against that paper's code.
Each output also gets a line on stdout with the mesh's flags (bit 0: non-finite vertices skipped, bit 1: invalid faces or no area), the
number of inside samples and the frame that was applied.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from sdflabel_amd import sdf_samples as S  # noqa: E402
from sdflabel_amd.mesh import Mesh, load_obj, load_ply  # noqa: E402


def load(path):
    low = path.lower()
    if low.endswith(".ply"):
        v, _, f = load_ply(path)
    elif low.endswith(".obj"):
        v, _, f = load_obj(path)
    else:
        raise SystemExit("mesh_to_sdf: %s is neither .ply nor .obj" % path)
    return v, f


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("meshes", nargs="+")
    ap.add_argument("--out", default=".")
    ap.add_argument("--n", type=int, default=500000)
    ap.add_argument("--frame", default="unit_sphere", choices=("unit_sphere", "unit_cube", "none"))
    ap.add_argument("--buffer", type=float, default=1.03)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--unsigned", action="store_true")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)
    os.makedirs(a.out, exist_ok=True)
    g = torch.Generator().manual_seed(a.seed)
    mode = None if a.frame == "none" else a.frame
    for i0 in range(0, len(a.meshes), max(1, a.batch)):
        paths = a.meshes[i0:i0 + max(1, a.batch)]
        meshes, frames = [], []
        for p in paths:
            v, f = load(p)
            centre, scale = S.fit_frame(v, mode, a.buffer)
            frames.append((centre, scale))
            meshes.append(Mesh(torch.from_numpy(S.normalize(v, centre, scale)).to(a.device), torch.from_numpy(np.ascontiguousarray(f)).to(a.device)))
        for p, s, (centre, scale) in zip(paths, S.draw_sdf_samples(meshes, n=a.n, generator=g, want_sign=not a.unsigned), frames):
            dst = os.path.join(a.out, os.path.splitext(os.path.basename(p))[0] + ".npz")
            s.save(dst)
            rows = s.numpy()
            print(json.dumps({"mesh": p, "npz": dst, "samples": len(s), "inside": int((rows[:, 3] < 0).sum()), "flags": int(s.flags.cpu()),
                              "centre": [float(c) for c in centre], "scale": float(scale)}), flush=True)


if __name__ == "__main__":
    main()
