"""Encode a folder of SDF samples (the .npz files of tools/mesh_to_sdf.py) under a trained shape prior: one latent per file, the decoder frozen.

Writes <out>_latents.pt ("latents" as the decoder sees them, "raw_latents", "unit_latents", "files", "loss", "flags") and prints the loss per
shape.  The defaults are DeepSDF's reconstruction settings as recalled (sdflabel_amd/encode.py); the rows are drawn from the library's own
random stream.

usage: python tools/encode_shapes.py PRIOR.pt SAMPLES_DIR --out prior/held_out [--iters 800] [--rows 8000] [--lr 5e-3] [--raw-latents] [--half]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("prior", help="the .pt of a prior (its .json next to it), as tools/train_prior.py writes them")
    ap.add_argument("samples", help="folder of .npz files (pos / neg), one per shape")
    ap.add_argument("--out", required=True, help="path stem; <out>_latents.pt is written")
    ap.add_argument("--iters", type=int, default=800)
    ap.add_argument("--rows", type=int, default=8000, help="rows per shape and iteration")
    ap.add_argument("--lr", type=float, default=5e-3)
    ap.add_argument("--raw-latents", action="store_true", help="DeepSDF's raw latents with the regulariser instead of unit latents")
    ap.add_argument("--half", action="store_true", help="the float16 decoder kernels")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device", default="cuda")
    args = ap.parse_args()

    from sdflabel_amd.pipelines.encode_shapes import encode_folder

    out = encode_folder(args.prior, args.samples, args.out, device=args.device, precision=torch.float16 if args.half else torch.float32,
                        iters=args.iters, rows_per_iter=args.rows, lr=args.lr, unit_latents=not args.raw_latents, seed=args.seed)
    d = torch.load(out)
    print("saved", out)
    for f, loss, fl in zip(d["files"], d["loss"].tolist(), d["flags"].tolist()):
        print("%s clamped_l1 %.6f flags %d" % (os.path.basename(f), loss, fl))


if __name__ == "__main__":
    main()
