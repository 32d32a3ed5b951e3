"""Train a DeepSDF shape prior on the device from a folder of SDF samples (the .npz files of tools/mesh_to_sdf.py).

Writes <out>.pt + <out>.json (what setup_dsdf loads) and <out>_latents.pt, then prints prior_residuals per shape.  The hyper-parameters are
DeepSDF's as recalled (sdflabel_amd/pipelines/train_prior.py); dropout is the library's own random stream.

usage: python tools/train_prior.py SAMPLES_DIR --out prior/deepsdf [--epochs 100] [--latent 3] [--width 512] [--layers 8] [--raw-latents]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("samples", help="folder of .npz files (pos / neg), one per shape")
    ap.add_argument("--out", required=True, help="path stem of the three files written")
    ap.add_argument("--epochs", type=int, default=100)
    ap.add_argument("--latent", type=int, default=3)
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--layers", type=int, default=8)
    ap.add_argument("--shapes-per-batch", type=int, default=8)
    ap.add_argument("--samples-per-shape", type=int, default=2048)
    ap.add_argument("--raw-latents", action="store_true", help="DeepSDF's raw latents with the regulariser instead of unit latents")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device", default="cuda")
    args = ap.parse_args()

    from sdflabel_amd.deepsdf.workspace import setup_dsdf
    from sdflabel_amd.pipelines.train_prior import default_specs, load_samples, train_prior
    from sdflabel_amd.sdf_samples import prior_residuals

    specs = default_specs(args.latent, (args.width,) * args.layers, (args.layers // 2,) if args.layers >= 2 else ())
    samples, files = load_samples(args.samples, args.device)

    def log(ep, loss):
        if ep % 10 == 0 or ep == args.epochs - 1:
            print("epoch %d loss %.6f" % (ep, float(loss)), flush=True)

    tr = train_prior(samples, specs, epochs=args.epochs, shapes_per_batch=args.shapes_per_batch, samples_per_shape=args.samples_per_shape,
                     device=args.device, unit_latents=not args.raw_latents, seed=args.seed, log=log)
    pt = tr.save(args.out)
    print("saved", pt)
    dsdf, _ = setup_dsdf(pt, precision=torch.float32)
    dsdf.to(args.device)
    l1, agree = prior_residuals(dsdf, tr.decoder_latents(), samples)
    for f, a, b in zip(files, l1.tolist(), agree.tolist()):
        print("%s clamped_l1 %.6f sign_agreement %.4f" % (os.path.basename(f), a, b))


if __name__ == "__main__":
    main()
