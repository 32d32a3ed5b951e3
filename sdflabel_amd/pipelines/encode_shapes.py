"""Encode a folder of shapes under a trained prior: the second half of the auto-decoder, for shapes the prior was not trained on.

    encode_folder("prior/deepsdf.pt", "held_out_samples/", "prior/held_out")     ->  prior/held_out_latents.pt

The prior is what pipelines.train_prior saved (or any .pt/.json pair setup_dsdf loads); the samples are the .npz files tools/mesh_to_sdf.py
writes.  The fit is sdflabel_amd.encode.encode_many; its defaults are DeepSDF's reconstruction settings as recalled (see there).
"""
import os

import torch

from ..deepsdf.workspace import setup_dsdf
from ..encode import encode_many
from .train_prior import load_samples


def encode_folder(prior_path, samples_dir, out_path, device="cuda", precision=torch.float32, **kw):
    """Load the prior with setup_dsdf, read the folder's .npz files (sorted by name) and fit one latent per file with encode_many(**kw).
    Writes <out>_latents.pt with the keys of PriorTrainer.save -- "latents" (as the decoder sees them), "raw_latents", "unit_latents" -- plus
    "files", "loss" and "flags" (encode.Encoded), all on the host.  Returns the path written."""
    dsdf, _ = setup_dsdf(prior_path, precision=precision)
    dsdf = dsdf.to(device).eval()
    samples, files = load_samples(str(samples_dir), device)
    enc = encode_many(dsdf, samples, **kw)
    out = os.path.splitext(str(out_path))[0] + "_latents.pt"
    torch.save({"latents": enc.latents.detach().cpu(), "raw_latents": enc.raw_latents.detach().cpu(), "unit_latents": bool(enc.unit_latents),
                "files": list(files), "loss": enc.loss.detach().cpu(), "flags": enc.flags.detach().cpu()}, out)
    return out
