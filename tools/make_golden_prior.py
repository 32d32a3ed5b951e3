"""Record golden G23 (tests/golden/g23_prior_train.npz) from the REFERENCE's own Decoder class in train() mode (runs in the build container
only; the class is imported, never copied): L = 3, dims [128] * 4, latent_in [2], weight-norm on every layer, dropout_prob 0, .double().

Four shapes x 24 rows: inputs = cat(latents[shape], xyz), loss = mean |clamp(pred, +-0.1) - clamp(target, +-0.1)|.  Recorded: the state
dict (float32-exact values), latents, xyz, target, sdf (the decoder's output), loss, and the float64 gradient of every parameter
(weight_g, weight_v, bias), of the inputs and of the latents.  Data only.

usage: python tools/make_golden_prior.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _ref_import  # noqa: E402

_ref_import.setup()

import numpy as np  # noqa: E402
import torch  # noqa: E402

SPEC = dict(dims=[128] * 4, dropout=[0, 1, 2, 3], dropout_prob=0.0, norm_layers=[0, 1, 2, 3, 4], latent_in=[2], xyz_in_all=False,
            use_tanh=False, latent_dropout=False, weight_norm=True)
S, K, L = 4, 24, 3


def main():
    from deepsdf.networks.deep_sdf_decoder_scale import Decoder  # the reference class
    torch.manual_seed(23)
    dec = Decoder(L, **SPEC)
    with torch.no_grad():
        dec.lin4.weight_g.mul_(0.25)                      # keeps most predictions inside the clamp, where the loss has a gradient
    dec = dec.double().train()
    gen = torch.Generator().manual_seed(2323)
    latents = (torch.randn(S, L, generator=gen) * (1.0 / L) ** 0.5).float().double().requires_grad_(True)
    xyz = (torch.rand(S * K, 3, generator=gen) * 2 - 1).float().double()
    target = (torch.randn(S * K, generator=gen) * 0.08).float().double()
    inputs = torch.cat([latents.repeat_interleave(K, 0), xyz], 1)
    inputs.retain_grad()
    pred, _ = dec(inputs)
    pred = pred[:, 0]
    loss = (pred.clamp(-0.1, 0.1) - target.clamp(-0.1, 0.1)).abs().mean()
    loss.backward()
    out = {"latents": latents.detach().numpy(), "xyz": xyz.numpy(), "target": target.numpy(), "sdf": pred.detach().numpy(),
           "loss": np.float64(loss.item()), "g_inputs": inputs.grad.numpy(), "g_latents": latents.grad.numpy(),
           "S": np.int64(S), "K": np.int64(K)}
    for name, p in dec.named_parameters():
        v = p.detach().numpy()
        assert np.array_equal(v.astype(np.float32).astype(np.float64), v), name
        out["state." + name] = v.astype(np.float32)
        if p.grad is not None:
            out["grad." + name] = p.grad.numpy()
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "g23_prior_train.npz")
    np.savez_compressed(path, **out)
    live = int((pred.detach().abs() < 0.1).sum())
    print("saved", os.path.abspath(path), os.path.getsize(path), "bytes; rows inside the clamp:", live, "of", S * K)


if __name__ == "__main__":
    main()
