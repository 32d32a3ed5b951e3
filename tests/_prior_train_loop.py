"""The prior-training loop in plain torch ops on the CPU (any dtype), for the trajectory and end-to-end tests of
tests/test_gpu_prior_train.py: the same decoder, initial state, batches, loss and Adam groups as PriorTrainer, the decoder's forward
written out with torch ops under torch's autograd (and torch's own dropout stream where dropout is on).
"""
import copy

import numpy as np
import torch

from sdflabel_amd.deepsdf.networks.deep_sdf_decoder_scale import Decoder
from sdflabel_amd.pipelines.train_prior import PriorTrainer, clamped_l1, default_specs, effective_weights

SPECS = default_specs(3, (128,) * 3, (2,))


def analytic_rows(n_per=256, seed=5):
    """4 analytic shapes (two spheres, two boxes) x n_per points uniform in the cube: rows float32 [4 n_per][4], shapes int64 [4]"""
    rng = np.random.default_rng(seed)
    rows = []
    for s in range(4):
        p = rng.uniform(-1, 1, (n_per, 3))
        if s < 2:
            d = np.linalg.norm(p, axis=1) - (0.45, 0.7)[s]
        else:
            q = np.abs(p) - np.array(((0.5, 0.3, 0.6), (0.3, 0.7, 0.4))[s - 2])
            d = np.linalg.norm(np.maximum(q, 0), axis=1) + np.minimum(q.max(1), 0)
        rows.append(np.concatenate([p, d[:, None]], 1))
    return torch.from_numpy(np.concatenate(rows).astype(np.float32)), torch.arange(4)


def plain_forward(decoder, inputs, drop_p=0.0):
    """Decoder.forward's SDF output with torch ops, dropout (torch's stream) on the layers of decoder.dropout when drop_p > 0"""
    Ws, bs = effective_weights(decoder)
    inj = decoder._inject_table()
    n = len(Ws) - 1
    x = inputs
    for l in range(n + 1):
        if inj[l][0]:
            x = torch.cat([x, inputs[:, inj[l][1]:inj[l][1] + inj[l][0]]], 1)
        x = x @ Ws[l].t() + bs[l]
        if l == n and decoder.use_tanh:
            x = torch.tanh(x)
        if l < n:
            x = torch.relu(x)
            if drop_p > 0 and decoder.dropout is not None and l in decoder.dropout:
                x = torch.nn.functional.dropout(x, p=drop_p, training=True)
    return torch.tanh(x)


def torch_loop(trainer0, batches, dtype, drop_p=0.0, torch_seed=0):
    """run the steps of `batches` ([(shapes, rows)]) from the initial state of the (untouched, CPU) PriorTrainer `trainer0`.
    Returns (losses float64 [steps], final latents, final decoder state dict)."""
    dec = Decoder(int(trainer0.specs["CodeLength"]), **trainer0.specs["NetworkSpecs"])
    dec.load_state_dict(copy.deepcopy(trainer0.decoder.state_dict()))
    dec.to(dtype)
    lat = trainer0.latents.detach().clone().to(dtype).requires_grad_(True)
    h = trainer0.h
    params = [p for n, p in dec.named_parameters() if not n.startswith("scale_net")]
    opt = torch.optim.Adam([{"params": params, "lr": h["lr_decoder"]}, {"params": [lat], "lr": h["lr_latents"]}])
    torch.manual_seed(torch_seed)
    losses = []
    for shapes, rows in batches:
        rows = rows.to(dtype)
        k = rows.shape[0] // shapes.shape[0]
        z = lat[shapes]
        zn = z / z.norm(dim=1, keepdim=True) if trainer0.unit_latents else z
        inputs = torch.cat([zn.repeat_interleave(k, 0), rows[:, :3]], 1)
        pred = plain_forward(dec, inputs, drop_p)[:, 0]
        loss = clamped_l1(pred, rows[:, 3], float(h["clamp"]))
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return np.array(losses), lat.detach(), {k: v.detach() for k, v in dec.state_dict().items()}


def fresh_trainer(device, n_shapes=4, seed=3, **hyper):
    return PriorTrainer(SPECS, n_shapes, device, seed=seed, **hyper)
