"""Training the DeepSDF shape prior on the device: an auto-decoder (decoder weights plus one latent per shape) fitted to SDF samples, the
first arrow of the loop  fit decoder -> synthetic crops -> train_css -> refine_sample -> verify -> export -> train again.

The three GEMM passes of the decoder run in csrc/mlp_train.hip (deepsdf/train.py: decoder_train); the weight-norm fold, the latent
expansion (its backward is a segmented sum in fixed order, no atomics), the loss and Adam are torch ops.

THE HYPER-PARAMETERS ARE DeepSDF's AS RECALLED -- clamp 0.1, learning rates 5e-4 (decoder) and 1e-3 (latents) halved on a step schedule,
latent regulariser 1e-4 ramped in over the first epochs, dropout 0.2 on every hidden layer, latents drawn from N(0, 1/L).  They are
parameters; they have not been checked against that paper's code.  Dropout uses the library's own random stream (an integer hash of seed,
layer, row and feature), not torch's.

unit_latents=True (the default here): the decoder is fed z / ||z||, because the refinement normalises the latent before the decoder
(pipelines/optimizer.py) and the CSS head projects its latent onto the unit sphere; the regulariser is then off.  unit_latents=False gives
DeepSDF's raw latents.  scale_net gets no gradient from this loss and keeps its initial values.
"""
import glob
import json
import os

import torch

from .. import _lib
from ..deepsdf.networks.deep_sdf_decoder_scale import Decoder
from ..deepsdf.train import TrainDesc, decoder_train, expand_latents
from ..sdf_samples import SdfSamples

DEFAULTS = dict(clamp=0.1, lr_decoder=5e-4, lr_latents=1e-3, lr_step=500, lr_factor=0.5, code_reg=1e-4, code_reg_ramp=100, drop_p=0.2)


def default_specs(latent_size=3, dims=(512,) * 8, latent_in=(4,)):
    n = len(dims)
    return {"Description": "shape prior trained by sdflabel_amd.pipelines.train_prior", "NetworkArch": "deep_sdf_decoder_scale",
            "CodeLength": int(latent_size),
            "NetworkSpecs": {"dims": list(dims), "dropout": list(range(n)), "dropout_prob": 0.2, "norm_layers": list(range(n)),
                             "latent_in": list(latent_in), "xyz_in_all": False, "use_tanh": False, "latent_dropout": False,
                             "weight_norm": True}}


def effective_weights(decoder):
    """[W_l], [b_l] of the decoder under autograd: W = v (g / ||v||_row) as nn.utils.weight_norm folds it, or the plain weight"""
    Ws, bs = [], []
    for l in range(decoder.num_layers - 1):
        lin = getattr(decoder, "lin" + str(l))
        if hasattr(lin, "weight_v"):
            v, g = lin.weight_v, lin.weight_g
            Ws.append(v * (g / v.norm(2, dim=1, keepdim=True)))
        else:
            Ws.append(lin.weight)
        bs.append(lin.bias)
    return Ws, bs


def clamped_l1(pred, sdf, clamp):
    return (pred.clamp(-clamp, clamp) - sdf.clamp(-clamp, clamp)).abs().mean()


class PriorTrainer:
    """Owns an sdflabel_amd Decoder built from `specs` (the reference's parameter names, scale_net included, so the saved state loads
    strictly), the latents [n_shapes][CodeLength] and two Adam groups.  See the module docstring for the hyper-parameters."""

    def __init__(self, specs, n_shapes, device, unit_latents=True, seed=0, **hyper):
        unknown = set(hyper) - set(DEFAULTS)
        if unknown:
            raise TypeError("PriorTrainer: unknown hyper-parameters %s" % sorted(unknown))
        self.h = dict(DEFAULTS, **hyper)
        self.specs = specs
        self.device = torch.device(device)
        self.unit_latents = bool(unit_latents)
        self.seed = int(seed)
        L = int(specs["CodeLength"])
        net = dict(specs["NetworkSpecs"])
        net.pop("samples_per_scene", None)
        gen = torch.Generator().manual_seed(self.seed)
        state = torch.random.get_rng_state()
        torch.manual_seed(self.seed)
        try:
            self.decoder = Decoder(L, **net)
        finally:
            torch.random.set_rng_state(state)
        self.decoder.to(self.device).train()
        self.desc = TrainDesc.from_decoder(self.decoder)
        # the specs' dropout_prob unless the caller passes drop_p; 0 when no layer is listed
        self.h["drop_p"] = float(hyper.get("drop_p", net.get("dropout_prob", DEFAULTS["drop_p"])))
        self.drop_p = self.h["drop_p"] if self.desc.drop_layers else 0.0
        self.latents = (torch.randn((int(n_shapes), L), generator=gen) * (1.0 / L) ** 0.5).to(self.device).requires_grad_(True)
        self.dec_params = [p for n, p in self.decoder.named_parameters() if not n.startswith("scale_net")]
        self.opt = torch.optim.Adam([{"params": self.dec_params, "lr": self.h["lr_decoder"]},
                                     {"params": [self.latents], "lr": self.h["lr_latents"]}])
        self.steps = 0
        self.epoch = 0

    def decoder_latents(self):
        """the latents as the decoder sees them (normalised with unit_latents): what meshes_many, prior_residuals and the refinement take"""
        z = self.latents.detach()
        return z / z.norm(dim=1, keepdim=True) if self.unit_latents else z

    def loss(self, shapes, rows):
        """shapes int64 [S] (indices of the batch's shapes), rows float32 [S * k][4] = x y z sdf, the k samples of each shape contiguous"""
        S = int(shapes.shape[0])
        k = rows.shape[0] // S
        if S * k != rows.shape[0]:
            raise _lib.SdfrError("PriorTrainer: a batch holds the same number of samples of each of its shapes (got %d rows for %d shapes)"
                                 % (rows.shape[0], S))
        z = self.latents[shapes]
        zn = z / z.norm(dim=1, keepdim=True) if self.unit_latents else z
        inputs = torch.cat([expand_latents(zn, k), rows[:, :3]], 1)
        Ws, bs = effective_weights(self.decoder)
        pred = decoder_train(inputs, Ws, bs, self.desc, self.drop_p, self.seed * 1000003 + self.steps)[:, 0]
        loss = clamped_l1(pred, rows[:, 3], float(self.h["clamp"]))
        if not self.unit_latents and self.h["code_reg"] > 0:
            ramp = min(1.0, (self.epoch + 1) / float(max(self.h["code_reg_ramp"], 1)))
            loss = loss + self.h["code_reg"] * ramp * z.norm(dim=1).mean()
        return loss

    def step(self, batch):
        """one Adam step on batch = (shapes, rows); returns the loss (a 0-d device tensor: no host read)"""
        shapes, rows = batch
        factor = self.h["lr_factor"] ** (self.epoch // max(int(self.h["lr_step"]), 1))
        self.opt.param_groups[0]["lr"] = self.h["lr_decoder"] * factor
        self.opt.param_groups[1]["lr"] = self.h["lr_latents"] * factor
        self.opt.zero_grad(set_to_none=True)
        loss = self.loss(shapes.to(self.device), rows.to(self.device).float())
        loss.backward()
        self.opt.step()
        self.steps += 1
        return loss.detach()

    def save(self, path):
        """<path>.pt ({"epoch", "model_state_dict"} with the DataParallel 'module.' prefix), <path>.json (the specs setup_dsdf reads) and
        <path>_latents.pt ({"latents" as the decoder sees them, "raw_latents", "unit_latents"})"""
        path = os.path.splitext(path)[0]
        state = {"module." + k: v.detach().cpu() for k, v in self.decoder.state_dict().items()}
        torch.save({"epoch": self.epoch, "model_state_dict": state}, path + ".pt")
        with open(path + ".json", "w") as f:
            json.dump(self.specs, f, indent=1)
        torch.save({"latents": self.decoder_latents().cpu(), "raw_latents": self.latents.detach().cpu(), "unit_latents": self.unit_latents},
                   path + "_latents.pt")
        return path + ".pt"


def load_samples(samples, device=None):
    """a list of SdfSamples, or a folder of .npz files as tools/mesh_to_sdf.py writes them (sorted by name)"""
    if isinstance(samples, str):
        files = sorted(glob.glob(os.path.join(samples, "*.npz")))
        if not files:
            raise FileNotFoundError("train_prior: no .npz files in %s" % samples)
        return [SdfSamples.load(f, device) for f in files], files
    samples = list(samples)
    return samples, [str(i) for i in range(len(samples))]


def draw_batch(samples, shapes, k, generator, device):
    """(shapes, rows [len(shapes) * k][4]): k rows of every listed shape, drawn with replacement from the host generator"""
    rows = []
    for s in shapes.tolist():
        r = samples[s].rows
        idx = torch.randint(0, r.shape[0], (k,), generator=generator)
        rows.append(r[idx.to(r.device)].to(device))
    return shapes.to(device), torch.cat(rows).float()


def train_prior(samples, specs=None, epochs=100, shapes_per_batch=None, samples_per_shape=2048, device="cuda", unit_latents=True, seed=0,
                log=None, **hyper):
    """Fit a decoder and one latent per shape to `samples` (a list of SdfSamples or a folder of .npz files).  An epoch visits every shape
    once, shapes_per_batch at a time (default: all, at most 8), samples_per_shape rows each.  Returns the PriorTrainer; call .save(path)."""
    samples, _ = load_samples(samples, device)
    S = len(samples)
    specs = specs or default_specs()
    tr = PriorTrainer(specs, S, device, unit_latents=unit_latents, seed=seed, **hyper)
    gen = torch.Generator().manual_seed(int(seed) + 1)
    per = min(S, int(shapes_per_batch or 8))
    last = None
    for ep in range(int(epochs)):
        tr.epoch = ep
        order = torch.randperm(S, generator=gen)
        for i in range(0, S - per + 1, per):
            last = tr.step(draw_batch(samples, order[i:i + per], int(samples_per_shape), gen, tr.device))
        if log is not None and last is not None:
            log(ep, last)
    tr.epoch = int(epochs)
    return tr
