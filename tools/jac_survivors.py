"""Survivor fractions and padded K extents of the band Jacobian's K compaction, on the CPU: python tools/jac_survivors.py [crop index]
A torch forward of the fixture decoder on the 40^3 grid with the bench's start latent of the crop (normalised), the ReLU masks x > 0 of
every hidden layer, the band |sdf| < 0.03 in grid order cut into consecutive tiles of 16 rows, as the 16-row kernel takes them, and per
layer: features alive in a single row, alive in at least one row of a tile (mean, worst tile), and the K extent the compacted product of
that mask runs (survivors padded to whole trips of 64, at least one; csrc/kcj_slots.h) as a share of the full chain's 512."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import torch.nn.functional as F

from oracle.torch_cpu_port import DecoderPort, generate_point_grid
from sdflabel_amd.fixtures import crop_start, fitted_state

D, THR, TILE, TRIP = 40, 0.03, 16, 64


def main():
    crop = int(sys.argv[1]) if len(sys.argv) > 1 else 0
    st, spec = fitted_state()
    dec = DecoderPort(st, spec).eval()
    lat = torch.from_numpy(crop_start(crop)[2])
    lat = F.normalize(lat, p=2, dim=0)
    pts = generate_point_grid(D)
    inp = torch.cat([lat.expand(pts.shape[0], -1), pts], 1)
    masks = []
    with torch.no_grad():
        x = inp
        for l in range(dec.n_lin):
            if l in dec.latent_in:
                x = torch.cat([x, inp], 1)
            v = getattr(dec, "l%d_weight_v" % l, None)
            w = v * (getattr(dec, "l%d_weight_g" % l) / v.norm(2, dim=1, keepdim=True)) if v is not None else getattr(dec, "l%d_weight" % l)
            x = F.linear(x, w, getattr(dec, "l%d_bias" % l))
            if l < dec.n_lin - 1:
                masks.append((x > 0).numpy())
                x = F.relu(x)
        sdf = torch.tanh(x)[:, 0].numpy()
    band = np.flatnonzero(np.abs(sdf) < THR)
    n_tiles = (len(band) + TILE - 1) // TILE
    print("crop %d: %d band rows, %d tiles of %d" % (crop, len(band), n_tiles, TILE))
    print("layer  out  alive/row  alive/tile mean  worst  padded K mean  share of 512")
    shares = []
    for l, m in enumerate(masks):
        mb = m[band]
        per_tile = np.array([mb[t * TILE:(t + 1) * TILE].any(0).sum() for t in range(n_tiles)])
        padded = np.maximum(TRIP, (per_tile + TRIP - 1) // TRIP * TRIP)
        if l >= 1:
            shares.append(padded.mean() / 512.0)
        print("%5d %4d %10.3f %16.3f %6.3f %14.1f %13.3f" % (l, m.shape[1], mb.mean(), per_tile.mean() / 512.0, per_tile.max() / 512.0, padded.mean(),
                                                          padded.mean() / 512.0))
    print("the seven products (masks 7 ... 1) run %.3f of the full K chain on average (survivors alone: %.3f)"
          % (float(np.mean(shares)), float(np.mean([np.mean([m[band][t * TILE:(t + 1) * TILE].any(0).sum() for t in range(n_tiles)]) / 512.0
                                                    for m in masks[1:]]))))


if __name__ == "__main__":
    main()
