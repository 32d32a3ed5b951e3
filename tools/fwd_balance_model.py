"""CPU model of how the tiles of the exact-f32 grid forward fill the machine (profiles/fwd_balance_notes.md), no GPU needed:
  python tools/fwd_balance_model.py [D]
A tile is one 4x4x4 block of the D^3 grid (sdfr_grid_tile_order); the per-tile K compaction makes its cost depend on how many operand
features survive in it.  Tile cost = FIXED + c * sum over the 7 compacted layers of the surviving K rounded up to 16 (shader cycles), c
calibrated so that tile 0 of the first fixture's crop 0 costs TILE0 cycles, the figure of the cycle trace (profiles/kc_dense_notes.md).
Tiles are handed out in launch order to whichever CU is free first -- over all 256 CUs, or per XCD with launch slot s on XCD s % 8 (32 CUs
each) -- and the makespan is set against the perfectly balanced sum / 256.  Orders compared: the static block order, heaviest tile first (LPT)
on the tile's own costs, LPT on the costs of another start latent of the same decoder, LPT on the other decoder's costs."""
import heapq
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

FIXED, TILE0, CUS, XCDS, GHZ = 55e3, 554e3, 256, 8, 2.4
STARTS = (0, 1, 5, 17, 40)


def tile_kpad(asset, latents, D=40):
    """[latent][tile] sum over the compacted layers of the surviving K, padded to 16, for the tiles of sdfr_grid_tile_order(D) (full
    64-row tiles only; rows of a partial last tile are left out)"""
    from tests.test_fwd_order_cpu import _alive, tile_order
    order = torch.from_numpy(tile_order(D).astype(np.int64))
    full = order.shape[0] // 64 * 64
    out = []
    for per_layer in _alive(asset, latents, D):
        k = 0
        for nz in per_layer:
            t = nz[order[:full]].view(-1, 64, nz.shape[1]).any(1).sum(1)
            k = k + (t + 15) // 16 * 16
        out.append(k.numpy().astype(np.int64))
    return out


def lpt_rank(cost):
    """launch positions, heaviest tile first, ties by static index: the stable descending sort"""
    return np.argsort(-np.asarray(cost), kind="stable")


def makespan(cost, launch, per_xcd):
    """greedy list scheduling: tile launch[s] goes to the CU that is free first (of all CUs, or of XCD s % 8)"""
    groups = XCDS if per_xcd else 1
    heaps = [[0.0] * (CUS // groups) for _ in range(groups)]
    for s, t in enumerate(launch):
        h = heaps[s % groups]
        heapq.heappush(h, heapq.heappop(h) + float(cost[t]))
    return max(max(h) for h in heaps)


def report(D=40, out=print):
    from sdflabel_amd.fixtures import ASSET, ASSET_ELLIPSOID, crop_start
    lat = [crop_start(i)[2] for i in STARTS]
    kp = {a: tile_kpad(a, lat, D) for a in (ASSET, ASSET_ELLIPSOID)}
    c = (TILE0 - FIXED) / float(kp[ASSET][0][0])
    cost = {a: [FIXED + c * k for k in kp[a]] for a in kp}
    out("model: D = %d, %d tiles, cost = %.0f + %.2f * sum K_pad cycles (tile 0 = %.0f)" % (D, len(kp[ASSET][0]), FIXED, c, TILE0))
    rows = []
    for a in kp:
        name = a.rsplit("/", 1)[-1]
        other = [x for x in kp if x != a][0]
        for i, s in enumerate(STARTS):
            w = cost[a][i]
            ideal = w.sum() / CUS
            share = kp[a][i] / (7 * 512.0)
            static = np.arange(len(w))
            prior = cost[a][(i + 1) % len(STARTS)]          # another start latent of the same decoder
            res = {}
            for label, launch in (("static", static), ("lpt", lpt_rank(w)), ("lpt_other_crop", lpt_rank(prior)),
                                  ("lpt_other_fixture", lpt_rank(cost[other][i]))):
                res[label] = (makespan(w, launch, False) / ideal - 1.0, makespan(w, launch, True) / ideal - 1.0)
            rows.append((name, s, res))
            out("%s start %2d: tile cost %.3f .. %.3f M cycles, K_pad share %.3f .. %.3f (mean %.4f), balanced %.3f M cycles, static makespan "
                "%.3f M = %.3f ms at %.1f GHz, cost correlation with the prior %.4f"
                % (name, s, w.min() / 1e6, w.max() / 1e6, share.min(), share.max(), share.mean(), ideal / 1e6,
                   makespan(w, static, True) / 1e6, makespan(w, static, True) / GHZ / 1e6, GHZ, np.corrcoef(w, prior)[0, 1]))
            out("    above balanced, global / per XCD:  " + "  ".join("%s %+.1f %% / %+.1f %%" % (k, 100 * v[0], 100 * v[1]) for k, v in res.items()))
    return rows


if __name__ == "__main__":
    report(int(sys.argv[1]) if len(sys.argv) > 1 else 40)
