"""Per-tile Gantt of the exact-f32 grid forward (library built with -DSDFR_MLP_TRACE, see tools/ab_variant.sh):
  SDFR_ALLOW_AB=1 SDFR_LIB=.../libsdfr_trace.so python tools/tile_gantt.py [--crop I] [--launches N] [--order FILE.npy | --balanced]
                                                                            [--save FILE.npz] [--lpt-out FILE.npy]
  python tools/tile_gantt.py --load FILE.npz          (the analysis alone, no GPU)
Runs sdfr_mlp_forward_ordered on the bench's shape (one crop, 40^3 grid, the start latent of crop I) with the tile trace on
(sdfr_debug_set_tile_trace: per workgroup start / end in shader cycles and in the 100 MHz constant clock, the CU it ran on, blockIdx.x) and
prints
  - the distribution of the tile times and their correlation with the CPU model's sum of padded K (tools/fwd_balance_model.py),
  - where the launch slots go: XCD of slot s against s % 8, and whether the tiles of an XCD start in blockIdx order,
  - tiles per CU, and the CU-idle time before the kernel's end as a share of CUs x kernel time.
--order: a row order to launch with instead of sdfr_grid_tile_order's (int32 [G]; e.g. the file --lpt-out wrote: is the tail gone?).
--balanced: sdfr_mlp_forward_balanced instead (the warm-up launches give it its prior; the input does not change, so neither does the order).
--lpt-out: the static order with its 64-entry chunks permuted heaviest measured tile first (median over the launches, ties by static index)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

WORDS = 6


def measure(args):
    import torch
    import torch.nn.functional as F
    import sdflabel_amd
    from sdflabel_amd import _lib
    from sdflabel_amd.fixtures import ASSET, ASSET_ELLIPSOID, crop_start
    dev = "cuda"
    asset = ASSET_ELLIPSOID if args.ellipsoid else ASSET
    dec, _ = sdflabel_amd.setup_dsdf(asset + ".pt", precision=torch.float32)
    dec = dec.to(dev)
    L, P = _lib.lib(), _lib.ptr
    h = dec.handle(torch.device(dev, 0)).h
    D = args.density
    grid = sdflabel_amd.Grid3D(D, dev)
    lat = F.normalize(torch.as_tensor(crop_start(args.crop)[2], dtype=torch.float32, device=dev).view(-1), dim=0)
    inp = torch.cat([lat.expand(grid.points.size(0), -1), grid.points.detach()], 1).contiguous()
    G = inp.shape[0]
    static = torch.empty(G, dtype=torch.int32)
    _lib.check(L.sdfr_grid_tile_order(D, P(static)), "sdfr_grid_tile_order")
    order = static
    if args.order:
        order = torch.from_numpy(np.load(args.order).astype(np.int32))
        assert order.shape == (G,) and np.array_equal(np.sort(order.numpy()), np.arange(G)), "--order: not a permutation of the grid's rows"
    order_d = order.to(dev)
    sdf = torch.empty(G, device=dev)
    mws = torch.zeros(int(L.sdfr_decoder_mask_words(h, G)), dtype=torch.int32, device=dev)
    tiles = (G + 63) // 64
    rec = torch.zeros(args.launches, tiles, WORDS, dtype=torch.int64, device=dev)

    state = None
    if args.balanced:
        state = torch.empty(int(L.sdfr_mlp_balance_bytes(G)) // 4, dtype=torch.int32, device=dev)
        _lib.check(L.sdfr_mlp_balance_init(P(state), P(order_d), G, _lib.stream_ptr()), "sdfr_mlp_balance_init")

    def fwd():
        if state is not None:
            return _lib.check(L.sdfr_mlp_forward_balanced(h, P(inp), G, P(sdf), P(mws), P(state), G, _lib.stream_ptr()), "sdfr_mlp_forward_balanced")
        _lib.check(L.sdfr_mlp_forward_ordered(h, P(inp), G, P(sdf), P(mws), P(order_d), G, _lib.stream_ptr()), "sdfr_mlp_forward_ordered")
    for _ in range(args.warmup):
        fwd()
    torch.cuda.synchronize()
    if state is not None:                                        # the order the traced launches run
        order = state[3 * tiles + 4:3 * tiles + 4 + G].cpu()          # (csrc/tile_balance.h: the state's order field)
    for i in range(args.launches):
        L.sdfr_debug_set_tile_trace(P(rec[i]), tiles)
        fwd()
        torch.cuda.synchronize()
    L.sdfr_debug_set_tile_trace(None, 0)
    rec = rec.cpu().numpy()
    if not rec[:, :, 2].any():
        sys.exit("no tile was stamped: is SDFR_LIB a library built with -DSDFR_MLP_TRACE?")
    # the chunk of the static order each launch slot evaluates (a chunk = 64 entries of sdfr_grid_tile_order = one 4x4x4 block at D % 4 == 0)
    first = {int(r): c for c, r in enumerate(static.numpy()[::64])}
    chunk = np.array([first.get(int(r), -1) for r in order.numpy()[::64]], np.int64)
    meta = dict(rec=rec, chunk=chunk, density=D, crop=args.crop, ellipsoid=int(args.ellipsoid))
    if args.save:
        os.makedirs(os.path.dirname(os.path.abspath(args.save)), exist_ok=True)
        np.savez_compressed(args.save, **meta)
    if args.lpt_out:
        dur = np.median(rec[:, :, 2] - rec[:, :, 0], axis=0)           # per launch slot
        cost = np.zeros(tiles)
        cost[chunk] = dur                                              # per static chunk
        full = G // 64
        rank = np.concatenate([np.argsort(-cost[:full], kind="stable"), np.arange(full, tiles)])
        st = static.numpy()
        out = np.concatenate([st[c * 64:(c + 1) * 64] for c in rank]).astype(np.int32)
        assert np.array_equal(np.sort(out), np.arange(G))
        np.save(args.lpt_out, out)
        print("wrote %s: %d chunks, heaviest measured first" % (args.lpt_out, tiles))
    return meta


def analyse(meta, model=True, out=print):
    rec, chunk = np.asarray(meta["rec"]), np.asarray(meta["chunk"])
    n_l, tiles, _ = rec.shape
    cyc = (rec[:, :, 2] - rec[:, :, 0]).astype(np.float64)
    t0, t1 = rec[:, :, 1].astype(np.float64) * 10.0, rec[:, :, 3].astype(np.float64) * 10.0          # ns
    xcd = (rec[:, :, 4] >> 32) & 0xF
    cu = xcd * 256 + ((rec[:, :, 4] >> 8) & 0xFF)                                                    # (XCD, SE, SH, CU)
    assert np.array_equal(rec[:, :, 5], np.broadcast_to(np.arange(tiles), (n_l, tiles))), "records are not indexed by blockIdx.x"
    out("%d launches x %d tiles, D = %d, start latent of crop %d%s" % (n_l, tiles, int(meta["density"]), int(meta["crop"]),
                                                                         ", ellipsoid fixture" if int(meta["ellipsoid"]) else ""))
    # ---- tile times -------------------------------------------------------------------------------------------------------------------
    ns = t1 - t0
    ghz = np.median(cyc / ns)
    out("tile time, shader cycles: min %.0f  p5 %.0f  median %.0f  p95 %.0f  max %.0f  (mean %.0f; %.3f GHz against the constant clock)"
        % (cyc.min(), np.percentile(cyc, 5), np.median(cyc), np.percentile(cyc, 95), cyc.max(), cyc.mean(), ghz))
    med = np.median(cyc, axis=0)
    out("per-slot median over the launches: min %.0f  max %.0f; spread of one slot between launches (max - min), median %.0f cycles"
        % (med.min(), med.max(), np.median(cyc.max(0) - cyc.min(0))))
    # first round (launch slots < 256, nothing else on the CU before) against the later ones
    nfirst = min(256, tiles)
    if tiles > nfirst:
        out("mean tile time of the first %d slots %.0f cycles, of the rest %.0f" % (nfirst, cyc[:, :nfirst].mean(), cyc[:, nfirst:].mean()))
    if model and int(meta["density"]) % 4 == 0:
        from tools.fwd_balance_model import tile_kpad
        from sdflabel_amd.fixtures import ASSET, ASSET_ELLIPSOID, crop_start
        kp = tile_kpad(ASSET_ELLIPSOID if int(meta["ellipsoid"]) else ASSET, [crop_start(int(meta["crop"]))[2]], int(meta["density"]))[0]
        k = kp[chunk].astype(np.float64)
        a, b = np.polyfit(k, med, 1)
        out("model: sum K_pad %d .. %d; correlation with the median tile time %.4f; least squares tile = %.0f + %.1f * sum K_pad cycles "
            "(model: 55000 + 302.8), residual rms %.0f cycles" % (k.min(), k.max(), np.corrcoef(k, med)[0, 1], b, a,
                                                                  np.sqrt(np.mean((med - (a * k + b)) ** 2))))
    # ---- placement --------------------------------------------------------------------------------------------------------------------
    for i in range(n_l):
        slot = np.arange(tiles)
        # one label per residue class s % 8?
        same = sum(len(np.unique(xcd[i][slot % 8 == r])) == 1 for r in range(8))
        ncu = len(np.unique(cu[i]))
        per_cu = np.bincount(np.unique(cu[i], return_inverse=True)[1])
        inv = tot = 0
        late = 0.0
        for x in np.unique(xcd[i]):
            m = np.nonzero(xcd[i] == x)[0]                      # ascending blockIdx
            s = t0[i][m]
            # pairs (a < b in blockIdx) that started in the opposite order, beyond the clock's resolution
            d = s[None, :] - s[:, None]
            iu = np.triu_indices(len(m), 1)
            inv += int((d[iu] < -10.0).sum())
            tot += len(iu[0])
            late = max(late, float((np.maximum.accumulate(s) - s).max()))
        kern0, kern1 = t0[i].min(), t1[i].max()
        span = kern1 - kern0
        busy = ns[i].sum()
        last = np.array([t1[i][cu[i] == c].max() for c in np.unique(cu[i])])
        first_ = np.array([t0[i][cu[i] == c].min() for c in np.unique(cu[i])])
        gaps = span * ncu - busy - (kern1 - last).sum() - (first_ - kern0).sum()
        out("launch %d: %d XCDs, %d CUs, tiles per CU %s; residues s %% 8 on one XCD each: %d of 8; start order against blockIdx within an XCD: "
            "%d of %d pairs inverted (%.2f %%), latest start behind a higher blockIdx %.0f ns"
            % (i, len(np.unique(xcd[i])), ncu, {int(k): int(v) for k, v in zip(*np.unique(per_cu, return_counts=True))}, same, inv, tot, 100.0 * inv / max(tot, 1), late))
        out("    kernel (first start to last end) %.1f us; CU idle %.2f %% of CUs x kernel: before the first tile %.2f %%, between tiles "
            "%.2f %%, behind the CU's last tile %.2f %%; balanced (busy / CUs) %.1f us, kernel above it %+.2f %%"
            % (span / 1e3, 100.0 * (1 - busy / (span * ncu)), 100.0 * (first_ - kern0).sum() / (span * ncu), 100.0 * gaps / (span * ncu),
               100.0 * (kern1 - last).sum() / (span * ncu), busy / ncu / 1e3, 100.0 * (span * ncu / busy - 1)))
        ends = np.sort(last)
        out("    a CU's last tile ends before the kernel's end: earliest CU %.1f us, median CU %.1f us"
            % ((kern1 - ends[0]) / 1e3, (kern1 - np.median(ends)) / 1e3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--crop", type=int, default=0)
    ap.add_argument("--density", type=int, default=40)
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--ellipsoid", action="store_true")
    ap.add_argument("--order", default=None)
    ap.add_argument("--balanced", action="store_true")
    ap.add_argument("--save", default=None)
    ap.add_argument("--lpt-out", default=None)
    ap.add_argument("--load", default=None)
    ap.add_argument("--no-model", action="store_true")
    args = ap.parse_args()
    meta = dict(np.load(args.load)) if args.load else measure(args)
    analyse(meta, model=not args.no_model)


if __name__ == "__main__":
    main()
