"""Per-layer cycle trace of one workgroup of the decoder forward kernels (library built with -DSDFR_MLP_TRACE, see tools/ab_variant.sh):
  SDFR_LIB=.../libsdfr_trace.so python tools/cycle_trace.py [f16|f32|ordered|split|t64]
Prints, per layer and for every wave of workgroup 0: product loop, wait at the first barrier, epilogue, wait at the second barrier (shader
cycles), then per layer the spread between the first and the last wave to finish the product and the longest wait at the first barrier.
ordered: the exact-f32 grid forward through sdfr_mlp_forward_ordered with the 4x4x4-block tile order, as the headline launches it."""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch, torch.nn.functional as F, sdflabel_amd
from sdflabel_amd import _lib
from sdflabel_amd.fixtures import ASSET
which = sys.argv[1] if len(sys.argv) > 1 else "f16"
dev = "cuda"
dec, _ = sdflabel_amd.setup_dsdf(ASSET + ".pt", precision=torch.float32); dec = dec.to(dev)
h = dec.handle(torch.device(dev, 0)).h
grid = sdflabel_amd.Grid3D(40, dev); lat = F.normalize(torch.tensor([0.3, -0.5, 0.8], device=dev), dim=0)
inp = torch.cat([lat.expand(grid.points.size(0), -1), grid.points.detach()], 1).contiguous()
out = torch.empty(inp.shape[0], device=dev)
L = _lib.lib()
mws = torch.empty(int(L.sdfr_decoder_mask_words(h, inp.shape[0])), dtype=torch.int32, device=dev)
fn = {"f16": L.sdfr_mlp_forward_f16, "f32": L.sdfr_mlp_forward, "split": L.sdfr_mlp_forward_split}.get(which)
if which == "ordered":
    order = torch.empty(inp.shape[0], dtype=torch.int32)
    _lib.check(L.sdfr_grid_tile_order(40, _lib.ptr(order)), "sdfr_grid_tile_order")
    order = order.to(dev)
    fn = lambda h_, i_, n_, o_, m_, s_: L.sdfr_mlp_forward_ordered(h_, i_, n_, o_, m_, _lib.ptr(order), n_, s_)
if which == "t64":
    # the 64-row half forward of the sphere tracer's march (sdfr_mlp_forward_counted, half | 2, on 16 000 rows: one round of 250 tiles)
    inp = inp[:16000].contiguous()
    cnt = torch.tensor([16000], dtype=torch.int32, device=dev)
    fn = lambda h_, i_, n_, o_, m_, s_: L.sdfr_mlp_forward_counted(h_, i_, n_, _lib.ptr(cnt), o_, 3, s_)
NWMAX, NL = 8, 16
trace = torch.zeros(NWMAX * NL * 5, dtype=torch.int64, device=dev)
for _ in range(3):
    _lib.check(fn(h, _lib.ptr(inp), inp.shape[0], _lib.ptr(out), _lib.ptr(mws), _lib.stream_ptr()), "fwd")
L.sdfr_debug_set_trace(_lib.ptr(trace))
_lib.check(fn(h, _lib.ptr(inp), inp.shape[0], _lib.ptr(out), _lib.ptr(mws), _lib.stream_ptr()), "fwd")
torch.cuda.synchronize()
L.sdfr_debug_set_trace(None)
t = trace.cpu().view(NWMAX, NL, 5)
waves = [w for w in range(NWMAX) if int(t[w, 0, 0]) != 0]
print("%s forward, workgroup 0, shader cycles (s_memtime): product / barrier 1 / epilogue / barrier 2" % which)
print("layer | " + " | ".join("wave %d" % w for w in waves))
tot = 0
summary = []
for l in range(8):
    cells = []
    for w in waves:
        s = t[w, l]
        cells.append("%d / %d / %d / %d" % (int(s[1] - s[0]), int(s[2] - s[1]), int(s[3] - s[2]), int(s[4] - s[3])))
    done = [int(t[w, l, 1]) for w in waves]
    wait = [int(t[w, l, 2] - t[w, l, 1]) for w in waves]
    start = min(int(t[w, l, 0]) for w in waves)
    summary.append((l, max(done) - min(done), waves[done.index(min(done))], waves[done.index(max(done))], max(wait), max(done) - start))
    tot += int(t[0, l, 4] - t[0, l, 0])
    print("%5d | %s" % (l, " | ".join(cells)))
print("sum of the 8 layers (wave 0): %d cycles" % tot)
print("layer | product spread (last - first wave done) | first wave | last wave | longest wait at barrier 1 | product of the last wave")
for row in summary:
    print("%5d | %7d | %d | %d | %7d | %7d" % row)
# finishing order of the product per layer, earliest first: which waves are late (young half or particular SIMDs: wave w runs on SIMD w % 4)
for l in range(8):
    order_l = sorted(waves, key=lambda w: int(t[w, l, 1]))
    print("layer %d finishing order: %s" % (l, " ".join(str(w) for w in order_l)))
