"""Per-layer cycle trace of one workgroup of the decoder forward kernels (library built with -DSDFR_MLP_TRACE, see tools/ab_variant.sh):
  SDFR_LIB=.../libsdfr_trace.so python tools/cycle_trace.py [f16|f32|ordered|split|t64|jac]
Prints, per layer and for every wave of workgroup 0: product loop, wait at the first barrier, epilogue, wait at the second barrier (shader
cycles), then per layer the spread between the first and the last wave to finish the product and the longest wait at the first barrier.
ordered: the exact-f32 grid forward through sdfr_mlp_forward_ordered with the 4x4x4-block tile order, as the headline launches it.
jac: the 16-row float32 mask-fed band Jacobian (library built with SDFR_JAC_DEFS="-DSDFR_MLP_TRACE"), layers 7 ... 1."""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch, torch.nn.functional as F, sdflabel_amd
from sdflabel_amd import _lib
from sdflabel_amd.fixtures import ASSET
which = sys.argv[1] if len(sys.argv) > 1 else "f16"
dev = "cuda"
if which == "jac":
    # the 16-row float32 mask-fed band Jacobian of the bench's shape (one crop, 40^3 grid), workgroup 0 = the band's first 16 rows; layers run
    # 7 ... 1: product / wait at the barrier behind it (the compaction's survivor vote included) / store_in_grad (masking and the compacted
    # operand) / second barrier.  SDFR_JAC_COMPACT=0 in the environment traces the full chain.
    from sdflabel_amd.fixtures import K_for
    dec, _ = sdflabel_amd.setup_dsdf(ASSET + ".pt", precision=torch.float32); dec = dec.to(dev)
    br = sdflabel_amd.BatchRenderer(dec, 40, K_for(64, 64), (64, 64), 1, device=dev)
    br.set_params(torch.full((1,), 0.7, device=dev), torch.tensor([[0.05, 0.02, 3.3]], device=dev), torch.tensor([[0.3, -0.5, 0.8]], device=dev))
    br.forward(); torch.cuda.synchronize()
    L, P = _lib.lib(), _lib.ptr
    jac = lambda: _lib.check(L.sdfr_mlp_jacobian(br.handle.h, P(br.inputs), br.G, 1, P(br.idx), br.cap, P(br.cnt), P(br.J), P(br.sdf_band), P(br.sdf),
                                                 P(br.mask_ws), 0, _lib.stream_ptr()), "sdfr_mlp_jacobian")
    trace = torch.zeros(8 * 16 * 5, dtype=torch.int64, device=dev)
    for _ in range(3): jac()
    L.sdfr_debug_set_trace(P(trace)); jac(); torch.cuda.synchronize(); L.sdfr_debug_set_trace(None)
    t = trace.cpu().view(8, 16, 5)
    print("band Jacobian (SDFR_JAC_COMPACT=%s), workgroup 0, shader cycles: product / barrier 1 / store_in_grad / barrier 2" % os.environ.get("SDFR_JAC_COMPACT", "1"))
    print("layer | " + " | ".join("wave %d" % w for w in range(4)) + " | layer, wave 0")
    tot = [0, 0, 0, 0]
    for l in range(7, 0, -1):
        cells = ["%d / %d / %d / %d" % tuple(int(t[w, l, i + 1] - t[w, l, i]) for i in range(4)) for w in range(4)]
        for i in range(4): tot[i] += max(int(t[w, l, i + 1] - t[w, l, i]) for w in range(4)) if i in (0, 2) else min(int(t[w, l, i + 1] - t[w, l, i]) for w in range(4))
        print("%5d | %s | %d" % (l, " | ".join(cells), int(t[0, l, 4] - t[0, l, 0])))
    print("layers 7 ... 1: slowest wave's product %d, shortest wait at barrier 1 %d, slowest store_in_grad %d, shortest wait at barrier 2 %d" % tuple(tot))
    print("kernel start to the end of layer 1 (wave 0): %d cycles; top operand (stamp 8: 3 -> 4) %d; first layer (stamp 9: 0 -> 2) %d"
          % (int(t[0, 1, 4] - t[0, 8, 0]), int(t[0, 8, 4] - t[0, 8, 3]), int(t[0, 9, 2] - t[0, 9, 0])))
    sys.exit(0)
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
