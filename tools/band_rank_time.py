"""Time the stretch between the grid forward and the band's Jacobian, both forms, on the sdf of a real step at D = 40:
    python tools/band_rank_time.py [B ...]            (default 1 2 4 8)
three launches: the ranking alone (sdfr_band_select_rank with no crops: the work of sdfr_tile_balance_kernel) + sdfr_band_select_ex's two kernels;
one launch:     sdfr_band_select_rank.
Each form is captured 20 times back to back into a graph and the graph replayed (no host launch cost between the kernels, as in a captured
refinement step); the figure is the best of 5 replays, per repetition.  The threshold of csrc/band_rank.hip (SDFR_BAND_RANK_MAX_ROWS) comes
from these figures."""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import sdflabel_amd
from sdflabel_amd import _lib
from sdflabel_amd.fixtures import ASSET, K_for

REPS = 20
dev = "cuda"
dec, _ = sdflabel_amd.setup_dsdf(ASSET + ".pt", precision=torch.float32)
dec = dec.to(dev)
L, P = _lib.lib(), _lib.ptr
ck = _lib.check
out = []
for B in [int(a) for a in sys.argv[1:]] or [1, 2, 4, 8]:
    br = sdflabel_amd.BatchRenderer(dec, 40, K_for(64, 64), (64, 64), B, device=dev)
    g = torch.Generator().manual_seed(1)
    lat = torch.tensor([[0.3, -0.5, 0.8]]) + 0.2 * (torch.rand(B, 3, generator=g) - 0.5)
    br.set_params(torch.full((B,), 0.7, device=dev), torch.tensor([[0.05, 0.02, 3.3]], device=dev).expand(B, 3), lat.to(dev))
    br.forward()
    torch.cuda.synchronize()
    G, cap = br.G, br.cap
    idx2, cnt2 = torch.empty_like(br.idx), torch.empty_like(br.cnt)

    def three(st):
        ck(L.sdfr_band_select_rank(P(br.sdf), G, 0, br.thr, None, None, P(idx2), cap, P(cnt2), None, None, 0, P(br.fwd_balance), G, st), "rank")
        ck(L.sdfr_band_select_ex(P(br.sdf), G, B, br.thr, None, None, P(idx2), cap, P(cnt2), None, P(br.scratch), P(br.over), 1, st), "ex")

    def one(st):
        ck(L.sdfr_band_select_rank(P(br.sdf), G, B, br.thr, None, None, P(idx2), cap, P(cnt2), None, P(br.over), 1, P(br.fwd_balance), G, st), "select_rank")

    res = {}
    for name, fn in (("three", three), ("one", one)):
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            fn(_lib.stream_ptr())
            s.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=s):
                for _ in range(REPS):
                    fn(_lib.stream_ptr())
        ts = []
        for _ in range(6):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            graph.replay()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) / REPS * 1e3)
        res[name] = min(ts[1:])
        assert torch.equal(cnt2, br.cnt) and all(torch.equal(idx2[b, :min(int(cnt2[b]), cap)], br.idx[b, :min(int(cnt2[b]), cap)]) for b in range(B)), name
        idx2.fill_(-1)
    out.append("B=%d (%d rows, band %d): three launches %.2f us, one launch %.2f us" % (B, B * G, int(br.cnt.sum()), res["three"], res["one"]))
    del br
print("\n".join(out))
