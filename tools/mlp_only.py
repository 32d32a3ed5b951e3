"""Run only the decoder forward (G=64000) a few times -- target for rocprofv3 PMC passes.
usage: mlp_only.py [launches] [f32|f16|split] [dropin|plain|ordered|balanced]
dropin (default): the drop-in Decoder(inputs) call.  plain / ordered (f32): sdfr_mlp_forward / sdfr_mlp_forward_ordered with a mask buffer, as
BatchRenderer launches them -- ordered with the 4x4x4-block tile order of sdfr_grid_tile_order; balanced: sdfr_mlp_forward_balanced on that
order (the renderer's default: the launch order of the tiles follows the last launch's costs, and the ranking kernel runs behind each)."""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch, torch.nn.functional as F
import sdflabel_amd
from sdflabel_amd.fixtures import ASSET
dev = "cuda"
dec, _ = sdflabel_amd.setup_dsdf(ASSET + ".pt", precision=torch.float32); dec = dec.to(dev)
grid = sdflabel_amd.Grid3D(40, dev)
lat = F.normalize(torch.tensor([0.3, -0.5, 0.8], device=dev), dim=0)
inputs = torch.cat([lat.expand(grid.points.size(0), -1), grid.points], 1).contiguous()
n = int(sys.argv[1]) if len(sys.argv) > 1 else 10
dec.mlp_precision = {"f32": torch.float32, "f16": torch.float16, "split": "float32_split"}[sys.argv[2] if len(sys.argv) > 2 else "f32"]
how = sys.argv[3] if len(sys.argv) > 3 else "dropin"
if how == "dropin":
    with torch.no_grad():
        for _ in range(n):
            dec(inputs)
else:
    from sdflabel_amd import _lib
    L, P, G = _lib.lib(), _lib.ptr, inputs.shape[0]
    h = dec.handle(torch.device(dev)).h
    sdf = torch.empty(G, device=dev)
    mw = torch.zeros(int(L.sdfr_decoder_mask_words(h, G)), dtype=torch.int32, device=dev)
    if how in ("ordered", "balanced"):
        order = torch.empty(G, dtype=torch.int32)
        _lib.check(L.sdfr_grid_tile_order(40, P(order)), "sdfr_grid_tile_order")
        order = order.to(dev)
    if how == "balanced":
        state = torch.empty(int(L.sdfr_mlp_balance_bytes(G)) // 4, dtype=torch.int32, device=dev)
        _lib.check(L.sdfr_mlp_balance_init(P(state), P(order), G, _lib.stream_ptr()), "sdfr_mlp_balance_init")
    for _ in range(n):
        if how == "balanced":
            _lib.check(L.sdfr_mlp_forward_balanced(h, P(inputs), G, P(sdf), P(mw), P(state), G, _lib.stream_ptr()), "sdfr_mlp_forward_balanced")
        elif how == "ordered":
            _lib.check(L.sdfr_mlp_forward_ordered(h, P(inputs), G, P(sdf), P(mw), P(order), G, _lib.stream_ptr()), "sdfr_mlp_forward_ordered")
        else:
            _lib.check(L.sdfr_mlp_forward(h, P(inputs), G, P(sdf), P(mw), _lib.stream_ptr()), "sdfr_mlp_forward")
torch.cuda.synchronize()
