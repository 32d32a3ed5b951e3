"""Run only the decoder forward (G=64000) a few times -- target for rocprofv3 PMC passes.
usage: mlp_only.py [launches] [f32|f16|split] [dropin|plain|ordered]
dropin (default): the drop-in Decoder(inputs) call.  plain / ordered (f32): sdfr_mlp_forward / sdfr_mlp_forward_ordered with a mask buffer, as
BatchRenderer launches them -- ordered with the 4x4x4-block tile order of sdfr_grid_tile_order."""
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
    if how == "ordered":
        order = torch.empty(G, dtype=torch.int32)
        _lib.check(L.sdfr_grid_tile_order(40, P(order)), "sdfr_grid_tile_order")
        order = order.to(dev)
    for _ in range(n):
        if how == "ordered":
            _lib.check(L.sdfr_mlp_forward_ordered(h, P(inputs), G, P(sdf), P(mw), P(order), G, _lib.stream_ptr()), "sdfr_mlp_forward_ordered")
        else:
            _lib.check(L.sdfr_mlp_forward(h, P(inputs), G, P(sdf), P(mw), _lib.stream_ptr()), "sdfr_mlp_forward")
torch.cuda.synchronize()
