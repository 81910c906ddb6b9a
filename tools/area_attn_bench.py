"""Developer tool: time the area-attention core (ey_area_attention) on the shapes of YOLOv12 -- the MFMA flash kernel (f16;
flash_attn_kernel<32>, the kernel of ey_flash_attention, with one group per run), the VALU
kernel (f16, areaattn_mfma=0) and torch's scaled_dot_product_attention on the same f16 data as a yardstick only -- each replayed
from a hipGraph.  Prints one JSON line per shape.
usage: area_attn_bench.py [reps]
Shapes (groups = images * areas, heads, tokens per area, head_dim 32): yolov12n at 640^2 batch 32 -- layer 6 (128 * 2 heads, 400),
layer 8 (32 * 4 heads, 400); at 1280^2 batch 8 -- layer 6 (8 * 4 areas * 2 heads, 1600), layer 8 (8 * 4 heads, 1600)."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import edge_yolo_amd  # noqa: E402,F401
from edge_yolo_amd import _lib as L  # noqa: E402
from edge_yolo_amd.nn import _ops as ops  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
# (label, B, H, W, area, heads)
SHAPES = [("640 layer6", 32, 40, 40, 4, 2), ("640 layer8", 32, 20, 20, 1, 4), ("1280 layer6", 8, 80, 80, 4, 2), ("1280 layer8", 8, 40, 40, 1, 4)]


def timed(fn):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(reps):
            fn()
    g.replay()
    torch.cuda.synchronize()
    st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    st.record()
    g.replay()
    en.record()
    torch.cuda.synchronize()
    return st.elapsed_time(en) * 1000 / reps  # us per call


def set_mfma(v):
    L.check(L.lib().ey_tune_set(b"areaattn_mfma", v), "tune")


for label, B, H, W, area, heads in SHAPES:
    C, N = heads * 32, H * W
    Na = N // area
    qkv = torch.randn(B, H, W, 3 * C, device="cuda", dtype=torch.float16).permute(0, 3, 1, 2)
    q, k, v = qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:]
    out = L.empty_nhwc(B, C, H, W, torch.float16, qkv.device)
    run = lambda: ops.area_attention(q, k, v, heads, area, 32 ** -0.5, out=out)  # noqa: E731
    set_mfma(1)
    t_mfma = timed(run)
    set_mfma(0)
    t_valu = timed(run)
    set_mfma(1)
    # SDPA on (B*area, heads, Na, 32) contiguous copies (its layout; the copies are not timed)
    rows = lambda t: t.permute(0, 2, 3, 1).reshape(B * area, Na, heads, 32).transpose(1, 2).contiguous()  # noqa: E731
    qs, ks, vs = rows(q), rows(k), rows(v)
    t_sdpa = timed(lambda: F.scaled_dot_product_attention(qs, ks, vs))
    ref = F.scaled_dot_product_attention(qs, ks, vs).transpose(1, 2).reshape(B, H, W, C).permute(0, 3, 1, 2)
    run()
    err = float((out.float() - ref.float()).abs().max())
    flops = 4.0 * B * area * heads * Na * Na * 32
    print(json.dumps(dict(shape=label, groups=B * area, heads=heads, tokens=Na, mfma_us=round(t_mfma, 2), valu_us=round(t_valu, 2),
                          sdpa_us=round(t_sdpa, 2), mfma_tflops=round(flops / t_mfma / 1e6, 2), valu_over_mfma=round(t_valu / t_mfma, 2),
                          sdpa_over_mfma=round(t_sdpa / t_mfma, 2), max_abs_diff_vs_sdpa=err)), flush=True)
