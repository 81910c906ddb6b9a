"""Developer tool: time the flash attention core (ey_flash_attention) on the three attention shapes of yolov13n-DSC3K2_LGL at 640^2,
batch 32 -- 6400 tokens x head_dim 16 (layer 2), 1600 x 32 (layers 4, 21), 400 x 64 (layers 17, 26; layer 30 is 100 x 64 x 2 heads) --
against the VALU path the same shapes took before the flash kernel existed (ey_area_attention with one area: f16 VALU for head_dim 16 and
64; head_dim 32 runs flash_attn_kernel<32> through that entry too, so the VALU form is forced with areaattn_mfma=0 and the area entry's
MFMA time is listed as a check that both entries cost the same), each
replayed from a hipGraph.  Prints one JSON line per shape; mfma_peak_frac is against 2.5 PFLOP/s dense f16.
usage: flash_attn_bench.py [reps]"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import edge_yolo_amd  # noqa: E402,F401
from edge_yolo_amd import _lib as L  # noqa: E402
from edge_yolo_amd.nn import _ops as ops  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
PEAK = 2.5e15
# (label, B, H, W, heads, head_dim)
SHAPES = [("layer2 6400x16", 32, 80, 80, 1, 16), ("layer4 1600x32", 32, 40, 40, 1, 32), ("layer17 400x64", 32, 20, 20, 1, 64),
          ("layer30 100x64x2", 32, 10, 10, 2, 64)]


def timed(fn, n):
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(n):
            fn()
    g.replay()
    torch.cuda.synchronize()
    st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    st.record()
    g.replay()
    en.record()
    torch.cuda.synchronize()
    return st.elapsed_time(en) * 1000 / n  # us per call


def set_mfma(v):
    L.check(L.lib().ey_tune_set(b"areaattn_mfma", v), "tune")


for label, B, H, W, heads, hd in SHAPES:
    C, N = heads * hd, H * W
    qkv = torch.randn(B, H, W, 3 * C, device="cuda", dtype=torch.float16).permute(0, 3, 1, 2)
    q, k, v = qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:]
    out, out2 = (L.empty_nhwc(B, C, H, W, torch.float16, qkv.device) for _ in range(2))
    t_flash = timed(lambda: ops.flash_attention(q, k, v, heads, hd ** -0.5, out=out), reps)
    assert L.lib().ey_attention_last_variant() == L.ATTN_FLASH_MFMA + hd
    set_mfma(0)
    t_valu = timed(lambda: ops.area_attention(q, k, v, heads, 1, hd ** -0.5, out=out2), 1 if N > 2000 else reps)
    assert L.lib().ey_attention_last_variant() == L.ATTN_AREA_F16
    set_mfma(1)
    err = float((out.float() - out2.float()).abs().max())
    t_area_mfma = timed(lambda: ops.area_attention(q, k, v, heads, 1, hd ** -0.5, out=out2), reps) if hd == 32 else None
    flops = 4.0 * B * heads * N * N * hd
    print(json.dumps(dict(shape=label, batch=B, heads=heads, tokens=N, head_dim=hd, flash_us=round(t_flash, 1), valu_us=round(t_valu, 1),
                          valu_over_flash=round(t_valu / t_flash, 2), area_mfma_us=None if t_area_mfma is None else round(t_area_mfma, 1),
                          flash_tflops=round(flops / t_flash / 1e6, 1), mfma_peak_frac=round(flops / (t_flash * 1e-6) / PEAK, 4),
                          max_abs_diff_flash_vs_valu=err)), flush=True)
