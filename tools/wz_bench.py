"""Developer tool: time the fused half-resolution wavelet branch (ey_wavelet_z / ey_wavelet_z2) at the shapes of EdgeLine-n, replayed
from a hipGraph.
usage: wz_bench.py [--wave NAME] [--use-ds] [reps] [c,hw ...]      (--wave: any pywt bank of 2, 4, 6 or 8 taps; default haar)"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import edge_yolo_amd  # noqa: E402,F401
from edge_yolo_amd.nn import _ops as ops  # noqa: E402
from edge_yolo_amd.nn.modules import block as B  # noqa: E402

args = sys.argv[1:]
wave, use_ds = "haar", "--use-ds" in args
args = [a for a in args if a != "--use-ds"]
if "--wave" in args:
    i = args.index("--wave")
    wave = args[i + 1]
    del args[i:i + 2]
SHAPES = [(16, 160), (32, 80), (64, 40), (128, 20)]
if len(args) > 1:
    SHAPES = [tuple(int(v) for v in a.split(",")) for a in args[1:]]
reps = int(args[0]) if args else 20
for c, hw in SHAPES:
    m = B._WaveletEnhancer(c, use_ds=use_ds, wave=wave).cuda().half().eval()
    dw_fn = (lambda m=m: m.f_h._dw_folded()[0]) if use_ds else None
    for mod in m.modules():
        if hasattr(mod, "fuse_bn") and hasattr(mod, "bn"):
            mod.fuse_bn()
    xs = [torch.randn(32, hw, hw, c, device="cuda", dtype=torch.float16).permute(0, 3, 1, 2) for _ in range(6)]
    for x in xs[:2]:
        ops.wavelet_z(m, x, m._subband_sets, m._fuse_z, dwt=m.dwt, dw_fn=dw_fn)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        zs = [ops.wavelet_z(m, xs[i % 6], m._subband_sets, m._fuse_z, dwt=m.dwt, dw_fn=dw_fn) for i in range(reps)]
    g.replay()
    torch.cuda.synchronize()
    st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    st.record()
    for _ in range(5):
        g.replay()
    en.record()
    torch.cuda.synchronize()
    us = st.elapsed_time(en) / (5 * reps) * 1e3
    print(f"wavelet_z {wave}{' use_ds' if use_ds else ''} C{c} {hw}x{hw}: {us:8.1f} us", flush=True)
