"""Developer tool: time the hypergraph stage of YOLOv13 (ey_hypergraph_conv: one C3AH branch's AdaHGConv, five launches) per scale at
640^2 and 1280^2 (the P4 map: 40x40 / 80x80 tokens), batch 32, f16, replayed from a hipGraph -- against the eager PyTorch composition of
the same operations (torch.bmm / F.linear / softmax / GELU on the same device and f16 data), a yardstick only.  Prints one JSON line
per shape with the time per call, the time per launch, and the algorithmic bytes of the call (X read three times, Y written once, the
fp32 logits written and read) against the MI355X's 8 TB/s HBM.
usage: hypergraph_bench.py [reps]"""
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import edge_yolo_amd  # noqa: E402,F401
from edge_yolo_amd import _lib as L  # noqa: E402
from edge_yolo_amd.nn import _ops as ops  # noqa: E402
from edge_yolo_amd.nn.modules import AdaHGConv  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
B = 32
SCALES = [("n", 64, 4), ("s", 128, 8), ("l", 256, 8), ("x", 384, 12)]  # (scale, D, E); heads = D / 16
HBM = 8.0e12


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


def torch_form(m, X):
    """The reference's AdaHGConv.forward (block.py:1686-1774) in eager torch on (B, N, D) f16 tokens."""
    g = m.edge_generator
    Bn, N, D = X.shape
    ctx = torch.cat([X.mean(1), X.amax(1)], -1)
    P = g.prototype_base.unsqueeze(0) + F.linear(ctx, g.context_net.weight, g.context_net.bias).view(Bn, g.num_hyperedges, D)
    Xp = F.linear(X, g.pre_head_proj.weight, g.pre_head_proj.bias)
    h, hd = g.num_heads, g.head_dim
    xh = Xp.view(Bn, N, h, hd).transpose(1, 2).reshape(Bn * h, N, hd)
    ph = P.view(Bn, -1, h, hd).permute(0, 2, 1, 3).reshape(Bn * h, -1, hd).transpose(1, 2)
    logits = (torch.bmm(xh, ph) / g.scaling).view(Bn, h, N, -1).mean(1)
    A = F.softmax(logits, dim=1)
    He = F.gelu(F.linear(torch.bmm(A.transpose(1, 2), X), m.edge_proj[0].weight, m.edge_proj[0].bias))
    return F.gelu(F.linear(torch.bmm(A, He), m.node_proj[0].weight, m.node_proj[0].bias)) + X


with torch.no_grad():
    for imgsz in (640, 1280):
        for sc, D, E in SCALES:
            H = W = imgsz // 16
            N = H * W
            torch.manual_seed(0)
            m = AdaHGConv(D, E, D // 16)
            for lin in (m.edge_generator.context_net, m.edge_generator.pre_head_proj, m.edge_proj[0], m.node_proj[0]):
                lin.weight.data.normal_(0, 1 / math.sqrt(lin.in_features))
            m = m.to("cuda").half().eval()
            x = torch.randn(B, H, W, D, device="cuda", dtype=torch.float16).permute(0, 3, 1, 2)
            out = L.empty_nhwc(B, D, H, W, torch.float16, x.device)
            t_hip = timed(lambda: ops.hypergraph_conv(m, x, out=out))
            X = x.permute(0, 2, 3, 1).reshape(B, N, D)
            t_torch = timed(lambda: torch_form(m, X))
            ops.hypergraph_conv(m, x, out=out)
            err = float((out.permute(0, 2, 3, 1).reshape(B, N, D).float() - torch_form(m, X).float()).abs().max())
            nbytes = 3 * X.numel() * 2 + X.numel() * 2 + 2 * 4 * B * N * E
            print(json.dumps(dict(scale=sc, imgsz=imgsz, B=B, tokens=N, D=D, E=E, hip_us=round(t_hip, 1), us_per_launch=round(t_hip / ops.HG_LAUNCHES, 1),
                                  torch_us=round(t_torch, 1), torch_over_hip=round(t_torch / t_hip, 2), alg_MB=round(nbytes / 1e6, 1),
                                  hbm_floor_us=round(nbytes / HBM * 1e6, 1), max_abs_diff_vs_torch=err)), flush=True)
