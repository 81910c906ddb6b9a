"""fp64 restatement of AdaHGConv (reference block.py:1640-1774, steps 1-5 of DESIGN.md section 7c) on (B, N, D) tokens, written from
the maths with the per-head logits (not the folded form the kernel uses), for the -m gpu kernel tests."""
import math

import torch


def hypergraph_fp64(x, w, heads, context="both"):
    """x (B,N,D); w = (proto_base, ctx_w, ctx_b, pre_w, pre_b, edge_w, edge_b, node_w, node_b) as nn.Linear stores them ([out][in])."""
    base, cw, cb, pw, pb, ew, eb, nw, nb = (t.detach().double().cpu() for t in w)
    x = x.double().cpu()
    B, N, D = x.shape
    E = base.shape[0]
    mean, mx = x.mean(1), x.amax(1)
    ctx = {"both": torch.cat([mean, mx], -1), "mean": mean, "max": mx}[context]
    P = base.unsqueeze(0) + (ctx @ cw.T + cb).view(B, E, D)
    xp = x @ pw.T + pb
    hd = D // heads
    logits = torch.einsum("bnhd,behd->bnhe", xp.view(B, N, heads, hd), P.view(B, E, heads, hd)) / math.sqrt(hd)
    A = torch.softmax(logits.mean(2), dim=1)  # (B, N, E): over the tokens
    gelu = torch.nn.functional.gelu
    He = gelu(A.transpose(1, 2) @ x @ ew.T + eb)
    return gelu((A @ He) @ nw.T + nb) + x
