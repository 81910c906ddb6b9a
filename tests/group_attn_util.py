"""Inputs, NaN-guarded channel windows and the float64 reference shared by test_gpu_area_attention_exact.py, test_gpu_flash_attention_exact.py
and test_gpu_attention_entries_equal.py.  Attention runs within token groups: the H*W tokens of an image, row-major, are cut into `area`
contiguous runs (area = 1: the whole image, ey_flash_attention).  The group layout below is (B*area, heads, tokens per group, head_dim)."""
import zlib

import torch


def gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def lib():
    from edge_yolo_amd import _lib as L
    return L


def window(vals, off, pad, dtype):
    """NHWC device view of logical (B, C, H, W) vals at channel offset `off` of a (off + C + pad)-channel NaN-filled buffer."""
    B, C, H, W = vals.shape
    buf = torch.full((B, H, W, off + C + pad), float("nan"), dtype=dtype, device="cuda")
    buf[..., off:off + C] = vals.permute(0, 2, 3, 1).to(device="cuda", dtype=dtype)
    return buf, buf.permute(0, 3, 1, 2)[:, off:off + C]


def run(op, q, k, v, dtype, qoff=8, yoff=8, ypad=8):
    """op(q view, k view, v view, out view) on windows of NaN-filled buffers -> y logical (B,C,H,W) float64 cpu"""
    B, C, H, W = q.shape
    qkbuf, _ = window(torch.cat([q, k], 1), qoff, 8, dtype)
    qv = qkbuf.permute(0, 3, 1, 2)[:, qoff:qoff + C]
    kv = qkbuf.permute(0, 3, 1, 2)[:, qoff + C:qoff + 2 * C]
    _, vv = window(v, 16, 8, dtype)
    ybuf = torch.full((B, H, W, yoff + C + ypad), float("nan"), dtype=dtype, device="cuda")
    yv = ybuf.permute(0, 3, 1, 2)[:, yoff:yoff + C]
    op(qv, kv, vv, yv)
    torch.cuda.synchronize()
    assert torch.isnan(ybuf[..., :yoff]).all() and torch.isnan(ybuf[..., yoff + C:]).all(), "writes outside the output window"
    assert not torch.isnan(ybuf[..., yoff:yoff + C]).any(), "NaN left inside the output window"
    return yv.double().cpu()


def groups(t, heads, area=1, rows=None):
    """Logical (B, C, H, W) -> group layout, float64; rows: token indices within the group to keep (None = all)."""
    B, C, H, W = t.shape
    t = t.double().permute(0, 2, 3, 1).reshape(B * area, H * W // area, heads, C // heads).transpose(1, 2)
    return t if rows is None else t[:, :, rows]


def ref(q, k, v, heads, scale, area=1, rows=None):
    """float64 on the queries `rows` of every group: (y, sum P|v|, max |score| terms, sum exp(s - max), max |v|), each in the group
    layout or broadcastable to it."""
    qq, kk, vv = groups(q, heads, area, rows), groups(k, heads, area), groups(v, heads, area)
    s = (qq @ kk.transpose(-1, -2)) * scale
    e = torch.exp(s - s.amax(-1, keepdim=True))
    Lsum = e.sum(-1, keepdim=True)
    P = e / Lsum
    A = (qq.abs() @ kk.abs().transpose(-1, -2)) * scale
    return P @ vv, P @ vv.abs(), A.amax(-1, keepdim=True), Lsum, vv.abs().amax(-2, keepdim=True)


def ulp(v, dtype):
    v = v.abs().to(dtype).double()
    if dtype == torch.float16:
        return torch.clamp(2.0 ** (torch.floor(torch.log2(torch.clamp(v, min=2.0 ** -14))) - 10), min=2.0 ** -24)
    return torch.clamp(2.0 ** (torch.floor(torch.log2(torch.clamp(v, min=2.0 ** -126))) - 23), min=2.0 ** -149)


def data(B, H, W, heads, hd, key):
    g = gen(*key)
    C = heads * hd
    f = lambda s: (torch.randn(B, C, H, W, generator=g) * s).half().float()  # noqa: E731  (f16-representable values)
    return f(1.5), f(1.5), f(1.0)


ONE_HOT_R = {16: 20.0, 32: 20.0, 64: 16.0}  # R^2 (hd - 1) + 8 must be an f16 number: 6008, 12408, 16136


def one_hot_target(Ng, h):
    return (7 * torch.arange(Ng) + 3 + h) % Ng


def one_hot(B, H, W, heads, area, hd, key):
    """q, k, v whose softmax rows are exact one-hot gathers: per query one key scores -8 and every other real key of its group far
    below, a zero-filled padded key would score 0 and win.  Query n of a group gathers key one_hot_target(Ng, h)[n] of that group."""
    R = ONE_HOT_R[hd]
    C, N = heads * hd, H * W
    Ng = N // area
    q = torch.zeros(B, N, C)
    k = torch.zeros(B, N, C)
    bits = 2.0 * ((torch.arange(Ng).view(-1, 1) >> torch.arange(hd - 1).view(1, -1)) & 1).float() - 1.0  # (Ng, hd - 1) distinct +-1 codes
    bias = R * R * (hd - 1) + 8.0  # best real score -8
    assert float(torch.tensor(bias).half()) == bias
    for h in range(heads):
        c0 = h * hd
        for a in range(area):
            sl = slice(a * Ng, (a + 1) * Ng)
            q[:, sl, c0] = 1.0
            q[:, sl, c0 + 1:c0 + hd] = R * bits[one_hot_target(Ng, h)]
            k[:, sl, c0] = -bias
            k[:, sl, c0 + 1:c0 + hd] = R * bits
    v = (torch.randn(B, N, C, generator=gen(*key)) * 4).half().float()
    to4 = lambda t: t.view(B, H, W, C).permute(0, 3, 1, 2).contiguous()  # noqa: E731
    return to4(q), to4(k), to4(v)
