"""-m gpu: ey_deconv2x2 (csrc/segment.hip), the dense k2/s2 transposed convolution with bias, against float64 with the project's
per-element bound: (Cin + 2) u sum|terms| for the fp32 accumulation (u = 2^-24) plus, in f16 storage, one output rounding (2^-11 |y|).
Inputs are drawn representable in the storage type, so the f16 products are exact in fp32.  x and y are channel windows of wider NaN-filled
buffers: only y's window may be written.  A one-hot weight probe must be bit-exact."""
import zlib

import numpy as np
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

import fp64_mask_ref as f64  # noqa: E402

U = 2.0 ** -24
CH = [8, 64, 96, 384]  # 96: the K tail of the 32-wide MFMA step
MAPS = [(1, 1), (3, 5), (17, 9)]
DTYPES = [torch.float32, torch.float16]


class _Holder(nn.Module):
    def __init__(self, deconv):
        super().__init__()
        self.up = deconv
        self._c = {}

    def _packed(self, key, build):
        if key not in self._c:
            self._c[key] = build()
        return self._c[key]


def _rep(a, dt):
    a = a.astype(np.float32)
    return a.astype(np.float16).astype(np.float32) if dt == torch.float16 else a


def _run(x, w, b, dt, lead=8):
    """x [B,Cin,H,W], w [Cin,Cout,2,2], b [Cout] numpy -> (y numpy [B,Cout,2H,2W] fp32, the whole output buffer)."""
    from edge_yolo_amd.nn import _ops
    B, cin, H, W = x.shape
    cout = w.shape[1]
    xb = torch.full((B, H, W, cin + 16), float("nan"), dtype=dt, device="cuda")
    xb[..., lead:lead + cin] = torch.tensor(x).permute(0, 2, 3, 1).to(dt)
    yb = torch.full((B, 2 * H, 2 * W, cout + 16), float("nan"), dtype=dt, device="cuda")
    up = nn.ConvTranspose2d(cin, cout, 2, 2, 0, bias=True)
    up.weight.data = torch.tensor(w)
    up.bias.data = torch.tensor(b)
    out = yb[..., lead:lead + cout].permute(0, 3, 1, 2)
    got = _ops.deconv2x2(_Holder(up), xb[..., lead:lead + cin].permute(0, 3, 1, 2), up, out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    assert bool(torch.isnan(yb[..., :lead]).all()) and bool(torch.isnan(yb[..., lead + cout:]).all()), "channels outside y's window were written"
    return got.float().cpu().numpy(), yb


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f16"])
@pytest.mark.parametrize("hw", MAPS, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("c", CH)
def test_against_fp64(c, hw, dt):
    r = np.random.default_rng([zlib.crc32(repr((c, hw, str(dt))).encode()), 1])
    x = _rep(r.normal(0, 1, (2, c, *hw)), dt)
    w = _rep(r.normal(0, 1, (c, c, 2, 2)) / np.sqrt(c), dt)
    b = r.normal(0, 0.5, c).astype(np.float32)
    got, _ = _run(x, w, b, dt)
    y, mag = f64.deconv64(x, w, b)
    bound = (c + 2) * U * mag + (2.0 ** -11 * np.abs(y) if dt == torch.float16 else 0.0)
    err = np.abs(got - y)
    print(f"C{c} {hw} {dt}: max err / bound = {float((err / bound).max()):.3f}")
    assert np.isfinite(got).all() and (err <= bound).all(), f"{int((err > bound).sum())} elements outside the bound, worst ratio {float((err / bound).max()):.2f}"


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f16"])
@pytest.mark.parametrize("c", [8, 96])
def test_one_hot_weight_is_bit_exact(c, dt):
    """W[ci, co, di, dj] = 1 where ci == perm(co, di, dj), else 0, zero bias: every output is a copy of one input element."""
    r = np.random.default_rng([c, 5])
    x = _rep(r.normal(0, 1, (2, c, 3, 5)), dt)
    w = np.zeros((c, c, 2, 2), np.float32)
    src = np.zeros((c, 2, 2), np.int64)
    for co in range(c):
        for d in range(4):
            src[co, d // 2, d % 2] = (5 * co + 3 * d + 1) % c
            w[src[co, d // 2, d % 2], co, d // 2, d % 2] = 1.0
    got, _ = _run(x, w, np.zeros(c, np.float32), dt)
    want = np.zeros((2, c, 6, 10), np.float32)
    for di in range(2):
        for dj in range(2):
            want[:, :, di::2, dj::2] = x[:, src[:, di, dj]]
    np.testing.assert_array_equal(got, want)


def test_refusals():
    from edge_yolo_amd.nn import _ops
    up = nn.ConvTranspose2d(12, 16, 2, 2, 0)
    x = torch.zeros(1, 2, 2, 12, device="cuda").permute(0, 3, 1, 2)
    with pytest.raises(NotImplementedError):
        _ops.deconv2x2(_Holder(up), x, up)
    up = nn.ConvTranspose2d(8, 8, 3, 2, 0)
    with pytest.raises(NotImplementedError):
        _ops.deconv2x2(_Holder(up), torch.zeros(1, 2, 2, 8, device="cuda").permute(0, 3, 1, 2), up)
