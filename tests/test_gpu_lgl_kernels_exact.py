"""-m gpu: the small kernels of the LGL block (csrc/lgl.hip) against float64, in fp32 and f16 storage: depthwise 9x9 / 3x3 with the gate
and residual epilogues, the element-wise gate, the exact GELU, the per-channel CMlp, LayerNorm over channels with and without the
ceil-mode 2x2 average pool, and the transposed 2x2 un-pool + LayerNorm on even maps and through the bilinear resize of odd ones.

Inputs and outputs are channel windows of wider NaN-filled buffers: nothing outside the output window may be written, nothing inside may
stay NaN.  Bounds are per element, from each kernel's operation count: u = 2^-24 per fp32 operation (a sum of K terms: K u sum|terms|),
v_exp_f32 / v_rcp_f32 within 2^-22, erff within 2^-21, one output rounding (ulp of the storage type), propagated through the gate
(sigmoid' <= 1/4), the GELU (|gelu'| <= 1.13) and the LayerNorm.  Maps 1x1, 1x9, 5x7, 9x16, 17x33 (narrower than the 9-tap support, odd
sizes for the pool and un-pool), C 8, 16, 24, 128 (and 384 for the LayerNorms).  Bit-exact probes: a single non-zero depthwise tap is a
shift; a constant pixel normalises to exactly the bias; power-of-two un-pool weights make the fused kernel equal LayerNorm of the
materialised map bit for bit; the CMlp border is told apart from a pad-before-affine reference."""
import math
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
EXP_REL = RCP_REL = 2.0 ** -22
ERF_REL = 2.0 ** -21
SHAPES = [(2, 8, 1, 1), (1, 16, 1, 9), (2, 24, 5, 7), (1, 128, 9, 16), (1, 16, 17, 33)]
DTYPES = [torch.float32, torch.float16]
WORST = {}


def _L():
    from edge_yolo_amd import _lib as L
    return L


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _rand(shape, key, s=1.0):
    return (torch.randn(*shape, generator=_gen(*key)) * s).half().double()  # f16-representable, as float64


def _window(vals, off, pad, dtype):
    """(buffer, NHWC view) of logical (B,C,H,W) vals at channel offset `off` of a (off + C + pad)-channel NaN-filled device buffer."""
    B, C, H, W = vals.shape
    buf = torch.full((B, H, W, off + C + pad), float("nan"), dtype=dtype, device="cuda")
    buf[..., off:off + C] = vals.permute(0, 2, 3, 1).to(device="cuda", dtype=dtype)
    return buf, buf.permute(0, 3, 1, 2)[:, off:off + C]


def _out(B, C, H, W, dtype, off=8, pad=8):
    buf = torch.full((B, H, W, off + C + pad), float("nan"), dtype=dtype, device="cuda")
    return buf, buf.permute(0, 3, 1, 2)[:, off:off + C], off


def _fetch(buf, view, off):
    torch.cuda.synchronize()
    C = view.shape[1]
    assert torch.isnan(buf[..., :off]).all() and torch.isnan(buf[..., off + C:]).all(), "writes outside the output window"
    assert not torch.isnan(buf[..., off:off + C]).any(), "NaN left inside the output window"
    return view.double().cpu()


def _ulp(v, dtype):
    v = v.abs().to(dtype).double()
    if dtype == torch.float16:
        return torch.clamp(2.0 ** (torch.floor(torch.log2(torch.clamp(v, min=2.0 ** -14))) - 10), min=2.0 ** -24)
    return torch.clamp(2.0 ** (torch.floor(torch.log2(torch.clamp(v, min=2.0 ** -126))) - 23), min=2.0 ** -149)


def _grade(case, fam, got, want, E, dtype):
    bnd = 1.05 * E + _ulp(want, dtype) + 2.0 ** -40
    assert torch.isfinite(got).all(), f"{case}: non-finite output"
    r = float(((got - want).abs() / bnd).max())
    print(f"[fp64] {case} max err/bound {r:.3f}")
    WORST[fam] = max(WORST.get(fam, (0.0, "")), (r, case))
    assert r <= 1.0, f"{case}: max err/bound {r:.3f}"
    return bnd


def _cs(v):
    from edge_yolo_amd import _lib as L
    return L.cstride(v)


def _code(dtype):
    return _L().dtype_code(dtype)


# ---- error models
def _gate(x, g, dg):
    """(y, E) of y = x + x (sigmoid(g) - 1/2) with g known to dg: sigmoid = rcp(1 + exp(-g)), then subtract, multiply, add."""
    s = torch.sigmoid(g)
    ds = s * (1 - s) * dg + s * ((1 - s) * (4 * U * g.abs() + EXP_REL) + U + RCP_REL)
    y = x + x * (s - 0.5)
    return y, x.abs() * (ds + 3 * U * (s - 0.5).abs()) + 2 * U * y.abs()


def _gelu(x, dx):
    """(y, E) of the exact GELU evaluated as 0.5 x (1 + erff(x * 0.70710678f)) with x known to dx."""
    z = x / math.sqrt(2.0)
    erf = torch.erf(z)
    e_erf = erf.abs() * ERF_REL + 2 / math.sqrt(math.pi) * torch.exp(-z * z) * z.abs() * 2 * U
    y = 0.5 * x * (1 + erf)
    return y, 1.13 * dx + 0.5 * x.abs() * (e_erf + U * (1 + erf).abs()) + 2 * U * y.abs()


def _ln(x, dx, gamma, beta, eps):
    """(y, E) of LayerNorm over dim 1 of (B,C,H,W) x known to dx: two-pass fp32 mean and variance in any summation order."""
    C = x.shape[1]
    mean = x.mean(1, keepdim=True)
    dmean = dx.mean(1, keepdim=True) + U * x.abs().sum(1, keepdim=True) + U * mean.abs()
    d = x - mean
    dd = dx + dmean + U * d.abs()
    var = (d * d).mean(1, keepdim=True)
    dvar = 2 * (d.abs() * dd).mean(1, keepdim=True) + (C + 3) * U * var
    rstd = 1 / torch.sqrt(var + eps)
    rel = 0.5 * dvar / (var + eps) + 4 * U
    g, b = gamma.view(1, -1, 1, 1), beta.view(1, -1, 1, 1)
    y = d * rstd * g + b
    return y, g.abs() * rstd * (dd + d.abs() * (rel + 2 * U)) + U * y.abs()


# ---- depthwise + epilogue
def _dw_run(x, w, bias, k, mode, dtype):
    L = _L()
    B, C, H, W = x.shape
    _, xv = _window(x, 8, 8, dtype)
    wk = w.view(C, k, k).permute(1, 2, 0).contiguous().to(device="cuda", dtype=dtype)
    bd = bias.float().cuda() if bias is not None else None
    ybuf, yv, off = _out(B, C, H, W, dtype)
    L.check(L.lib().ey_dwconv_gate(_code(dtype), B, H, W, C, k, mode, xv.data_ptr(), _cs(xv), wk.data_ptr(), bd.data_ptr() if bd is not None else None,
                                   yv.data_ptr(), _cs(yv), L.stream()), "ey_dwconv_gate")
    return _fetch(ybuf, yv, off)


@pytest.mark.parametrize("B,C,H,W", SHAPES)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16"])
@pytest.mark.parametrize("k,mode", [(9, 1), (9, 0), (3, 2)])
def test_dwconv_gate_bounded(B, C, H, W, dtype, k, mode):
    x = _rand((B, C, H, W), ("dwx", B, C, H, W), 1.5)
    w = _rand((C, 1, k, k), ("dww", C, k), 1.0 / k)
    bias = _rand((C,), ("dwb", C), 0.3).float().double()
    got = _dw_run(x, w, bias, k, mode, dtype)
    g = F.conv2d(x, w, bias, padding=k // 2, groups=C)
    G = F.conv2d(x.abs(), w.abs(), bias.abs(), padding=k // 2, groups=C)
    dg = (k * k + 2) * U * G
    if mode == 1:
        y, E = _gate(x, g, dg)
    elif mode == 2:
        y, E = x + g, dg + U * (x + g).abs()
    else:
        y, E = g, dg
    _grade(f"dw{k} mode{mode} {dtype} B{B} C{C} {H}x{W}", f"dw{k} mode{mode}", got, y, E, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16"])
@pytest.mark.parametrize("k,ty,tx", [(9, 0, 0), (9, 8, 3), (9, 4, 4), (3, 2, 0)])
def test_dwconv_single_tap_is_a_shift(dtype, k, ty, tx):
    B, C, H, W = 2, 16, 5, 7
    x = _rand((B, C, H, W), ("tap", k, ty, tx), 2.0)
    w = torch.zeros(C, 1, k, k, dtype=torch.float64)
    w[:, 0, ty, tx] = 1.0
    got = _dw_run(x, w, None, k, 0, dtype)
    want = F.conv2d(x, w, None, padding=k // 2, groups=C)  # exact: one product by 1 and zeros
    assert torch.equal(got, want)


@pytest.mark.parametrize("B,C,H,W", SHAPES + [(1, 20, 3, 5)])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16"])
def test_sigmoid_gate_and_gelu_bounded(B, C, H, W, dtype):
    L = _L()
    x = _rand((B, C, H, W), ("gx", B, C, H, W), 2.0)
    g = _rand((B, C, H, W), ("gg", B, C, H, W), 3.0)
    _, xv = _window(x, 8, 8, dtype)
    _, gv = _window(g, 3, 5, dtype)
    ybuf, yv, off = _out(B, C, H, W, dtype, off=5, pad=3)
    L.check(L.lib().ey_sigmoid_gate(_code(dtype), B, H, W, C, xv.data_ptr(), _cs(xv), gv.data_ptr(), _cs(gv), yv.data_ptr(), _cs(yv), L.stream()), "gate")
    y, E = _gate(x, g, torch.zeros_like(g))
    _grade(f"gate {dtype} B{B} C{C} {H}x{W}", "gate", _fetch(ybuf, yv, off), y, E, dtype)
    x5 = _rand((B, C, H, W), ("gelu", B, C, H, W), 2.5)  # reaches |x| > 6: 1 + erf cancels
    _, xv = _window(x5, 8, 8, dtype)
    ybuf, yv, off = _out(B, C, H, W, dtype, off=5, pad=3)
    L.check(L.lib().ey_gelu(_code(dtype), B, H, W, C, xv.data_ptr(), _cs(xv), yv.data_ptr(), _cs(yv), L.stream()), "gelu")
    y, E = _gelu(x5, torch.zeros_like(x5))
    assert torch.allclose(y, F.gelu(x5), rtol=1e-12, atol=1e-15)
    _grade(f"gelu {dtype} B{B} C{C} {H}x{W}", "gelu", _fetch(ybuf, yv, off), y, E, dtype)


# ---- CMlp
def _cmlp_ref(x, sc, sh, w1, b1, w2, b2, r, pad_after=True):
    """float64 (o, E): fc2(GELU(fc1(a))), a = sc x + sh zero-padded AFTER the affine (pad_after) or computed on the zero-padded x."""
    B, C, H, W = x.shape
    aff = lambda t: t * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1)  # noqa: E731
    a = F.pad(aff(x), (1, 1, 1, 1)) if pad_after else aff(F.pad(x, (1, 1, 1, 1)))
    da = U * a.abs()
    s = F.conv2d(a, w1, b1, groups=C)
    ds = F.conv2d(da, w1.abs(), None, groups=C) + 10 * U * F.conv2d(a.abs(), w1.abs(), b1.abs(), groups=C)
    h, dh = _gelu(s, ds)
    o = F.conv2d(h, w2, b2, padding=1, groups=C)
    do = F.conv2d(dh, w2.abs(), None, padding=1, groups=C) + (9 * r + 1) * U * F.conv2d(h.abs(), w2.abs(), b2.abs(), padding=1, groups=C)
    return o, do


def _cmlp_run(x, sc, sh, w1, b1, w2, b2, r, gate, dtype):
    L = _L()
    B, C, H, W = x.shape
    _, xv = _window(x, 8, 8, dtype)
    f = lambda t: t.float().contiguous().cuda()  # noqa: E731
    d = [f(sc), f(sh), f(w1.view(C, r, 9).permute(1, 2, 0)), f(b1.view(C, r).t()), f(w2.view(C, r, 9).permute(1, 2, 0)), f(b2)]
    ybuf, yv, off = _out(B, C, H, W, dtype)
    L.check(L.lib().ey_cmlp(_code(dtype), B, H, W, C, r, gate, xv.data_ptr(), _cs(xv), *[t.data_ptr() for t in d], yv.data_ptr(), _cs(yv), L.stream()), "ey_cmlp")
    return _fetch(ybuf, yv, off)


def _cmlp_data(C, r, key):
    f32 = lambda t: t.float().double()  # noqa: E731  (the kernel's weights are fp32)
    return (f32(_rand((C,), (key, "sc"), 0.3) + 1.0), f32(_rand((C,), (key, "sh"), 0.5)), f32(_rand((C * r, 1, 3, 3), (key, "w1"), 0.4)),
            f32(_rand((C * r,), (key, "b1"), 0.3)), f32(_rand((C, r, 3, 3), (key, "w2"), 0.25)), f32(_rand((C,), (key, "b2"), 0.3)))


@pytest.mark.parametrize("B,C,H,W", SHAPES)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16"])
@pytest.mark.parametrize("r,gate", [(4, 1), (4, 0), (2, 1)])
def test_cmlp_bounded(B, C, H, W, dtype, r, gate):
    x = _rand((B, C, H, W), ("cmx", B, C, H, W), 1.5)
    p = _cmlp_data(C, r, ("cm", C, r))
    got = _cmlp_run(x, *p, r, gate, dtype)
    o, do = _cmlp_ref(x, *p, r)
    y, E = _gate(x, o, do) if gate else (o, do)
    bnd = _grade(f"cmlp r{r} gate{gate} {dtype} B{B} C{C} {H}x{W}", f"cmlp gate{gate}", got, y, E, dtype)
    # the test tells the two paddings apart: folding the affine into the weights (= padding before it) differs at the border by far
    # more than the bound, and the kernel is not that
    o2, _ = _cmlp_ref(x, *p, r, pad_after=False)
    y2 = _gate(x, o2, do)[0] if gate else o2
    if dtype == torch.float32:
        assert float(((y2 - y).abs() / bnd).max()) > 100.0
        assert float(((got - y2).abs() / bnd).max()) > 100.0
        if H > 2 and W > 2:  # the interior (receptive field inside the map) does not see the padding
            assert torch.equal(y2[:, :, 2:-2, 2:-2], y[:, :, 2:-2, 2:-2])


# ---- LayerNorm (+ pool)
def _ln_run(x, gamma, beta, eps, pool, dtype, xoff=8):
    L = _L()
    B, C, H, W = x.shape
    _, xv = _window(x, xoff, 8, dtype)
    gd, bd = gamma.float().cuda(), beta.float().cuda()
    Ho, Wo = ((H + 1) // 2, (W + 1) // 2) if pool else (H, W)
    ybuf, yv, off = _out(B, C, Ho, Wo, dtype, off=xoff)
    L.check(L.lib().ey_layernorm_channels(_code(dtype), B, H, W, C, eps, pool, xv.data_ptr(), _cs(xv), gd.data_ptr(), bd.data_ptr(), yv.data_ptr(), _cs(yv),
                                          L.stream()), "ey_layernorm_channels")
    return _fetch(ybuf, yv, off)


def _ceil_pool(y, E):
    """AvgPool2d(2, 2, ceil_mode=True): partial windows divide by their in-bounds count; the sum of <= 4 fp32 terms adds 4 u."""
    cnt = F.avg_pool2d(torch.ones_like(y), 2, 2, ceil_mode=True, count_include_pad=False)
    p = F.avg_pool2d(y, 2, 2, ceil_mode=True, count_include_pad=False)
    a = F.avg_pool2d(y.abs(), 2, 2, ceil_mode=True, count_include_pad=False)
    assert float(cnt.min()) == 1.0
    return p, F.avg_pool2d(E, 2, 2, ceil_mode=True, count_include_pad=False) + 4 * U * a


LN_SHAPES = SHAPES + [(1, 384, 3, 5), (2, 64, 2, 3), (1, 256, 5, 4)]


@pytest.mark.parametrize("B,C,H,W", LN_SHAPES)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16"])
@pytest.mark.parametrize("pool", [0, 1])
def test_layernorm_bounded(B, C, H, W, dtype, pool):
    x = _rand((B, C, H, W), ("lnx", B, C, H, W), 2.0) + _rand((B, 1, H, W), ("lnm", B, H, W), 3.0)
    x = x.half().double()
    gamma = (_rand((C,), ("lng", C), 0.3) + 1.0).float().double()
    beta = _rand((C,), ("lnb", C), 0.5).float().double()
    for xoff in (8, 4):  # 4: windows the 16-byte path cannot take
        got = _ln_run(x, gamma, beta, 1e-5, pool, dtype, xoff)
        y, E = _ln(x, torch.zeros_like(x), gamma, beta, float(np.float32(1e-5)))
        if pool:
            y, E = _ceil_pool(y, E)
            assert tuple(y.shape[2:]) == ((H + 1) // 2, (W + 1) // 2)
        _grade(f"ln pool{pool} {dtype} B{B} C{C} {H}x{W} off{xoff}", f"layernorm pool{pool}", got, y, E, dtype)


@pytest.mark.parametrize("C", [8, 24, 128, 384])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16"])
@pytest.mark.parametrize("pool", [0, 1])
def test_layernorm_constant_pixel_is_the_bias(C, dtype, pool):
    B, H, W = 2, 5, 7
    x = (torch.arange(B * H * W, dtype=torch.float64).view(B, 1, H, W) % 7 - 3) * 0.5 * torch.ones(1, C, 1, 1, dtype=torch.float64)
    gamma = (_rand((C,), ("cg", C), 0.3) + 1.0).float().double()
    beta = _rand((C,), ("cb", C), 0.5)  # f16 numbers: the average of up to four equal values is exact
    got = _ln_run(x, gamma, beta, 1e-5, pool, dtype)
    assert torch.equal(got, beta.view(1, C, 1, 1).expand_as(got))


# ---- un-pool + LayerNorm
def _src_index(o, n_in, n_out):
    """ATen area_pixel_compute_source_index (align_corners=False) in fp32, as the kernel evaluates it."""
    s = np.float32(np.float32(n_in) / np.float32(n_out)) * (np.float32(o) + np.float32(0.5)) - np.float32(0.5)
    s = np.maximum(s, np.float32(0)).astype(np.float32)
    i0 = np.minimum(s.astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    return i0, i1, (s - i0.astype(np.float32)).astype(np.float64)


def _unpool_ref(t, w, H, W):
    """float64 (U resized to H x W, E): ConvTranspose2d(k 2, s 2, depthwise) then the bilinear resize when the sizes differ."""
    Up = F.conv_transpose2d(t, w, None, stride=2, groups=t.shape[1])
    dU = U * Up.abs()
    if tuple(Up.shape[2:]) == (H, W):
        return Up, dU
    y0, y1, ly = _src_index(np.arange(H), Up.shape[2], H)
    x0, x1, lx = _src_index(np.arange(W), Up.shape[3], W)
    ly, lx = torch.from_numpy(ly).view(1, 1, H, 1), torch.from_numpy(lx).view(1, 1, 1, W)
    # the kernel's 1 - l is one more fp32 rounding of an exact fp32 l
    g = lambda a, yy, xx: a[:, :, torch.from_numpy(yy)][:, :, :, torch.from_numpy(xx)]  # noqa: E731
    wy0, wx0 = (1 - ly).float().double(), (1 - lx).float().double()
    val = wy0 * (wx0 * g(Up, y0, x0) + lx * g(Up, y0, x1)) + ly * (wx0 * g(Up, y1, x0) + lx * g(Up, y1, x1))
    mag = wy0 * (wx0 * g(Up.abs(), y0, x0) + lx * g(Up.abs(), y0, x1)) + ly * (wx0 * g(Up.abs(), y1, x0) + lx * g(Up.abs(), y1, x1))
    return val, 7 * U * mag


def _unpool_run(t, w, gamma, beta, eps, H, W, dtype):
    L = _L()
    B, C, Hs, Ws = t.shape
    _, tv = _window(t, 8, 8, dtype)
    wd = w.view(C, 2, 2).permute(1, 2, 0).float().contiguous().cuda()
    gd, bd = gamma.float().cuda(), beta.float().cuda()
    ybuf, yv, off = _out(B, C, H, W, dtype)
    L.check(L.lib().ey_unpool2_layernorm(_code(dtype), B, Hs, Ws, H, W, C, eps, tv.data_ptr(), _cs(tv), wd.data_ptr(), gd.data_ptr(), bd.data_ptr(),
                                         yv.data_ptr(), _cs(yv), L.stream()), "ey_unpool2_layernorm")
    return _fetch(ybuf, yv, off)


@pytest.mark.parametrize("B,C,H,W", SHAPES + [(1, 384, 3, 5), (2, 64, 2, 3), (1, 32, 6, 10), (1, 32, 6, 7), (1, 32, 5, 8)])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16"])
def test_unpool_layernorm_bounded(B, C, H, W, dtype):
    Hs, Ws = (H + 1) // 2, (W + 1) // 2
    t = _rand((B, C, Hs, Ws), ("upt", B, C, H, W), 2.0)
    w = _rand((C, 1, 2, 2), ("upw", C), 0.7).float().double()
    gamma = (_rand((C,), ("upg", C), 0.3) + 1.0).float().double()
    beta = _rand((C,), ("upb", C), 0.5).float().double()
    got = _unpool_run(t, w, gamma, beta, 1e-5, H, W, dtype)
    v, dv = _unpool_ref(t, w, H, W)
    assert tuple(v.shape) == (B, C, H, W)
    if (2 * Hs, 2 * Ws) != (H, W):  # the reference's own resize agrees with the restated one
        want = F.interpolate(F.conv_transpose2d(t, w, None, stride=2, groups=C), size=(H, W), mode="bilinear", align_corners=False)
        # (the restated weights are fp32 like the kernel's and ATen's fp32 path: each is within 3 u * source coordinate of the exact one)
        tol = 12 * U * 2 * max(Hs, Ws) * float(want.abs().max())
        assert float((v - want).abs().max()) <= tol
    y, E = _ln(v, dv, gamma, beta, float(np.float32(1e-5)))
    _grade(f"unpool+ln {dtype} B{B} C{C} {H}x{W}", "unpool even" if (2 * Hs, 2 * Ws) == (H, W) else "unpool odd", got, y, E, dtype)


@pytest.mark.parametrize("C", [16, 24, 128])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16"])
def test_unpool_power_of_two_weights_equal_layernorm_of_the_map(C, dtype):
    """With weights +-2^k the un-pooled map is exact, so the fused kernel must equal ey_layernorm_channels on the materialised map bit
    for bit (same lanes, same sums)."""
    B, Hs, Ws = 2, 3, 4
    t = _rand((B, C, Hs, Ws), ("p2t", C), 2.0)
    e = torch.randint(-2, 3, (C, 1, 2, 2), generator=_gen("p2e", C)).double()
    w = torch.sign(_rand((C, 1, 2, 2), ("p2s", C)) + 1e-3) * 2.0 ** e
    gamma = (_rand((C,), ("p2g", C), 0.3) + 1.0).float().double()
    beta = _rand((C,), ("p2b", C), 0.5).float().double()
    got = _unpool_run(t, w, gamma, beta, 1e-5, 2 * Hs, 2 * Ws, dtype)
    Up = F.conv_transpose2d(t, w, None, stride=2, groups=C)
    assert torch.equal(Up.to(dtype).double(), Up)
    assert torch.equal(got, _ln_run(Up, gamma, beta, 1e-5, 0, dtype))


def test_refusals_launch_nothing():
    L = _L()
    x = torch.zeros(1, 5, 5, 400, dtype=torch.float16, device="cuda")
    p, st = x.data_ptr(), L.stream()
    lib = L.lib()
    assert lib.ey_dwconv_gate(L.F16, 1, 5, 5, 16, 5, 0, p, 16, p, None, p, 16, st) == -2      # k = 5: ey_dwconv's
    assert lib.ey_dwconv_gate(L.F16, 1, 5, 5, 12, 9, 0, p, 16, p, None, p, 16, st) == -2      # C % 8
    assert lib.ey_dwconv_gate(L.F16, 1, 5, 5, 16, 9, 3, p, 16, p, None, p, 16, st) == -1      # mode
    assert lib.ey_cmlp(L.F16, 1, 5, 5, 16, 9, 0, p, 16, None, None, p, p, p, p, p, 16, st) == -2  # r > 8
    assert lib.ey_layernorm_channels(L.F16, 1, 5, 5, 392, 1e-5, 0, p, 400, p, p, p, 400, st) == -2  # C > 384
    assert lib.ey_layernorm_channels(L.F16, 1, 5, 5, 12, 1e-5, 0, p, 16, p, p, p, 16, st) == -2
    assert lib.ey_unpool2_layernorm(L.F16, 1, 2, 2, 5, 5, 16, 1e-5, p, 16, p, p, p, p, 16, st) == -1  # 2x2 does not un-pool to 5x5
    assert lib.ey_gelu(L.F16, 1, 5, 5, 16, p, 8, p, 16, st) == -1                              # cstride < C
    torch.cuda.synchronize()
    assert float(x.abs().max()) == 0.0


def test_zz_worst_report():
    for fam, (r, case) in sorted(WORST.items()):
        print(f"[fp64] worst {fam}: err/bound {r:.3f} at {case}")
