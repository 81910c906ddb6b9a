"""-m gpu: ey_dysample (csrc/dysample.hip) against the float64 restatement of tests/fp64_dysample_ref.py, in fp32 and f16 storage.

Input and output are channel windows of wider NaN-filled buffers: nothing outside the output window may be written, nothing inside may
stay NaN (and the kernel may not read a channel outside the input window: a NaN there would reach the offsets).  The bound is per
element and comes from the operation count, u = 2^-24 per fp32 operation:
  offsets   lin = W.x + b is a sum of C + 1 terms: (C + 2) u sum|terms| (f16 products are exact in fp32, fp32 ones round once each);
            without scope O = 0.25 lin + init_pos: 0.25 d_lin + u |O|; with scope the second GEMM the same way, sigmoid = rcp(1 + exp(-s))
            with v_exp_f32 / v_rcp_f32 within 2^-22 (sigmoid' <= 1/4 through s (1 - s)), two products and the sum;
  position  w + O_x and h + O_y round once each: u (|O| + max(H, W)); the clamp is 1-Lipschitz;
  sampler   the bilinear interpolant is continuous across cell borders and, inside a cell, changes per pixel of displacement by at most the
            largest difference between adjacent map values of that cell; a position known to d therefore moves the sample by at most
            d x (largest adjacent difference over the cell and the cells around it: a 5x5 window of the difference map);
  blend     four weights of two roundings each, four products, three sums: 8 u max|corner|;
  output    one rounding to the storage type (_grade adds the ulp).
Derived, not measured.  Maps 1x1 (every read clamped), 1x9, 5x7, 9x16, 17x33 (pixel-tile tails), B = 2; C 16 with 2 groups, 32 and 96 with 4
(96: K tail of the 32-wide MFMA step), 128 with 8, 768; with and without scope; one 'pl'-expanded weight.  Bit-exact probes: zero weights
(offsets exactly +-0.25) on dyadic data, and integer offsets (an exact border-clamped shift).  Refusals leave the output untouched."""
import zlib

import pytest
import torch

import fp64_dysample_ref as ref

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
EXP_REL = RCP_REL = 2.0 ** -22
DTYPES = [torch.float32, torch.float16]
# (C, groups, B, H, W)
SHAPES = [(16, 2, 1, 1, 1), (32, 4, 1, 1, 9), (96, 4, 2, 5, 7), (128, 8, 1, 9, 16), (768, 4, 1, 17, 33), (32, 4, 2, 17, 33), (96, 4, 1, 1, 1), (16, 2, 1, 9, 16),
          (128, 8, 2, 5, 7), (768, 4, 1, 1, 9)]
WORST = {}


def _L():
    from edge_yolo_amd import _lib as L
    return L


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _rand(shape, key, dtype, s=1.0):
    """Values representable in the storage type, as float64."""
    return (torch.randn(*shape, generator=_gen(*key)) * s).to(dtype).double()


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


def _run(x, w, b, s, pos, groups, dtype, x_off=8, y_off=8, expect=0):
    """ey_dysample on windows; returns (y buffer, y view, y offset, return code).  x, w, s: float64 values representable in dtype."""
    L = _L()
    B, C, H, W = x.shape
    _, xv = _window(x, x_off, 8, dtype)
    wd = w.to(device="cuda", dtype=dtype).contiguous()
    sd = None if s is None else s.to(device="cuda", dtype=dtype).contiguous()
    bd, pd = b.float().cuda().contiguous(), pos.float().cuda().contiguous()
    ybuf, yv, off = _out(B, C, 2 * H, 2 * W, dtype, off=y_off)
    rc = L.lib().ey_dysample(L.dtype_code(dtype), B, H, W, C, 2, groups, xv.data_ptr(), L.cstride(xv), wd.data_ptr(), bd.data_ptr(),
                             None if sd is None else sd.data_ptr(), pd.data_ptr(), yv.data_ptr(), L.cstride(yv), L.stream())
    torch.cuda.synchronize()
    assert rc == expect, (rc, L.lib().ey_last_error())
    return ybuf, yv, off


def _init_pos(groups):
    from edge_yolo_amd.nn.modules import DySample
    return DySample(8 * groups, 2, "lp", groups).init_pos.flatten().double()


def _bound(x, w, b, s, pos, groups):
    """(y, E): the float64 result and the per-element bound of the module docstring, without the output rounding."""
    B, C, H, W = x.shape
    o, lin, sc, mag, smag = ref.offsets(x, w, b, s, pos, parts=True)
    d_lin = (C + 2) * U * mag
    if s is None:
        d_o = 0.25 * d_lin + U * o.abs()
    else:
        sg = torch.sigmoid(sc)
        d_sc = (C + 1) * U * smag
        d_sg = sg * (1 - sg) * d_sc + sg * ((1 - sg) * (4 * U * sc.abs() + EXP_REL) + U + RCP_REL)
        d_o = 0.5 * (d_lin * sg + lin.abs() * d_sg) + 2 * U * (lin * sg * 0.5).abs() + U * o.abs()
    d_pos = d_o + U * (o.abs() + max(H, W))
    y, y0, x0, vmax = ref.sample(x, o, groups, parts=True)
    dh, dv = torch.zeros_like(x), torch.zeros_like(x)
    dh[..., :-1] = (x[..., 1:] - x[..., :-1]).abs()
    dv[..., :-1, :] = (x[..., 1:, :] - x[..., :-1, :]).abs()
    slope = torch.nn.functional.max_pool2d(torch.maximum(dh, dv), 5, 1, 2)  # largest adjacent difference within two pixels
    d = d_pos.view(B, 2, groups, 2, 2, H, W)
    E = ref.per_group_to_out(d[:, 0] + d[:, 1], C) * ref.gather_at(slope, y0, x0, groups) + 8 * U * vmax
    return y, E


def _case(C, groups, B, H, W, dtype, scope, key):
    x = _rand((B, C, H, W), (key, "x"), dtype)
    w = _rand((8 * groups, C), (key, "w"), dtype, 2.0 / C ** 0.5)  # offsets of about half a pixel rms, two and more at the tails
    b = _rand((8 * groups,), (key, "b"), torch.float32, 0.5)
    s = _rand((8 * groups, C), (key, "s"), dtype, 1.0 / C ** 0.5) if scope else None
    return x, w, b, s


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "f16"])
@pytest.mark.parametrize("scope", [False, True], ids=["plain", "scope"])
@pytest.mark.parametrize("shape", SHAPES, ids=["C{}g{}_b{}_{}x{}".format(*s) for s in SHAPES])
def test_dysample_vs_fp64(shape, scope, dtype):
    C, groups, B, H, W = shape
    x, w, b, s = _case(C, groups, B, H, W, dtype, scope, shape)
    pos = _init_pos(groups)
    ybuf, yv, off = _run(x, w, b, s, pos, groups, dtype)
    want, E = _bound(x, w, b, s, pos, groups)
    assert float((ref.offsets(x, w, b, s, pos) - pos.view(1, -1, 1, 1)).abs().max()) > (0.2 if H * W == 1 else 1.0)  # samples leave their cell
    name = f"dysample C{C} G{groups} B{B} {H}x{W} {'scope ' if scope else ''}{'f16' if dtype == torch.float16 else 'fp32'}"
    _grade(name, ("scope " if scope else "plain ") + ("f16" if dtype == torch.float16 else "fp32"), _fetch(ybuf, yv, off), want, E, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "f16"])
def test_pl_expanded_weight_vs_fp64(dtype):
    """A 'pl' module's (2G, C/4) weights through pl_to_dense: three of every four columns are zero."""
    from edge_yolo_amd.nn.modules.dysample import pl_to_dense
    C, groups, B, H, W = 32, 4, 2, 5, 7
    x = _rand((B, C, H, W), ("pl", "x"), dtype)
    w, b = pl_to_dense(_rand((2 * groups, C // 4), ("pl", "w"), dtype, 4.0 / C ** 0.5), _rand((2 * groups,), ("pl", "b"), torch.float32, 0.5))
    s, _ = pl_to_dense(_rand((2 * groups, C // 4), ("pl", "s"), dtype, 2.0 / C ** 0.5))
    assert float((w == 0).double().mean()) >= 0.75
    pos = _init_pos(groups)
    ybuf, yv, off = _run(x, w, b, s, pos, groups, dtype)
    want, E = _bound(x, w, b, s, pos, groups)
    _grade(f"dysample pl-expanded C{C} {'f16' if dtype == torch.float16 else 'fp32'}", "pl", _fetch(ybuf, yv, off), want, E, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "f16"])
@pytest.mark.parametrize("shape", [(16, 2, 1, 1, 1), (96, 4, 2, 5, 7), (128, 8, 1, 17, 33)], ids=["1x1", "5x7", "17x33"])
def test_zero_weights_bit_exact(shape, dtype):
    """Zero offset weight and bias: offsets are exactly +-0.25, the blend weights 9/16, 3/16, 3/16, 1/16; on multiples of 1/8 in [-4, 4]
    every product and sum is exact in fp32 and representable in f16, so the kernel equals the exact (float64, CPU torch) result bit for
    bit; on the 1x1 map every read is clamped and the output is the input pixel four times."""
    C, groups, B, H, W = shape
    x = torch.randint(-32, 33, (B, C, H, W), generator=_gen("zero", shape)).double() / 8
    w, b, pos = torch.zeros(8 * groups, C, dtype=torch.float64), torch.zeros(8 * groups, dtype=torch.float64), _init_pos(groups)
    ybuf, yv, off = _run(x, w, b, None, pos, groups, dtype)
    got = _fetch(ybuf, yv, off)
    want = ref.dysample(x, w, b, None, pos, groups)
    assert torch.equal(want.to(dtype).double(), want)
    assert torch.equal(got, want)
    if H * W == 1:
        assert torch.equal(got, x.expand(B, C, 2, 2))


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "f16"])
@pytest.mark.parametrize("groups,C", [(2, 16), (4, 96), (8, 128)])
def test_integer_offsets_are_a_clamped_shift(groups, C, dtype):
    """Zero weight and bias = 4 (k - init_pos): 0.25 bias + init_pos = k exactly, every output pixel is x at (clamp(h + ky), clamp(w + kx))
    bit for bit.  Each (group, output sub-pixel) has its own shift in [-9, 9]^2: on a 5x7 map the samples leave on every side."""
    B, H, W = 2, 5, 7
    x = _rand((B, C, H, W), ("shift", C), dtype)
    pos = _init_pos(groups)
    k = torch.randint(-9, 10, (8 * groups,), generator=_gen("k", groups)).double()
    k[:4] = torch.tensor([-9.0, 9.0, 0.0, 1.0])  # x of group 0: past the left and the right edge
    k[4 * groups:4 * groups + 4] = torch.tensor([9.0, -9.0, -1.0, 0.0])  # y of group 0: past the bottom and the top edge
    b = 4 * (k - pos)
    w = torch.zeros(8 * groups, C, dtype=torch.float64)
    ybuf, yv, off = _run(x, w, b, None, pos, groups, dtype)
    got = _fetch(ybuf, yv, off)
    want = torch.empty(B, C, 2 * H, 2 * W, dtype=torch.float64)
    cg = C // groups
    hh, ww = torch.arange(H), torch.arange(W)
    for g in range(groups):
        for i in range(2):
            for j in range(2):
                kx, ky = int(k[g * 4 + i * 2 + j]), int(k[4 * groups + g * 4 + i * 2 + j])
                src = x[:, g * cg:(g + 1) * cg][:, :, (hh + ky).clamp(0, H - 1)][:, :, :, (ww + kx).clamp(0, W - 1)]
                want[:, g * cg:(g + 1) * cg, i::2, j::2] = src
    assert torch.equal(got, want)


@pytest.mark.parametrize("what", ["groups3", "four_per_group", "misaligned_x", "misaligned_y", "scale3"])
def test_refusals_launch_nothing(what):
    L = _L()
    dtype = torch.float16
    C, groups, scale, x_off, y_off = {"groups3": (24, 3, 2, 8, 8), "four_per_group": (16, 4, 2, 8, 8), "misaligned_x": (32, 4, 2, 4, 8),
                                      "misaligned_y": (32, 4, 2, 8, 4), "scale3": (32, 4, 3, 8, 8)}[what]
    B, H, W = 1, 3, 5
    x = _rand((B, C, H, W), ("refuse", what), dtype)
    _, xv = _window(x, x_off, 8, dtype)
    n = 8 * groups
    wd = torch.zeros(n, C, dtype=dtype, device="cuda")
    bd = torch.zeros(n, dtype=torch.float32, device="cuda")
    ybuf, yv, _ = _out(B, C, 2 * H, 2 * W, dtype, off=y_off)
    rc = L.lib().ey_dysample(L.dtype_code(dtype), B, H, W, C, scale, groups, xv.data_ptr(), L.cstride(xv), wd.data_ptr(), bd.data_ptr(), None, bd.data_ptr(),
                             yv.data_ptr(), L.cstride(yv), L.stream())
    torch.cuda.synchronize()
    assert rc == -2, (rc, L.lib().ey_last_error())  # EY_EUNSUPPORTED
    msg = L.lib().ey_last_error().decode()
    assert {"groups3": "groups=3", "four_per_group": "multiple of 8", "misaligned_x": "16-byte", "misaligned_y": "16-byte", "scale3": "scale=3"}[what] in msg, msg
    assert torch.isnan(ybuf).all(), "a refused call wrote to the output"


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "f16"])
def test_run_to_run_identical(dtype):
    C, groups, B, H, W = 96, 4, 2, 17, 33
    x, w, b, s = _case(C, groups, B, H, W, dtype, True, "again")
    pos = _init_pos(groups)
    a, _, _ = _run(x, w, b, s, pos, groups, dtype)
    for _ in range(3):
        c, _, _ = _run(x, w, b, s, pos, groups, dtype)
        assert torch.equal(torch.nan_to_num(a, nan=7.0), torch.nan_to_num(c, nan=7.0))


def test_zz_worst_ratios():
    for fam, (r, case) in sorted(WORST.items()):
        print(f"[fp64] worst err/bound {fam}: {r:.3f} ({case})")
