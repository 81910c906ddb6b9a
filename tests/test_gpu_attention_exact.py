"""-m gpu: the attention cores (ey_linear_attention, ey_softmax_attention and the EY_BLK_LINATTN block stage) against the fp64
references of tests/fp64_attn_ref.py, on every launch path; each case asserts the kernel it meant to run
(ey_attention_last_variant).

* Bit-exact probes: data for which every exponential but one per softmax row underflows to exactly 0 (arguments <= -120), so the
  result is a gather that every path must reproduce bit for bit.  Softmax: ±R codes of a target key per query and a negative
  bias channel (every real score < 0: a zero-filled padded key that leaked through the mask would win with score 0).  Linear:
  one-hot ks (k[n] = R e_sigma(n)), one dominant pixel per q column (some in the last partial 128-pixel chunk), small-integer v.
* Bounded checks on general data: the per-element fp64 bound and a mean-ulp gate (ulp16 for f16 outputs, ulp32 for f32).
* Every output is a channel view into a wider buffer with one spare image, prefilled with NaN: nothing outside the view may be
  written, nothing inside may stay NaN.  Refusals (key_dim / head_dim > 64, N past the LDS limit) launch nothing."""
import math
import zlib

import pytest
import torch

pytestmark = pytest.mark.gpu

import fp64_attn_ref as AR  # noqa: E402
import fp64_ref as R  # noqa: E402
from gpu_util import _traced, tuned  # noqa: E402

LIN_F32, LIN_F16, LIN_MFMA = 101, 102, 103
SV = 200  # + 4 f16, + 2 K in LDS, + 1 nsplit == 1
SM = 300  # + NKS
ALL_VARIANTS = {LIN_F32, LIN_F16, LIN_MFMA} | {SV + i for i in range(8)} | {SM + n for n in (4, 8, 10, 13)}
MEAN_ULP32 = 4.0   # gate on the mean |err| / ulp32(magnitude) of the f32 outputs (fp64_attn_ref.report32)
WORST = {}         # family -> [(max err/bound, case), (max mean ulp, case)], printed by test_variant_coverage


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _lib():
    from edge_yolo_amd import _lib as L
    return L


def _variant():
    return _lib().lib().ey_attention_last_variant()


def _hw(N):
    """a (H, W) map of N pixels (ragged where N allows)."""
    for h in range(int(math.isqrt(N)), 0, -1):
        if N % h == 0:
            return h, N // h
    return 1, N


def _rows_t(x):
    B, C, H, W = x.shape
    return x.permute(0, 2, 3, 1).reshape(B, H * W, C)


def _input(vals, dtype, off=0, pad=0):
    """NHWC device view of logical (B, C, H, W) `vals` at channel offset `off` of a (C + pad)-channel buffer whose other channels
    hold NaN (a kernel that reads outside its view turns its output into NaN)."""
    L = _lib()
    B, C, H, W = vals.shape
    buf = L.empty_nhwc(B, C + pad, H, W, dtype, "cuda")
    buf.copy_(torch.full((B, C + pad, H, W), float("nan")))
    t = buf[:, off:off + C]
    t.copy_(vals.to(dtype))
    return t


class _Out:
    """Output view: channels [8, 8 + C) of a (C + 16)-channel NHWC buffer with one spare image, all NaN beforehand."""

    def __init__(self, B, C, H, W, dtype):
        L = _lib()
        self.C = C
        self.buf = L.empty_nhwc(B + 1, C + 16, H, W, dtype, "cuda")
        self.buf.fill_(float("nan"))
        self.y = self.buf[:B, 8:8 + C]

    def check(self, case):
        torch.cuda.synchronize()
        b = self.buf
        assert not torch.isnan(self.y).any(), f"{case}: {int(torch.isnan(self.y).sum())} output elements were not written"
        outside = torch.cat([b[:-1, :8].flatten(), b[:-1, 8 + self.C:].flatten(), b[-1].flatten()])
        assert torch.isnan(outside).all(), f"{case}: {int((~torch.isnan(outside)).sum())} elements outside the output view were written"


def _note(family, case, rb, mu):
    w = WORST.setdefault(family, [(0.0, ""), (0.0, "")])
    if rb > w[0][0]:
        w[0] = (rb, case)
    if mu > w[1][0]:
        w[1] = (mu, case)


def _check(family, case, label, got, y, E, Y, dtype):
    bnd = AR.out_bound(y, E, dtype)
    if dtype == torch.float16:
        rb, mu = R.report(case, label, got, y, bnd)
    else:
        rb, mu = AR.report32(case, label, got, y, bnd, Y, MEAN_ULP32)
    _note(family, case, rb, mu)


# ------------------------------------------------------------------------------------------------------------- linear attention
def _lin_run(qkv, heads, dtype, **tune):
    from edge_yolo_amd.nn import _ops
    B, C3, H, W = qkv.shape
    out = _Out(B, C3 // 3, H, W, dtype)
    with tuned(**tune):
        _ops.linear_attention(qkv, heads, out=out.y)
        v = _variant()
    return out, v


def _lin_case(case, vals, heads, dtype, want_variant, f16_points, off=0, pad=0, **tune):
    qkv = _input(vals, dtype, off, pad)
    out, v = _lin_run(qkv, heads, dtype, **tune)
    assert v == want_variant, f"{case}: ran variant {v}, expected {want_variant}"
    out.check(case)
    y, E, Y = AR.linear_attention_ref(qkv, heads, f16_points=f16_points)
    _check({LIN_F32: "linear f32 VALU", LIN_F16: "linear f16 VALU", LIN_MFMA: "linear f16 MFMA"}[v], case, v, _rows_t(out.y), y, E, Y, dtype)


LIN_F32_CASES = [(d, h, N) for d in (16, 32, 48, 64) for h in (1, 2, 4) for N in (1, 7, 35, 117, 400, 1600)]


@pytest.mark.parametrize("d,heads,N", LIN_F32_CASES)
def test_linear_f32_valu(d, heads, N):
    """d < 64 is the regression case of the lanes without a channel (their exp(-inf - -inf) = NaN reached every output)."""
    H, W = _hw(N)
    vals = torch.randn((2, 3 * d * heads, H, W), generator=_gen("lf32", d, heads, N)) * 1.5
    _lin_case(f"linear f32 d={d} heads={heads} N={N}", vals, heads, torch.float32, LIN_F32, False)


@pytest.mark.parametrize("d,N,off,pad,tune", [(32, 400, 0, 0, {}), (48, 117, 0, 0, {}), (32, 1600, 0, 0, {}), (16, 35, 0, 0, {}),
                                              (64, 400, 1, 9, {}), (64, 129, 1, 9, {}), (64, 400, 0, 0, {"linattn_mfma": 0})])
def test_linear_f16_valu(d, N, off, pad, tune):
    """d != 64, a qkv view one channel off the 16-byte alignment, or the MFMA kernel switched off."""
    H, W = _hw(N)
    vals = torch.randn((2, 3 * d * 2, H, W), generator=_gen("lf16", d, N, off)) * 1.5
    _lin_case(f"linear f16 d={d} N={N} off={off} {tune}", vals, 2, torch.float16, LIN_F16, False, off, pad, **tune)


@pytest.mark.parametrize("N", [1, 8, 63, 64, 127, 128, 129, 256, 400, 1600, 6400])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("heads", [2, 4])
def test_linear_mfma(N, B, heads):
    H, W = _hw(N)
    vals = torch.randn((B, 3 * 64 * heads, H, W), generator=_gen("lmfma", N, B, heads)) * 1.5
    _lin_case(f"linear mfma N={N} B={B} heads={heads}", vals, heads, torch.float16, LIN_MFMA, True)


@pytest.mark.parametrize("heads,N", [(2, 400), (4, 400), (2, 169), (4, 169)])
def test_linear_block_stage(heads, N):
    """The EY_BLK_LINATTN stage (two heads side by side per workgroup) as a one-stage block program through ey_block_run."""
    from edge_yolo_amd.nn import _block, _ops
    H, W = _hw(N)
    case = f"linear block stage heads={heads} N={N}"
    vals = torch.randn((2, 3 * 64 * heads, H, W), generator=_gen("lblk", heads, N)) * 1.5
    qkv = _input(vals, torch.float16)
    out = _Out(2, 64 * heads, H, W, torch.float16)
    cache = _block.BlockCache("attn_exact")
    got, ker = _traced(lambda: cache.run(lambda q: [_ops.linear_attention(q, heads, out=out.y)], [qkv]))
    assert got is not None and got[0].data_ptr() == out.y.data_ptr(), f"{case}: not run as a block program into the output view"
    assert ker == ["block_kernel<attn_exact>"], ker
    out.check(case)
    y, E, Y = AR.linear_attention_ref(qkv, heads, f16_points=True)
    _check("linear block stage", case, ker[0], _rows_t(out.y), y, E, Y, torch.float16)


def _gathered(y):
    """The probes' fp64 results are integers up to the exp(-R) terms of the non-winning entries (< 1e-50): that integer is the
    answer every kernel must produce, the fp32 exponentials of those terms being exactly 0."""
    want = y.round()
    assert float((y - want).abs().max()) < 1e-30, "probe construction: the fp64 result is not a gather"
    return want


def _lin_probe(B, N, heads, d, gen, R_=256.0):
    """k[n] = R e_sigma(n); column i of q is R at pixel tau(i) and 0 elsewhere (tau(0) = N - 1: the last, partial 128-pixel chunk);
    v small integers.  Then ks and qs are one-hot and y[n] = sum_{tau(i) = n} sum_{sigma(m) = i} v[m]."""
    C = heads * d
    q = torch.zeros(B, N, heads, d, dtype=torch.float64)
    k = torch.zeros_like(q)
    v = torch.randint(-3, 4, (B, N, heads, d), generator=gen).double()
    sigma = torch.randint(0, d, (B, N, heads), generator=gen)
    k.scatter_(-1, sigma.unsqueeze(-1), R_)
    tau = (N - 1 - 3 * torch.arange(d)) % N
    tau = tau.roll(int(torch.randint(0, d, (1,), generator=gen)))
    tau[0] = N - 1
    q[:, tau, :, torch.arange(d)] = R_
    t = torch.cat([x.reshape(B, N, C) for x in (q, k, v)], -1)
    H, W = _hw(N)
    return t.reshape(B, H, W, 3 * C).permute(0, 3, 1, 2)


@pytest.mark.parametrize("dtype,d,N,heads,B,variant,kind", [
    (torch.float32, 16, 7, 2, 2, LIN_F32, "direct"), (torch.float32, 64, 400, 2, 2, LIN_F32, "direct"),
    (torch.float32, 48, 1600, 1, 1, LIN_F32, "direct"), (torch.float16, 32, 400, 2, 2, LIN_F16, "direct"),
    (torch.float16, 64, 129, 2, 3, LIN_MFMA, "direct"), (torch.float16, 64, 400, 2, 3, LIN_MFMA, "direct"),
    (torch.float16, 64, 1600, 4, 1, LIN_MFMA, "direct"), (torch.float16, 64, 400, 2, 2, None, "block")])
def test_linear_exact_probe(dtype, d, N, heads, B, variant, kind):
    from edge_yolo_amd.nn import _block, _ops
    case = f"linear probe {kind} {str(dtype)[6:]} d={d} N={N} heads={heads} B={B}"
    vals = _lin_probe(B, N, heads, d, _gen("lprobe", d, N, heads, B))
    qkv = _input(vals, dtype)
    if kind == "block":
        H, W = _hw(N)
        out = _Out(B, heads * d, H, W, dtype)
        got, ker = _traced(lambda: _block.BlockCache("attn_probe").run(lambda q: [_ops.linear_attention(q, heads, out=out.y)], [qkv]))
        assert got is not None and ker == ["block_kernel<attn_probe>"], ker
        label = ker[0]
    else:
        out, label = _lin_run(qkv, heads, dtype)
        assert label == variant, f"{case}: ran variant {label}, expected {variant}"
    out.check(case)
    y, _, _ = AR.linear_attention_ref(qkv, heads, f16_points=dtype == torch.float16 and d == 64)
    R.assert_exact(case, label, _rows_t(out.y), _gathered(y))


# ------------------------------------------------------------------------------------------------------------ softmax attention
def _nks(N):
    n = (N + 31) // 32
    return 4 if n <= 4 else 8 if n <= 8 else 10 if n <= 10 else 13


def _soft_run(qkv, heads, kd, hd, scale, dtype, **tune):
    from edge_yolo_amd.nn import _ops
    B, _, H, W = qkv.shape
    out = _Out(B, heads * hd, H, W, dtype)
    with tuned(**tune):
        _ops.softmax_attention(qkv, heads, kd, hd, scale, out=out.y)
        v = _variant()
    return out, v


def _soft_family(v):
    if v >= SM:
        return "softmax f16 MFMA"
    return f"softmax {'f16' if (v - SV) & 4 else 'f32'} VALU"


def _soft_case(case, vals, heads, kd, hd, scale, dtype, want_variant, off=0, pad=0, bsel=None, **tune):
    qkv = _input(vals, dtype, off, pad)
    out, v = _soft_run(qkv, heads, kd, hd, scale, dtype, **tune)
    assert v == want_variant, f"{case}: ran variant {v}, expected {want_variant}"
    out.check(case)
    mfma = v >= SM
    sel = slice(None) if bsel is None else bsel
    y, E, Y = AR.softmax_attention_ref(qkv[sel], heads, kd, hd, scale, f16_points=mfma)
    _check(_soft_family(v), case, v, _rows_t(out.y)[sel], y, E, Y, dtype)


@pytest.mark.parametrize("N", [1, 16, 31, 33, 128, 129, 256, 257, 300, 320, 321, 400, 416])
def test_softmax_mfma(N):
    """All four NKS tiers of the score registers and their edges (32-key steps: N <= 128 / 256 / 320 / 416)."""
    H, W = _hw(N)
    vals = torch.randn((2, 2 * 128, H, W), generator=_gen("smfma", N)) * 1.2
    _soft_case(f"softmax mfma N={N}", vals, 2, 32, 64, 32 ** -0.5, torch.float16, SM + _nks(N))


def test_softmax_mfma_scale():
    vals = torch.randn((3, 2 * 128, 15, 20), generator=_gen("smfma_scale")) * 1.2
    _soft_case("softmax mfma N=300 scale=0.61", vals, 2, 32, 64, 0.61, torch.float16, SM + 10)


# (dtype, B, heads, kd, hd, N, scale, off/pad of the qkv view, tune, variant, rows checked)
F16, F32 = torch.float16, torch.float32
SOFT_VALU = [
    (F16, 2, 2, 32, 64, 417, None, 0, {}, SV + 4 + 2, None),          # first N past the MFMA kernel
    *[(F32, 2, 2, kd, hd, 100, None, 0, {}, SV + 2, None) for kd in (16, 32, 64) for hd in (32, 64, 128)],
    (F16, 2, 2, 16, 128, 77, None, 0, {}, SV + 4 + 2, None),
    (F16, 2, 2, 64, 32, 77, None, 0, {}, SV + 4 + 2, None),
    (F16, 2, 2, 32, 64, 100, None, 1, {}, SV + 4 + 2, None),           # misaligned qkv view
    (F16, 2, 2, 32, 64, 100, None, 0, {"softattn_mfma": 0}, SV + 4 + 2, None),
    (F32, 1, 2, 32, 64, 1600, None, 0, {}, SV, None),                  # K from global (K_LDS = false)
    (F16, 1, 2, 32, 64, 1600, None, 0, {}, SV + 4 + 2, None),
    (F16, 1, 2, 64, 32, 1600, None, 0, {}, SV + 4, None),              # f16, K from global
    (F32, 128, 4, 16, 32, 16, None, 0, {}, SV + 2 + 1, None),          # B * heads = 512: nsplit == 1
    (F16, 128, 4, 16, 32, 16, None, 0, {}, SV + 4 + 2 + 1, None),
    (F32, 64, 8, 64, 8, 600, None, 0, {}, SV + 1, [0, 63]),            # nsplit == 1, K from global
    (F16, 64, 8, 64, 8, 1140, None, 0, {}, SV + 4 + 1, [0, 63]),
    (F32, 2, 2, 32, 64, 100, 0.37, 0, {}, SV + 2, None),               # non-default scale
    (F32, 1, 1, 8, 8, 10176, None, 0, {}, SV, None),                   # the largest N: 160 KiB of LDS scores
]


@pytest.mark.parametrize("dtype,B,heads,kd,hd,N,scale,off,tune,variant,bsel", SOFT_VALU)
def test_softmax_valu(dtype, B, heads, kd, hd, N, scale, off, tune, variant, bsel):
    H, W = _hw(N)
    scale = kd ** -0.5 if scale is None else scale
    vals = torch.randn((B, heads * (2 * kd + hd), H, W), generator=_gen("svalu", str(dtype), B, heads, kd, hd, N)) * 1.2
    case = f"softmax valu {str(dtype)[6:]} B={B} heads={heads} kd={kd} hd={hd} N={N} scale={scale:.3g} off={off} {tune}"
    _soft_case(case, vals, heads, kd, hd, scale, dtype, variant, off, 7 if off else 0, bsel, **tune)


def _soft_probe(B, N, heads, kd, hd, gen, R_=1024.0):
    """Key m carries R * (±1 code of m) in kd - 1 channels and 1 in the last; query n carries the ±1 code of its target t(n) and
    -(bits + 1) R in the last channel: score(n, m) = R (bits - 2 hamming(t(n), m)) - (bits + 1) R, i.e. -R for the target and <= -3R
    for every other real key, 0 for a zero padded key.  With scale 2^-3 every exp but the target's gets an argument <= -256."""
    bits = max(1, (N - 1).bit_length())
    assert bits <= kd - 1
    idx = torch.arange(N)
    code = ((idx.unsqueeze(-1) >> torch.arange(bits)) & 1).double() * 2 - 1       # (N, bits)
    tgt = (idx * 5 + 3) % N
    tgt[0] = N - 1
    tgt = tgt[torch.randperm(N, generator=gen)]
    per = 2 * kd + hd
    t = torch.zeros(B, N, heads, per, dtype=torch.float64)
    t[..., :bits] = code[tgt].view(1, N, 1, bits)
    t[..., kd - 1] = -(bits + 1) * R_
    t[..., kd:kd + bits] = R_ * code.view(1, N, 1, bits)
    t[..., 2 * kd - 1] = 1
    v = torch.randint(1, 9, (B, N, heads, hd), generator=gen).double() * (torch.randint(0, 2, (B, N, heads, hd), generator=gen) * 2 - 1)
    t[..., 2 * kd:] = v
    H, W = _hw(N)
    return t.reshape(B, H, W, heads * per).permute(0, 3, 1, 2)


@pytest.mark.parametrize("dtype,N,kd,hd,tune,variant", [
    (F16, 31, 32, 64, {}, SM + 4), (F16, 129, 32, 64, {}, SM + 8), (F16, 300, 32, 64, {}, SM + 10), (F16, 416, 32, 64, {}, SM + 13),
    (F16, 417, 32, 64, {}, SV + 6), (F16, 100, 16, 128, {}, SV + 6), (F32, 417, 16, 128, {}, SV + 2), (F32, 1600, 32, 64, {}, SV),
    (F16, 1600, 64, 32, {}, SV + 4)])
def test_softmax_exact_probe(dtype, N, kd, hd, tune, variant):
    B, heads, scale = 2, 2, 0.125
    case = f"softmax probe {str(dtype)[6:]} N={N} kd={kd} hd={hd}"
    vals = _soft_probe(B, N, heads, kd, hd, _gen("sprobe", str(dtype), N, kd, hd))
    qkv = _input(vals, dtype)
    t = _rows_t(qkv).double().reshape(B, N, heads, 2 * kd + hd)
    S = scale * (t[..., :kd].transpose(1, 2) @ t[..., kd:2 * kd].permute(0, 2, 3, 1))
    assert torch.equal(S.float().double(), S), f"{case}: the probe's scores are not exact in fp32"
    out, v = _soft_run(qkv, heads, kd, hd, scale, dtype, **tune)
    assert v == variant, f"{case}: ran variant {v}, expected {variant}"
    out.check(case)
    y, _, _ = AR.softmax_attention_ref(qkv, heads, kd, hd, scale, f16_points=v >= SM)
    R.assert_exact(case, v, _rows_t(out.y), _gathered(y))


# ---------------------------------------------------------------------------------------------------------------------- refusals
def test_refusals():
    L = _lib()
    lib = L.lib()
    st = L.stream()
    # key_dim 65 / head_dim 65: nothing launched, the output untouched
    for kd, hd in ((65, 8), (64, 8)):
        qkv = _input(torch.randn(1, 2 * kd + hd, 4, 4), torch.float32)
        out = _Out(1, hd, 4, 4, torch.float32)
        rc = lib.ey_softmax_attention(L.F32, 1, 16, 1, kd, hd, 0.1, qkv.data_ptr(), L.cstride(qkv), out.y.data_ptr(), L.cstride(out.y), st)
        torch.cuda.synchronize()
        if kd > 64:
            assert rc == -2 and _variant() == 0, (rc, lib.ey_last_error())
            assert torch.isnan(out.buf).all(), "refused softmax attention wrote its output"
        else:
            assert rc == 0 and _variant() == SV + 2
    qkv = _input(torch.randn(1, 3 * 130, 4, 4), torch.float32)
    out = _Out(1, 130, 4, 4, torch.float32)
    rc = lib.ey_linear_attention(L.F32, 1, 16, 130, 2, qkv.data_ptr(), L.cstride(qkv), out.y.data_ptr(), L.cstride(out.y), st)
    torch.cuda.synchronize()
    assert rc == -2 and _variant() == 0, (rc, lib.ey_last_error())
    assert torch.isnan(out.buf).all(), "refused linear attention wrote its output"
    # N = 10177: the fp32 scores of 4 queries no longer fit 160 KiB of LDS
    N = 10177
    qkv = _input(torch.randn(1, 24, 1, N), torch.float32)
    out = _Out(1, 8, 1, N, torch.float32)
    rc = lib.ey_softmax_attention(L.F32, 1, N, 1, 8, 8, 0.1, qkv.data_ptr(), L.cstride(qkv), out.y.data_ptr(), L.cstride(out.y), st)
    torch.cuda.synchronize()
    assert rc == -2 and _variant() == 0 and b"LDS" in lib.ey_last_error(), (rc, lib.ey_last_error())
    assert torch.isnan(out.buf).all(), "refused softmax attention wrote its output"
    print("[exact] refusals: key_dim 65, head_dim 65, N = 10177 launch nothing")


# ------------------------------------------------------------------------------------------------------------------ coverage
def _declared():
    out = {LIN_F32, LIN_F16, LIN_MFMA}
    out |= {SM + _nks(N) for N in (1, 16, 31, 33, 128, 129, 256, 257, 300, 320, 321, 400, 416)}
    out |= {c[9] for c in SOFT_VALU}
    return out


def test_variant_coverage():
    """Every variant code is asserted by at least one case of this file (each case asserts its own at run time)."""
    assert _declared() == ALL_VARIANTS, sorted(ALL_VARIANTS ^ _declared())
    for fam, ((rb, c1), (mu, c2)) in sorted(WORST.items()):
        print(f"[fp64] worst {fam}: err/bound {rb:.3f} ({c1}); mean ulp {mu:.3f} ({c2})")
