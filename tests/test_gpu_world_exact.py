"""-m gpu: ey_max_sigmoid_attn (csrc/world.hip) against the float64 restatement of tests/fp64_world_ref.py, in fp32 and f16 storage.

E, P and Y are channel windows of wider NaN-filled buffers: nothing outside the output window may be written, nothing inside may stay NaN, and
the kernel may not read a channel outside the input windows (a NaN there would reach the gate or the product).  The bound is per element and
comes from the operation count, u = 2^-24 per fp32 operation:
  dot      32 terms accumulated in fp32 (f16 products are exact in fp32, fp32 ones round once each): 34 u sum|e_c g_c|, in any order;
  max      1-Lipschitz in each dot: the largest dot bound over the texts of the pixel and head;
  a        the division by fp32 sqrt(32) and the bias add round once each: d_max / sqrt(32) + u |max / sqrt(32)| + u |a|;
  sigmoid  s = rcp(1 + exp(-a)) with v_exp_f32 / v_rcp_f32 within 2^-22 (as tests/test_gpu_dysample_exact.py states them), the exponent's
           scaling by log2(e) another 2 u |a| relative in exp(-a), the sum one rounding; s' = s (1 - s) <= 1/4:
           s (1 - s) (d_a + 2^-22 + 2 u |a|) + s (u + 2^-22);
  products aw = s * scale and y = p * aw: |scale| d_s + u |aw|, then |p| d_aw + u |y|;
  output   one rounding to the storage type (_grade adds the ulp).
Derived, not measured.  Maps 1x1, 1x9, 5x7 and 17x33 (pixel-tile tails) at B = 2; 1, 2, 3, 5 and 10 heads (C = 32 ... 320); 1, 5, 15, 16, 17, 80
and 257 texts (one text, tile tails on both sides, several tiles); one guide for the batch and one per image (the images' guides differ).
Bit-exact probes on dyadic data, refusals that leave the output untouched, and the same bits on a second run."""
import zlib

import numpy as np
import pytest
import torch

import fp64_world_ref as f64
import world_synth as ws

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
EXP_REL = RCP_REL = 2.0 ** -22
DTYPES = [torch.float32, torch.float16]
EINVAL, EUNSUPPORTED = -1, -2


def _L():
    from edge_yolo_amd import _lib as L
    return L


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


def _run(e, p, g, bias, scale, nh, dtype, e_off=8, p_off=16, y_off=8, hc=32, C=None, n=None, null=None, expect=0):
    """ey_max_sigmoid_attn on windows -> (y buffer, y view, y offset).  e, p, g: values representable in dtype."""
    L = _L()
    B, Cc, H, W = e.shape
    _, ev = _window(e, e_off, 8, dtype)
    _, pv = _window(p, p_off, 24, dtype)
    gd = g.to(device="cuda", dtype=dtype).contiguous()
    bd = bias.float().cuda().contiguous()
    sd = None if scale is None else scale.float().cuda().contiguous()
    ybuf, yv, off = _out(B, Cc, H, W, dtype, off=y_off)
    ptr = {"e": ev.data_ptr(), "p": pv.data_ptr(), "g": gd.data_ptr(), "bias": bd.data_ptr(), "y": yv.data_ptr()}
    if null:
        ptr[null] = None
    rc = L.lib().ey_max_sigmoid_attn(L.dtype_code(dtype), B, H * W, nh, hc, Cc if C is None else C, g.shape[1] if n is None else n, g.shape[0], ptr["e"],
                                     L.cstride(ev), ptr["p"], L.cstride(pv), ptr["g"], ptr["bias"], None if sd is None else sd.data_ptr(), ptr["y"],
                                     L.cstride(yv), L.stream())
    torch.cuda.synchronize()
    assert rc == expect, (rc, L.lib().ey_last_error())
    return ybuf, yv, off


def _bound(e, p, g, bias, scale, nh):
    """(y, E): the float64 result and the per-element bound of the module docstring, without the output rounding."""
    e64, p64, g64 = e.double().numpy(), p.double().numpy(), g.double().numpy()
    b64 = bias.double().numpy()
    s64 = None if scale is None else scale.double().numpy()
    y, mx = f64.max_sigmoid_attn64(e64, p64, g64, b64, s64)
    B, C, H, W = e64.shape
    gg = np.broadcast_to(np.abs(g64), (B,) + g64.shape[1:]).reshape(B, -1, nh, 32)
    d_dot = 34 * U * np.einsum("bmchw,bnmc->bmhwn", np.abs(e64).reshape(B, nh, 32, H, W), gg).max(-1)
    q = mx / f64.SQRT_HC
    a = q + b64[None, :, None, None]
    d_a = d_dot / f64.SQRT_HC + U * np.abs(q) + U * np.abs(a)
    s = 1.0 / (1.0 + np.exp(-a))
    d_s = s * (1.0 - s) * (d_a + EXP_REL + 2 * U * np.abs(a)) + s * (U + RCP_REL)
    sc = np.ones(nh) if s64 is None else s64
    aw = s * sc[None, :, None, None]
    d_aw = np.abs(sc)[None, :, None, None] * d_s + U * np.abs(aw)
    d_aw = np.repeat(d_aw, 32, axis=1)
    E = np.abs(p64) * d_aw + U * np.abs(y)
    return torch.tensor(y), torch.tensor(E)


def _grade(case, got, want, E, dtype):
    bnd = 1.05 * E + _ulp(want, dtype) + 2.0 ** -40
    assert torch.isfinite(got).all(), f"{case}: non-finite output"
    r = float(((got - want).abs() / bnd).max())
    print(f"[fp64] {case} max err/bound {r:.3f}")
    assert r <= 1.0, f"{case}: max err/bound {r:.3f}"


def _cases():
    """Every (heads, texts) pair on the 5x7 map; on the other maps every heads value and every texts value at least once."""
    out = [((5, 7), nh, n) for nh in ws.HEADS for n in ws.TEXTS]
    for hw in ((1, 1), (1, 9), (17, 33)):
        for i, n in enumerate(ws.TEXTS):
            out.append((hw, ws.HEADS[i % len(ws.HEADS)], n))
    return out


@pytest.mark.parametrize("per_image", [False, True], ids=["Bg1", "BgB"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16"])
def test_against_fp64(dtype, per_image):
    B = 2
    for (H, W), nh, n in _cases():
        case = f"msa_{H}x{W}_nh{nh}_n{n}_{'BgB' if per_image else 'Bg1'}_{'f16' if dtype == torch.float16 else 'f32'}"
        e, p, g, bias, scale = ws.attn_case(case, B, H, W, nh, n, B if per_image else 1, dtype == torch.float16)
        if per_image:
            assert not torch.equal(g[0], g[1])
        use_scale = scale if (nh + n) % 2 else None
        want, E = _bound(e, p, g, bias, use_scale, nh)
        ybuf, yv, off = _run(e, p, g, bias, use_scale, nh, dtype)
        _grade(case, _fetch(ybuf, yv, off), want, E, dtype)


def _dyadic(B, nh, H, W, n, seed):
    """p: dyadic values of both signs; e = 2 everywhere; g = -32 everywhere: every dot is -2048, far below the sigmoid's flush to 0."""
    C = 32 * nh
    gen = torch.Generator().manual_seed(zlib.crc32(repr(("dyadic", B, nh, H, W, n, seed)).encode()))
    p = (torch.randint(-64, 65, (B, C, H, W), generator=gen).float() / 8.0)
    p[p == 0] = 0.125
    return torch.full((B, C, H, W), 2.0), p, torch.full((1, n, C), -32.0), torch.zeros(nh)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16"])
def test_padded_text_columns_stay_out_of_the_maximum(dtype):
    """Every real dot is -2048: sigmoid(-2048 / sqrt(32)) is exactly 0 (exp overflows, rcp(inf) = 0), so the output is exactly +-0.  A
    zero-padded text column would give a dot of 0, a gate of 1/2 and a non-zero output."""
    for n in (1, 5, 17, 21):
        e, p, g, bias = _dyadic(2, 3, 5, 7, n, 0)
        ybuf, yv, off = _run(e, p, g, bias, None, 3, dtype)
        got = _fetch(ybuf, yv, off)
        assert bool((got == 0).all()), f"n={n}: a padded column entered the maximum"


@pytest.mark.parametrize("where", ["last", "first"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16"])
def test_single_large_dot_gives_gate_one(dtype, where):
    """One text (the last of a partial tile, or text 0) has a dot of +2048: exp(-362) is 0, rcp(1) is 1, no scale: Y == P bit for bit."""
    for n in (5, 21, 33):
        e, p, g, bias = _dyadic(2, 2, 5, 7, n, 1)
        g[0, n - 1 if where == "last" else 0] = 32.0
        ybuf, yv, off = _run(e, p, g, bias, None, 2, dtype)
        got = _fetch(ybuf, yv, off)
        assert torch.equal(got, p.double()), f"n={n} {where}"


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16"])
def test_heads_keep_to_their_channels(dtype):
    """Four heads, five texts.  Even head m: e = +2 and only text m has g = +32 (a different winner per head): gate exactly 1.  Odd head m: e = -2
    and every text has g = +32: every dot is -2048, gate exactly 0.  A head that read a neighbour's embedding or guide channels would flip."""
    nh, n = 4, 5
    e, p, g, bias = _dyadic(2, nh, 5, 7, n, 2)
    for m in range(nh):
        ch = slice(32 * m, 32 * m + 32)
        if m % 2 == 0:
            g[0, m, ch] = 32.0
        else:
            e[:, ch] = -2.0
            g[0, :, ch] = 32.0
    ybuf, yv, off = _run(e, p, g, bias, None, nh, dtype)
    got = _fetch(ybuf, yv, off)
    for m in range(nh):
        ch = slice(32 * m, 32 * m + 32)
        if m % 2 == 0:
            assert torch.equal(got[:, ch], p[:, ch].double()), f"head {m}"
        else:
            assert bool((got[:, ch] == 0).all()), f"head {m}"


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16"])
def test_refusals_leave_the_output_untouched(dtype):
    L = _L()
    e, p, g, bias, _ = ws.attn_case("refuse", 2, 5, 7, 2, 5, 1, dtype == torch.float16)
    for kw, code in ((dict(hc=16), EUNSUPPORTED), (dict(C=48), EUNSUPPORTED), (dict(n=0), EINVAL), (dict(n=L.MSA_MAX_TEXTS + 1), EUNSUPPORTED),
                     (dict(null="e"), EINVAL), (dict(null="p"), EINVAL), (dict(null="g"), EINVAL), (dict(null="bias"), EINVAL)):
        ybuf, yv, off = _run(e, p, g, bias, None, 2, dtype, expect=code, **kw)
        assert torch.isnan(ybuf).all(), kw
    _run(e, p, g, bias, None, 2, dtype, null="y", expect=EINVAL)
    assert L.MSA_MAX_TEXTS >= 1203


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16"])
def test_same_bits_on_a_second_run(dtype):
    e, p, g, bias, scale = ws.attn_case("again", 2, 17, 33, 5, 80, 2, dtype == torch.float16)
    a = _fetch(*_run(e, p, g, bias, scale, 5, dtype))
    b = _fetch(*_run(e, p, g, bias, scale, 5, dtype))
    assert torch.equal(a, b)


def test_wrapper_writes_a_concat_slot():
    """nn._ops.max_sigmoid_attn with out= a channel slot of a wider buffer, as C2fAttn calls it; equal to the direct call bit for bit."""
    from edge_yolo_amd.nn import _ops as ops
    L = _L()
    e, p, g, bias, scale = ws.attn_case("slot", 2, 5, 7, 2, 5, 1, True)
    buf = L.empty_nhwc(2, 3 * 64, 5, 7, torch.float16, torch.device("cuda"))
    buf[:] = float("nan")
    buf[:, :64] = e.cuda().half()
    pd = L.as_nhwc(p.cuda().half())
    y = ops.max_sigmoid_attn(buf[:, :64], pd, g.cuda().half(), bias.cuda(), scale.cuda(), 2, out=buf[:, 128:])
    want = _fetch(*_run(e, p, g, bias, scale, 2, torch.float16))
    assert y.data_ptr() == buf[:, 128:].data_ptr() and torch.equal(buf[:, 128:].double().cpu(), want) and torch.isnan(buf[:, 64:128]).all()
