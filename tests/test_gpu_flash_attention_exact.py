"""-m gpu: the flash attention core (ey_flash_attention, GlobalSparseAttn of the LGL block) against a float64 reference, on the f16 MFMA
kernels for head_dim 16 / 32 / 64 and the fp32 / f16 VALU fallback; each case asserts the kernel that ran (ey_attention_last_variant).

* Bounded checks: head_dim 16, 32, 64 x 1, 2, 4 heads x 1, 6, 15, 16, 17, 63, 64, 65, 240, 401 and 1600 tokens, 6400 tokens (layer 2 of
  yolov13n-LGL at 640^2) and 25 600 tokens (1280^2) at head_dim 16.  q, k, v and y are channel windows of wider buffers whose other
  channels hold NaN: nothing outside y's window may be written, nothing inside may stay NaN.  Bound per element, from the kernels'
  arithmetic: fp32 scores of exact f16 products, exp to a few ulp, P rounded to f16 before the P.V MFMA (f16 path), fp32 sums, one
  output rounding -- the derivation of test_gpu_area_attention_exact.py with the head_dim as a parameter, plus the f16 subnormal range
  of P, which only matters at thousands of keys.
* Bit-exact one-hot probe: per query one key scores -8 and every other real key scores below -500 (times scale), so softmax is a gather
  of one v row that every path must reproduce bit for bit; a zero-filled padded key would score 0 and win if the mask leaked.  Token
  counts 1, 17, 65, 401 leave a partly padded last key tile.
* Refusals launch nothing."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from group_attn_util import data as _data, groups as _tok_out, lib as _L, one_hot, one_hot_target, ref as _ref, run, ulp as _ulp  # noqa: E402

FLASH_MFMA, FLASH_F32, FLASH_F16 = 500, 501, 502
WORST = {}


def _run(q, k, v, heads, scale, dtype, qoff=8, yoff=8, ypad=8):
    """-> y logical (B,C,H,W) float64 cpu"""
    from edge_yolo_amd.nn import _ops
    return run(lambda qv, kv, vv, yv: _ops.flash_attention(qv, kv, vv, heads, scale, out=yv), q, k, v, dtype, qoff, yoff, ypad)


def _check(case, got, q, k, v, heads, scale, dtype, mfma, rows=None):
    y, Y, Amax, Lsum, vmax = _ref(q, k, v, heads, scale, rows=rows)
    N, hd = q.shape[2] * q.shape[3], q.shape[1] // heads
    u = 2.0 ** -24
    # score error: fp32 sums of hd exact products (2 hd u |s|), scale multiply; propagated through exp (relative) for every key
    # against the row max -> 2 * (2 hd + 2) u * max|s| relative on P; exp itself 2^-21 relative; the P.V sum over N keys in fp32
    rel = 2 * (2 * hd + 2) * u * Amax + 2.0 ** -20 + 2 * N * u
    extra = 0.0
    if mfma:
        rel = rel + 2.0 ** -11  # P rounded to f16 before the MFMA
        # ... and a P below 2^-14 of its tile's running max is an f16 subnormal: absolute error 2^-25 per key, scaled by 1 / sum exp(s - max)
        extra = N * 2.0 ** -25 * vmax / Lsum
    bnd = rel * Y * 1.25 + extra + _ulp(y, dtype) + 2.0 ** -30  # (a whole ulp: the kernel's value may round across a binade boundary)
    g = _tok_out(got, heads, rows=rows)
    assert torch.isfinite(got).all(), f"{case}: non-finite output"
    r = float(((g - y).abs() / bnd).max())
    print(f"[fp64] {case} max err/bound {r:.3f}")
    fam = f"mfma hd{hd}" if mfma else ("f16 valu" if dtype == torch.float16 else "f32 valu")
    WORST[fam] = max(WORST.get(fam, (0.0, "")), (r, case))
    assert r <= 1.0, f"{case}: max err/bound {r:.3f}"


# tokens -> (B, H, W)
MAPS = {1: (2, 1, 1), 6: (2, 2, 3), 15: (2, 3, 5), 16: (1, 4, 4), 17: (2, 1, 17), 63: (1, 7, 9), 64: (2, 8, 8), 65: (1, 5, 13), 240: (2, 12, 20),
        401: (1, 1, 401), 1600: (1, 40, 40)}


@pytest.mark.parametrize("heads", [1, 2, 4])
@pytest.mark.parametrize("hd", [16, 32, 64])
def test_flash_attention_bounded(hd, heads):
    L = _L()
    scale = hd ** -0.5
    for N, (B, H, W) in MAPS.items():
        q, k, v = _data(B, H, W, heads, hd, (N, heads, hd))
        got = _run(q, k, v, heads, scale, torch.float16)
        assert L.lib().ey_attention_last_variant() == FLASH_MFMA + hd
        _check(f"mfma hd{hd} h{heads} B{B} N{N}", got, q, k, v, heads, scale, torch.float16, True)


def test_flash_attention_6400_tokens_hd16():
    """Layer 2 of yolov13n-LGL at 640^2: 80 x 80 pooled tokens, one head of 16 channels."""
    L = _L()
    q, k, v = _data(2, 80, 80, 1, 16, ("6400",))
    got = _run(q, k, v, 1, 0.25, torch.float16)
    assert L.lib().ey_attention_last_variant() == FLASH_MFMA + 16
    _check("mfma hd16 h1 B2 N6400", got, q, k, v, 1, 0.25, torch.float16, True)


def test_flash_attention_25600_tokens_hd16():
    """1280^2: 160 x 160 pooled tokens, beyond the VALU kernel's 10 176.  Every output is checked for NaN and window overrun; 512 queries
    (the first and last tiles, tile edges, a stride through the rest) against float64."""
    L = _L()
    q, k, v = _data(1, 160, 160, 1, 16, ("25600",))
    got = _run(q, k, v, 1, 0.25, torch.float16)
    assert L.lib().ey_attention_last_variant() == FLASH_MFMA + 16
    rows = torch.unique(torch.cat([torch.arange(0, 70), torch.arange(25530, 25600), torch.arange(63, 25600, 69)]))[:512]
    _check("mfma hd16 h1 B1 N25600", got, q, k, v, 1, 0.25, torch.float16, True, rows=rows)


@pytest.mark.parametrize("hd,heads,N", [(16, 1, 17), (32, 2, 240), (64, 4, 65), (24, 2, 63)])
def test_flash_attention_f32_valu(hd, heads, N):
    L = _L()
    B, H, W = MAPS[N]
    q, k, v = _data(B, H, W, heads, hd, ("f32", N, heads, hd))
    got = _run(q, k, v, heads, hd ** -0.5, torch.float32)
    assert L.lib().ey_attention_last_variant() == FLASH_F32
    _check(f"f32 hd{hd} h{heads} N{N}", got, q, k, v, heads, hd ** -0.5, torch.float32, False)


@pytest.mark.parametrize("hd,qoff,yoff", [(16, 4, 8), (32, 8, 2), (24, 8, 8)])
def test_flash_attention_f16_valu(hd, qoff, yoff):
    """f16 views the MFMA kernel cannot take (q not 16-byte aligned, y not 8-byte aligned, head_dim 24) run the VALU kernel."""
    L = _L()
    B, H, W = MAPS[65]
    q, k, v = _data(B, H, W, 2, hd, ("f16valu", hd))
    got = _run(q, k, v, 2, hd ** -0.5, torch.float16, qoff=qoff, yoff=yoff)
    assert L.lib().ey_attention_last_variant() == FLASH_F16
    _check(f"f16 valu hd{hd}", got, q, k, v, 2, hd ** -0.5, torch.float16, False)


@pytest.mark.parametrize("N,heads", [(1, 1), (17, 2), (64, 1), (65, 4), (401, 1), (1600, 2)])
@pytest.mark.parametrize("hd", [16, 32, 64])
@pytest.mark.parametrize("path", ["mfma", "f32"])
def test_flash_attention_one_hot_exact(hd, N, heads, path):
    L = _L()
    B, H, W = MAPS[N]
    q, k, v = one_hot(B, H, W, heads, 1, hd, ("onehot", B, H, W, heads, hd))
    dtype = torch.float32 if path == "f32" else torch.float16
    got = _run(q, k, v, heads, hd ** -0.5, dtype)
    assert L.lib().ey_attention_last_variant() == (FLASH_MFMA + hd if path == "mfma" else FLASH_F32)
    tgt = torch.stack([one_hot_target(N, h) for h in range(heads)])  # (heads, N)
    vt = _tok_out(v.double(), heads)  # (B, heads, N, hd)
    want = torch.gather(vt, 2, tgt.view(1, heads, N, 1).expand(B, heads, N, hd))
    g = _tok_out(got, heads)
    assert torch.equal(g, want), f"{path} hd{hd} N{N}: one-hot gather not bit-exact (max diff {float((g - want).abs().max())})"


def test_flash_attention_refusals():
    L = _L()
    q = torch.zeros(1, 128, 5, 5, dtype=torch.float32, device="cuda")
    p = q.data_ptr()
    f = L.lib().ey_flash_attention
    assert f(L.F32, 1, 25, 1, 128, 0.1, p, 128, p, 128, p, 128, p, 128, L.stream()) == -2 and L.lib().ey_attention_last_variant() == 0  # head_dim > 64
    assert f(L.F32, 1, 10177, 1, 16, 0.25, p, 16, p, 16, p, 16, p, 16, L.stream()) == -2 and L.lib().ey_attention_last_variant() == 0
    assert b"10176" in L.lib().ey_last_error()
    assert f(L.F16, 1, 25, 2, 32, 0.1, p, 32, p, 64, p, 64, p, 64, L.stream()) == -1 and L.lib().ey_attention_last_variant() == 0  # cstride < heads * hd
    assert f(L.F16, 1, 0, 1, 32, 0.1, p, 32, p, 32, p, 32, p, 32, L.stream()) == -1
    assert f(L.F16, 1, 25, 1, 32, 0.1, None, 32, p, 32, p, 32, p, 32, L.stream()) == -1
    assert f(2, 1, 25, 1, 32, 0.1, p, 32, p, 32, p, 32, p, 32, L.stream()) == -1
    torch.cuda.synchronize()
    assert float(q.abs().max()) == 0.0


def test_zz_worst_report():
    for fam, (r, case) in sorted(WORST.items()):
        print(f"[fp64] worst {fam}: err/bound {r:.3f} at {case}")
