"""-m gpu: the area attention core (ey_area_attention, YOLOv12's AAttn) against a float64 reference, on the f16 MFMA flash kernel
and the fp32 / f16 VALU kernels; each case asserts the kernel that ran (ey_attention_last_variant).

* Bounded checks: token counts per area 1, 6, 15, 16, 17, 240, 400, 401 and 1600, 1-8 heads, areas that split rows.  q, k, v and y
  are channel windows of wider buffers whose other channels hold NaN: nothing outside y's window may be written, nothing inside
  may stay NaN.  Bound per element, from the kernels' arithmetic: fp32 scores of exact f16 products, exp to a few ulp, P rounded
  to f16 before the P.V MFMA (f16 path), fp32 sums, one output rounding.
* Bit-exact one-hot probe: per query one key scores -8 and every other real key scores below -800 (times scale), so softmax is a
  gather of one v row that every path must reproduce bit for bit; a zero-filled padded key would score 0 and win if the mask leaked.
* Refusals: N % area != 0 launches nothing."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from gpu_util import tuned  # noqa: E402
from group_attn_util import data as _data, groups, lib as _L, one_hot, ref, run, ulp as _ulp  # noqa: E402

AREA_F32, AREA_F16, AREA_MFMA = 401, 402, 403
WORST = {}


def _run(q, k, v, heads, area, scale, dtype):
    """-> y logical (B,C,H,W) float64 cpu"""
    from edge_yolo_amd.nn import _ops
    return run(lambda qv, kv, vv, yv: _ops.area_attention(qv, kv, vv, heads, area, scale, out=yv), q, k, v, dtype)


def _check(case, got, q, k, v, heads, area, scale, dtype, mfma):
    y, Y, Amax, _, _ = ref(q, k, v, heads, scale, area)
    Na = q.shape[2] * q.shape[3] // area
    u = 2.0 ** -24
    # score error: fp32 sums of hd exact products (2 hd u |s|), scale multiply; propagated through exp (relative) for every key
    # against the row max -> 2 * (2 hd + 2) u * max|s| relative on P; exp itself 2^-21 relative; the P.V sum over Na keys in fp32
    rel = 2 * (2 * q.shape[1] // heads + 2) * u * Amax + 2.0 ** -20 + 2 * Na * u
    if mfma:
        rel = rel + 2.0 ** -11  # P rounded to f16 before the MFMA
    bnd = rel * Y * 1.25 + _ulp(y, dtype) + 2.0 ** -30  # (a whole ulp: the kernel's value may round across a binade boundary)
    err = (groups(got, heads, area) - y).abs()
    assert torch.isfinite(got).all(), f"{case}: non-finite output"
    r = float((err / bnd).max())
    print(f"[fp64] {case} max err/bound {r:.3f}")
    fam = "mfma" if mfma else ("f16" if dtype == torch.float16 else "f32")
    WORST[fam] = max(WORST.get(fam, (0.0, "")), (r, case))
    assert r <= 1.0, f"{case}: max err/bound {r:.3f}"


# (B, H, W, area, heads): tokens per area in the comment
CASES = [
    (1, 1, 1, 1, 1),      # 1
    (2, 2, 3, 1, 2),      # 6
    (2, 6, 10, 4, 2),     # 15, areas split rows
    (1, 4, 4, 1, 3),      # 16
    (1, 1, 17, 1, 4),     # 17
    (2, 12, 20, 1, 5),    # 240
    (1, 16, 15, 1, 8),    # 240, 8 heads
    (2, 40, 40, 4, 2),    # 400 (layer 6 of yolov12n at 640)
    (2, 20, 20, 1, 4),    # 400 (layer 8)
    (1, 1, 401, 1, 1),    # 401
    (1, 40, 40, 1, 6),    # 1600 (1280 input)
    (1, 80, 80, 4, 7),    # 1600 per area
]


@pytest.mark.parametrize("B,H,W,area,heads", CASES)
@pytest.mark.parametrize("path", ["mfma", "f32"])
def test_area_attention_bounded(B, H, W, area, heads, path):
    L = _L()
    hd = 32
    q, k, v = _data(B, H, W, heads, hd, (B, H, W, area, heads))
    dtype = torch.float16 if path == "mfma" else torch.float32
    scale = hd ** -0.5
    got = _run(q, k, v, heads, area, scale, dtype)
    assert L.lib().ey_attention_last_variant() == (AREA_MFMA if path == "mfma" else AREA_F32)
    _check(f"{path} B{B} {H}x{W} area{area} h{heads}", got, q, k, v, heads, area, scale, dtype, path == "mfma")


@pytest.mark.parametrize("hd,knob", [(16, None), (32, {"areaattn_mfma": 0}), (64, None)])
def test_area_attention_f16_valu(hd, knob):
    L = _L()
    B, H, W, area, heads = 2, 6, 10, 4, 2
    q, k, v = _data(B, H, W, heads, hd, ("valu", hd))
    with tuned(**(knob or {})):
        got = _run(q, k, v, heads, area, hd ** -0.5, torch.float16)
        assert L.lib().ey_attention_last_variant() == AREA_F16
    _check(f"f16 valu hd{hd}", got, q, k, v, heads, area, hd ** -0.5, torch.float16, False)


@pytest.mark.parametrize("B,H,W,area,heads", [(1, 1, 1, 1, 1), (2, 6, 10, 4, 2), (1, 1, 17, 1, 3), (1, 5, 80, 1, 2), (1, 1, 401, 1, 1),
                                              (1, 40, 40, 4, 2)])
@pytest.mark.parametrize("path", ["mfma", "f32", "f16valu"])
def test_area_attention_one_hot_exact(B, H, W, area, heads, path):
    L = _L()
    q, k, v = one_hot(B, H, W, heads, area, 32, ("onehot", B, H, W, area, heads))
    dtype = torch.float32 if path == "f32" else torch.float16
    with tuned(**({"areaattn_mfma": 0} if path == "f16valu" else {})):
        got = _run(q, k, v, heads, area, 32 ** -0.5, dtype)
        assert L.lib().ey_attention_last_variant() == {"mfma": AREA_MFMA, "f32": AREA_F32, "f16valu": AREA_F16}[path]
    y = ref(q, k, v, heads, 32 ** -0.5, area)[0]
    got = groups(got, heads, area)
    assert torch.equal(got, y.to(dtype).double()), f"{path}: one-hot gather not bit-exact (max diff {float((got - y).abs().max())})"


def test_area_attention_refusals():
    L = _L()
    from edge_yolo_amd.nn import _ops
    q = torch.zeros(1, 64, 5, 5, dtype=torch.float16, device="cuda")
    with pytest.raises(ValueError, match="equal areas"):
        _ops.area_attention(q, q, q, 2, 4, 0.17)
    p = q.data_ptr()
    rc = L.lib().ey_area_attention(L.F16, 1, 25, 4, 2, 32, 0.17, p, 64, p, 64, p, 64, p, 64, L.stream())
    assert rc == -1 and L.lib().ey_attention_last_variant() == 0
    rc = L.lib().ey_area_attention(L.F32, 1, 25, 1, 1, 128, 0.17, p, 128, p, 128, p, 128, p, 128, L.stream())
    assert rc == -2 and L.lib().ey_attention_last_variant() == 0


def test_zz_worst_report():
    for fam, (r, case) in sorted(WORST.items()):
        print(f"[fp64] worst {fam}: err/bound {r:.3f} at {case}")
