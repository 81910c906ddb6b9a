"""-m gpu: ey_stem_conv_ks -- the image stems (k, s, p) = (6, 2, 2) of YOLOv5 and (3, 1, 1) of YOLOv3, planar NCHW image in, NHWC out --
against the fp64 reference of tests/fp64_ref.py, in the idiom of tests/test_gpu_conv_exact.py.

* Exact matrix: integer images in [-2, 2], weights and biases in multiples of 1/4, act none / ReLU: every partial sum is exact in fp32 (at most
  108 taps of magnitude <= 2 plus a bias <= 2: |y| <= 218 < 512, exact in f16 too), so the output must be BIT-IDENTICAL to fp64 in both dtypes.
  2x2 (one output pixel at stride 2), 12x20, 34x50 (VALU form, ragged) and 24x136 (MFMA form in f16: crosses a 64-column and an 8-row tile),
  B = 2, Cout 16 / 48 / 80, the output a slot of a wider buffer.  Each case asserts the label it launched.
* Single-tap probes: one non-zero pixel (corners, last row, last column, both sides of the tile seams): the output is the shifted weight
  pattern, stated here by index arithmetic of its own -- the 6x6 window of output o covers the inputs 2o - 2 ... 2o + 3.
* Bounded: f16, SiLU, general data against the per-element fp64 bound and the mean-ulp gate of fp64_ref.report.
* (5, 2, 2) is refused with EY_EUNSUPPORTED and launches nothing."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import fp64_ref as R  # noqa: E402
from gpu_util import _traced  # noqa: E402

DT = [torch.float16, torch.float32]
KSP = [(6, 2, 2), (3, 1, 1)]
STEM = {(6, 2, 2): "stem6", (3, 1, 1): "stem3s1"}
SHAPES = [(2, 2), (12, 20), (34, 50), (24, 136)]
COUTS = [16, 48, 80]
B = 2


def _label(ksp, dtype, W):
    return STEM[ksp] + ("_mfma_kernel" if dtype == torch.float16 and W % 8 == 0 else "_kernel")


def _run(ksp, x, w, b, act, cout, pad_c=24):
    """ops.stem_conv_ks into channels [8, 8 + cout) of a (cout + pad_c)-channel NHWC buffer -> (output view, whole buffer, labels)."""
    from edge_yolo_amd import _lib as L
    from edge_yolo_amd.nn import _ops as ops
    from edge_yolo_amd.nn.modules.conv import _Packed
    k, s, p = ksp
    Bn, _, H, W = x.shape
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    buf = L.empty_nhwc(Bn, cout + pad_c, Ho, Wo, x.dtype, x.device)
    buf.fill_(7.0)
    out = buf[:, 8:8 + cout]
    mod = _Packed()
    _, labels = _traced(lambda: ops.stem_conv_ks(mod, x, lambda: (w.float(), b.float()), k, s, p, act, x.dtype, out=out))
    return out, buf, labels


def _check_slot(buf, cout):
    assert bool((buf[:, :8] == 7.0).all()) and bool((buf[:, 8 + cout:] == 7.0).all()), "the kernel wrote outside its channel slot"


@pytest.mark.parametrize("dtype", DT, ids=["f16", "f32"])
@pytest.mark.parametrize("cout", COUTS)
@pytest.mark.parametrize("hw", SHAPES, ids=[f"{h}x{w}" for h, w in SHAPES])
@pytest.mark.parametrize("ksp", KSP, ids=["k6s2p2", "k3s1p1"])
def test_exact_matrix(ksp, hw, cout, dtype):
    k, s, p = ksp
    H, W = hw
    gen = torch.Generator().manual_seed(1000 * k + 10 * H + cout + (dtype == torch.float16))
    x = R.ex_input((B, 3, H, W), gen)
    w = R.ex_weight((cout, 3, k, k), gen)
    b = R.ex_bias(cout, gen)
    act = R.ACT_RELU if cout == 48 else R.ACT_NONE
    got, buf, labels = _run(ksp, x.to(dtype).cuda().contiguous(), w, b, act, cout)
    assert labels == [_label(ksp, dtype, W)], labels
    y, _, _ = R.conv_ref([x.cuda()], w, b, k, s, p, act)
    R.assert_exact(f"stem {ksp} {H}x{W} cout{cout}", labels[0], got, y)
    _check_slot(buf, cout)


# probe pixels (iy, ix) by image size: the corners, the last row and column, and both sides of the tile seams of the MFMA form (an 8 x 64
# output tile: output row 8 / column 64 start at input row / column 16 / 128 at stride 2 and 8 / 64 at stride 1)
def _probes(H, W, s):
    pts = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (H - 1, W // 2), (H // 2, W - 1)]
    for iy in (8 * s - 1, 8 * s, 8 * s + 1):
        for ix in (64 * s - 1, 64 * s, 64 * s + 1):
            if iy < H and ix < W:
                pts.append((iy, ix))
    return pts


@pytest.mark.parametrize("dtype", DT, ids=["f16", "f32"])
@pytest.mark.parametrize("hw", [(34, 50), (24, 136)], ids=["34x50", "24x136"])
@pytest.mark.parametrize("ksp", KSP, ids=["k6s2p2", "k3s1p1"])
def test_single_tap_probes(ksp, hw, dtype):
    k, s, p = ksp
    H, W = hw
    cout = 16
    gen = torch.Generator().manual_seed(77 + k)
    w = R.ex_weight((cout, 3, k, k), gen)
    w[w == 0] = 0.5  # every tap visible
    b = torch.zeros(cout)
    pts = _probes(H, W, s)
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    x = torch.zeros((len(pts), 3, H, W), dtype=torch.float64)
    want = torch.zeros((len(pts), cout, Ho, Wo), dtype=torch.float64)
    for n, (iy, ix) in enumerate(pts):
        c = n % 3
        x[n, c, iy, ix] = 2.0
        for oy in range(Ho):  # output (oy, ox) reads input (oy s - p + ky, ox s - p + kx), ky, kx = 0 ... k - 1: at (6, 2, 2) the rows 2 oy - 2 ... 2 oy + 3
            ky = iy - (oy * s - p)
            if not 0 <= ky < k:
                continue
            for ox in range(Wo):
                kx = ix - (ox * s - p)
                if 0 <= kx < k:
                    want[n, :, oy, ox] = 2.0 * w[:, c, ky, kx]
    got, buf, labels = _run(ksp, x.to(dtype).cuda().contiguous(), w, b, R.ACT_NONE, cout)
    assert labels == [_label(ksp, dtype, W)], labels
    R.assert_exact(f"stem probe {ksp} {H}x{W}", labels[0], got, want.cuda())
    y, _, _ = R.conv_ref([x.cuda()], w, b, k, s, p, R.ACT_NONE)  # and the reference conv agrees with the index arithmetic above
    assert torch.equal(y.cpu(), want)
    _check_slot(buf, cout)


@pytest.mark.parametrize("cout", [16, 80])
@pytest.mark.parametrize("hw", [(34, 50), (24, 136)], ids=["34x50", "24x136"])
@pytest.mark.parametrize("ksp", KSP, ids=["k6s2p2", "k3s1p1"])
def test_bounded_f16_silu(ksp, hw, cout):
    k, s, p = ksp
    H, W = hw
    gen = torch.Generator().manual_seed(5 + k + cout)
    x = torch.randn((B, 3, H, W), generator=gen).half()
    w = (torch.randn((cout, 3, k, k), generator=gen) / (3 * k * k) ** 0.5).float()
    b = torch.randn(cout, generator=gen).float() * 0.5
    got, buf, labels = _run(ksp, x.cuda().contiguous(), w, b, R.ACT_SILU, cout)
    assert labels == [_label(ksp, torch.float16, W)], labels
    wk = w.half() if labels[0].endswith("_mfma_kernel") else w  # the MFMA form rounds the weights to f16; the VALU form keeps them in fp32
    y, A, Y = R.conv_ref([x.cuda()], wk, b, k, s, p, R.ACT_SILU)
    R.report(f"stem {ksp} {H}x{W} cout{cout}", labels[0], got, y, R.bound(y, A, Y, R.nterms(3, k)))
    _check_slot(buf, cout)


def test_unsupported_shape_launches_nothing():
    from edge_yolo_amd import _lib as L
    from edge_yolo_amd.nn import _ops as ops
    from edge_yolo_amd.nn.modules.conv import _Packed
    x = torch.zeros((1, 3, 16, 16), dtype=torch.float16, device="cuda")
    w, b = torch.zeros((16, 3, 5, 5), device="cuda"), torch.zeros(16, device="cuda")
    y = L.empty_nhwc(1, 16, 8, 8, torch.float16, x.device)
    y.fill_(3.0)
    code = L.lib().ey_stem_conv_ks(L.F16, L.F16, 1, 3, 16, 16, 16, 5, 2, 2, L.ACT_NONE, x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), 16, L.stream())
    assert code == -2, code  # EY_EUNSUPPORTED
    assert b"stem_ks" in L.lib().ey_last_error()
    mod = _Packed()

    def call():
        with pytest.raises(NotImplementedError):
            ops.stem_conv_ks(mod, x, lambda: (w, b), 5, 2, 2, L.ACT_NONE, x.dtype, out=y)

    _, labels = _traced(call)
    assert labels == []
    torch.cuda.synchronize()
    assert bool((y == 3.0).all())
