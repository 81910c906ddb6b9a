"""-m gpu: the operators of the ResNet backbones.

* ey_maxpool3x3s2 (nn.MaxPool2d(3, 2, 1), the padding left out of the maximum): bit-equal to torch's CPU F.max_pool2d(x, 3, 2, 1), f16 and
  fp32, at 1x1, 6x5, 17x24 (more than one block), as a channel slot of a wider buffer, and on an all-negative map (a zero-padded pool would
  give 0 on the border); a NaN cell makes every window that holds it NaN, as in torch.  ey_maxpool2d and ops.maxpool2d keep refusing a 3x3 window.
* ey_stem_conv_ks at (7, 2, 3): against tests/fp64_ref.py in the idiom of tests/test_gpu_stem_ks.py -- a dyadic exact probe (147 taps of
  magnitude <= 2 plus a bias <= 2: |y| <= 296 < 512, exact in f16), bit for bit in both dtypes, and f16 SiLU on general data under
  bound(y, A, Y, nterms(3, 7)) -- at 1x1, 16x16, 33x47 (the VALU form) and 64x72 (more than one MFMA tile both ways).  (5, 2, 2) stays refused.
* ey_resnet_stem (layer 0 as one launch): bit-equal to ey_stem_conv_ks (7, 2, 3) + ey_maxpool3x3s2 at the four stem images and at 40x136 / 41x131,
  which span more than one pooled tile both ways in the MFMA and the VALU form, f16 and fp32, batch 2, into a channel slot; zero weights with a
  negative bias give silu(bias) everywhere; the trace shows one launch; refused shapes launch nothing.
* The closing 1x1 of a ResNetBlock, relu(W3 t + b3 + shortcut(x)), as the module runs it -- fused: ONE ey_resnet_tail launch (f16; x read at
  pixel stride s, [W3 | Ws] along K; the residual of an identity block added in fp32 before the ReLU); composed: the shortcut conv where
  there is one, then ey_conv2d with ReLU and the shortcut / the block input as its same-size pre-activation term -- against
  conv_ref([t, x[..., ::s, ::s]], [W3 | Ws], b3 + bs, ReLU), for the identity block conv_ref([t], W3, b3, ReLU, addz = x), under
  fp64_ref.bound with one more accumulated term than the taps and the bias for the added map.  The composed projection stores the shortcut
  map in f16 (fp32) before it is added; its bound carries one unit of that map for it, the fused kernel and the identity forms carry nothing.
  A dyadic probe is bit-exact in every form.  Channel slots; refused shapes (fp32, widths off the list, a wrong residual) launch nothing.
* ey_classify_pool at C1 = 2048 and 2024 (above the 64 KiB LDS tile of the f16 form), HW 1 / 4 / 49, under fp64_cls_ref.pool_bound."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import cls_synth  # noqa: E402
import fp64_cls_ref as f64c  # noqa: E402
import fp64_ref as R  # noqa: E402
import resnet_synth as rs  # noqa: E402
from gpu_util import _traced  # noqa: E402

DT = [torch.float16, torch.float32]


def _nhwc(x, dt, lead=0, extra=0, fill=float("nan")):
    """(B, C, H, W) -> NHWC device view, a channel window [lead, lead + C) of a `fill`ed buffer when lead or extra is set -> (view, buffer)."""
    from edge_yolo_amd import _lib as L
    B, C, H, W = x.shape
    buf = L.empty_nhwc(B, lead + C + extra, H, W, dt, "cuda")
    buf.fill_(fill)
    v = buf[:, lead:lead + C]
    v.copy_(torch.as_tensor(x).to(dt))
    return v, buf


# ------------------------------------------------------------------------------------------------------------------ ey_maxpool3x3s2
@pytest.mark.parametrize("dtype", DT, ids=["f16", "f32"])
@pytest.mark.parametrize("negative", [False, True], ids=["normal", "all-negative"])
@pytest.mark.parametrize("case", rs.POOL_CASES, ids=[c[0] for c in rs.POOL_CASES])
def test_maxpool3x3s2_equals_torch(case, negative, dtype):
    from edge_yolo_amd.nn import _ops as ops
    tag, B, C, H, W = case
    x = torch.tensor(rs.pool_input(tag, (B, C, H, W), negative)).to(dtype)
    want = F.max_pool2d(x.float(), 3, 2, 1).to(dtype)  # (exact: a maximum of f16 values is one of them)
    xv, _ = _nhwc(x, dtype)
    got, labels = _traced(lambda: ops.maxpool3x3s2(xv))
    assert labels == ["maxpool3x3s2_kernel"] and tuple(got.shape) == tuple(want.shape) == (B, C, (H - 1) // 2 + 1, (W - 1) // 2 + 1)
    assert torch.equal(got.cpu(), want)
    if negative:
        assert bool((got < 0).all())


@pytest.mark.parametrize("dtype", DT, ids=["f16", "f32"])
def test_maxpool3x3s2_channel_slots(dtype):
    from edge_yolo_amd import _lib as L
    from edge_yolo_amd.nn import _ops as ops
    tag, B, C, H, W = "mp_slot", 2, 16, 9, 7
    x = torch.tensor(rs.pool_input(tag, (B, C, H, W))).to(dtype)
    xv, _ = _nhwc(x, dtype, lead=8, extra=8)
    Ho, Wo = 5, 4
    buf = L.empty_nhwc(B, C + 24, Ho, Wo, dtype, "cuda")
    buf.fill_(7.0)
    out = buf[:, 16:16 + C]
    got = ops.maxpool3x3s2(xv, out=out)
    assert got.data_ptr() == out.data_ptr()
    assert torch.equal(got.cpu(), F.max_pool2d(x.float(), 3, 2, 1).to(dtype))
    assert bool((buf[:, :16] == 7.0).all()) and bool((buf[:, 16 + C:] == 7.0).all()), "the kernel wrote outside its channel slot"


@pytest.mark.parametrize("dtype", DT, ids=["f16", "f32"])
def test_maxpool3x3s2_propagates_nan_like_torch(dtype):
    from edge_yolo_amd.nn import _ops as ops
    x = torch.tensor(rs.pool_input("mp_nan", (1, 8, 7, 6))).to(dtype)
    x[0, 3, 2, 3] = float("nan")
    x[0, 5, 6, 0] = float("nan")
    want = F.max_pool2d(x.float(), 3, 2, 1).to(dtype)
    got = ops.maxpool3x3s2(_nhwc(x, dtype)[0]).cpu()
    assert int(want.isnan().sum()) >= 3 and torch.equal(got.isnan(), want.isnan()) and torch.equal(got.nan_to_num(0.0), want.nan_to_num(0.0))


def test_maxpool_refusals():
    from edge_yolo_amd import _lib as L
    from edge_yolo_amd.nn import _ops as ops
    x = L.empty_nhwc(1, 12, 4, 4, torch.float16, "cuda")
    y = L.empty_nhwc(1, 12, 2, 2, torch.float16, "cuda")
    y.fill_(3.0)
    assert L.lib().ey_maxpool3x3s2(L.F16, 1, 4, 4, 12, x.data_ptr(), 12, y.data_ptr(), 12, L.stream()) == -2  # C % 8: EY_EUNSUPPORTED
    assert b"maxpool3x3s2" in L.lib().ey_last_error()
    _, labels = _traced(lambda: pytest.raises(NotImplementedError, ops.maxpool3x3s2, x))
    assert labels == []
    torch.cuda.synchronize()
    assert bool((y == 3.0).all())
    x8 = L.empty_nhwc(1, 8, 6, 6, torch.float16, "cuda")
    with pytest.raises(NotImplementedError):  # the zero-padded pool keeps refusing a 3x3 window
        ops.maxpool2d(x8, 3, 2)
    assert L.lib().ey_maxpool2d(L.F16, 1, 6, 6, 8, 3, 2, 1, 1, 1, 1, x8.data_ptr(), 8, y.data_ptr(), 8, L.stream()) == -2


# ------------------------------------------------------------------------------------------------------------------ stem (7, 2, 3)
KSP = (7, 2, 3)


def _stem(x, w, b, act, cout, pad_c=24):
    from edge_yolo_amd import _lib as L
    from edge_yolo_amd.nn import _ops as ops
    from edge_yolo_amd.nn.modules.conv import _Packed
    k, s, p = KSP
    Bn, _, H, W = x.shape
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    buf = L.empty_nhwc(Bn, cout + pad_c, Ho, Wo, x.dtype, x.device)
    buf.fill_(7.0)
    out = buf[:, 8:8 + cout]
    _, labels = _traced(lambda: ops.stem_conv_ks(_Packed(), x, lambda: (w.float(), b.float()), k, s, p, act, x.dtype, out=out))
    assert bool((buf[:, :8] == 7.0).all()) and bool((buf[:, 8 + cout:] == 7.0).all()), "the kernel wrote outside its channel slot"
    return out, labels


def _stem_label(dtype, W):
    return "stem7" + ("_mfma_kernel" if dtype == torch.float16 and W % 8 == 0 else "_kernel")


@pytest.mark.parametrize("dtype", DT, ids=["f16", "f32"])
@pytest.mark.parametrize("hw", rs.STEM_IMAGES, ids=[f"{h}x{w}" for h, w in rs.STEM_IMAGES])
def test_stem7_exact_probe(hw, dtype):
    H, W = hw
    gen = torch.Generator().manual_seed(7000 + 10 * H + (dtype == torch.float16))
    x = R.ex_input((2, 3, H, W), gen)
    w = R.ex_weight((64, 3, 7, 7), gen)
    b = R.ex_bias(64, gen)
    got, labels = _stem(x.to(dtype).cuda().contiguous(), w, b, R.ACT_NONE, 64)
    assert labels == [_stem_label(dtype, W)], labels
    y, _, _ = R.conv_ref([x.cuda()], w, b, 7, 2, 3, R.ACT_NONE)
    assert tuple(y.shape[2:]) == ((H - 1) // 2 + 1, (W - 1) // 2 + 1)
    R.assert_exact(f"stem7 {H}x{W}", labels[0], got, y)


@pytest.mark.parametrize("hw", rs.STEM_IMAGES, ids=[f"{h}x{w}" for h, w in rs.STEM_IMAGES])
def test_stem7_bounded_f16_silu(hw):
    H, W = hw
    gen = torch.Generator().manual_seed(70 + H)
    x = torch.randn((2, 3, H, W), generator=gen).half()
    w = (torch.randn((64, 3, 7, 7), generator=gen) / 147 ** 0.5).float()
    b = torch.randn(64, generator=gen).float() * 0.5
    got, labels = _stem(x.cuda().contiguous(), w, b, R.ACT_SILU, 64)
    assert labels == [_stem_label(torch.float16, W)], labels
    wk = w.half() if labels[0].endswith("_mfma_kernel") else w  # the MFMA form rounds the weights to f16; the VALU form keeps them in fp32
    y, A, Y = R.conv_ref([x.cuda()], wk, b, 7, 2, 3, R.ACT_SILU)
    R.report(f"stem7 {H}x{W}", labels[0], got, y, R.bound(y, A, Y, R.nterms(3, 7)))


def test_stem7_layer0_sizes():
    """layer 0 of a ResNet in both forms: 33x47 -> 9x12, 32x32 -> 8x8, 30x34 -> 8x9; one launch fused, two launches otherwise, the same bits."""
    from edge_yolo_amd.nn import modules as M
    layer = M.ResNetLayer(3, 64, 1, True, 1).cuda().half().eval()
    for (H, W), want in (((33, 47), (9, 12)), ((32, 32), (8, 8)), ((30, 34), (8, 9))):
        x = torch.rand(1, 3, H, W, dtype=torch.float16, device="cuda")
        layer.stem_fused = True
        y1, labels = _traced(lambda: layer(x))
        assert tuple(y1.shape) == (1, 64) + want and labels == ["resnet_stem_mfma_kernel" if W % 8 == 0 else "resnet_stem_kernel"], (labels, tuple(y1.shape))
        layer.stem_fused = False
        y2, labels = _traced(lambda: layer(x))
        assert len(labels) == 2 and labels[1] == "maxpool3x3s2_kernel" and torch.equal(y1, y2), labels


# ------------------------------------------------------------------------------------------------------------------ ey_resnet_stem
# the stem images, and two that span more than one pooled tile (3 x 30 pooled pixels) in both directions: MFMA form and VALU form
FUSED_IMAGES = rs.STEM_IMAGES + [(40, 136), (41, 131)]


def _fused_label(dtype, W):
    return "resnet_stem_mfma_kernel" if dtype == torch.float16 and W % 8 == 0 else "resnet_stem_kernel"


def _stem_pair_and_fused(x, w, b, act):
    """(ey_stem_conv_ks (7, 2, 3) + ey_maxpool3x3s2, ey_resnet_stem into a channel slot of a wider buffer, the fused call's labels)."""
    from edge_yolo_amd import _lib as L
    from edge_yolo_amd.nn import _ops as ops
    from edge_yolo_amd.nn.modules.conv import _Packed
    mod, folded = _Packed(), (lambda: (w.float(), b.float()))
    pair = ops.maxpool3x3s2(ops.stem_conv_ks(mod, x, folded, 7, 2, 3, act, x.dtype))
    buf = L.empty_nhwc(x.shape[0], 64 + 24, pair.shape[2], pair.shape[3], x.dtype, x.device)
    buf.fill_(7.0)
    out = buf[:, 8:8 + 64]
    got, labels = _traced(lambda: ops.resnet_stem(mod, x, folded, act, out=out))
    assert got.data_ptr() == out.data_ptr()
    assert bool((buf[:, :8] == 7.0).all()) and bool((buf[:, 8 + 64:] == 7.0).all()), "the kernel wrote outside its channel slot"
    return pair, got, labels


@pytest.mark.parametrize("dtype", DT, ids=["f16", "f32"])
@pytest.mark.parametrize("hw", FUSED_IMAGES, ids=[f"{h}x{w}" for h, w in FUSED_IMAGES])
def test_resnet_stem_equals_stem_plus_pool(hw, dtype):
    H, W = hw
    gen = torch.Generator().manual_seed(90 + H)
    x = torch.randn((2, 3, H, W), generator=gen).to(dtype).cuda().contiguous()
    w = (torch.randn((64, 3, 7, 7), generator=gen) / 147 ** 0.5).float()
    b = torch.randn(64, generator=gen).float() * 0.5
    pair, got, labels = _stem_pair_and_fused(x, w, b, R.ACT_SILU)
    assert labels == [_fused_label(dtype, W)], labels  # one launch
    assert tuple(got.shape) == tuple(pair.shape) == (2, 64, ((H - 1) // 2) // 2 + 1, ((W - 1) // 2) // 2 + 1)
    assert torch.equal(got, pair), f"{int((got != pair).sum())} of {got.numel()} values differ from stem + pool"


@pytest.mark.parametrize("dtype", DT, ids=["f16", "f32"])
@pytest.mark.parametrize("hw", [(16, 16), (33, 47), (40, 136)], ids=["16x16", "33x47", "40x136"])
def test_resnet_stem_zero_weights_negative_bias(hw, dtype):
    """every window of the pool holds silu(bias) only; a pool whose padding took part (zeros, or a stale LDS cell) would show at the border."""
    H, W = hw
    x = torch.randn((2, 3, H, W), generator=torch.Generator().manual_seed(3)).to(dtype).cuda().contiguous()
    w = torch.zeros((64, 3, 7, 7))
    b = -(torch.arange(64).float() + 1.0) / 16.0
    pair, got, labels = _stem_pair_and_fused(x, w, b, R.ACT_SILU)
    assert labels == [_fused_label(dtype, W)], labels
    want = torch.nn.functional.silu(b.double()).view(1, 64, 1, 1).expand_as(got)
    assert torch.equal(got, pair) and bool((got < 0).all())
    assert bool((got[:, :, :1, :1].expand_as(got) == got).all())  # one value per channel everywhere
    torch.testing.assert_close(got.double().cpu(), want, rtol=2.0 ** -10 if dtype == torch.float16 else 1e-5, atol=0.0)  # (one f16 ulp; fp32: the device's exp)


def test_resnet_stem_refused_shapes_launch_nothing():
    from edge_yolo_amd import _lib as L
    x = torch.zeros((1, 3, 16, 16), dtype=torch.float16, device="cuda")
    w, b = torch.zeros((64, 3, 7, 7), device="cuda"), torch.zeros(64, device="cuda")
    y = L.empty_nhwc(1, 64, 4, 4, torch.float16, x.device)
    y.fill_(3.0)

    def call(xd=L.F16, yd=L.F16, cin=3, cout=64, cs=64):
        return L.lib().ey_resnet_stem(xd, yd, 1, cin, 16, 16, cout, L.ACT_NONE, x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), cs, L.stream())

    assert call(yd=L.F32) == -2 and b"resnet_stem" in L.lib().ey_last_error()
    assert call(cout=32) == -2 and call(cin=5) == -2 and call(cs=68) == -2
    torch.cuda.synchronize()
    assert bool((y == 3.0).all())


def test_stem_unsupported_window_launches_nothing():
    from edge_yolo_amd import _lib as L
    x = torch.zeros((1, 3, 16, 16), dtype=torch.float16, device="cuda")
    w, b = torch.zeros((16, 3, 5, 5), device="cuda"), torch.zeros(16, device="cuda")
    y = L.empty_nhwc(1, 16, 8, 8, torch.float16, x.device)
    y.fill_(3.0)
    for k, s, p in ((5, 2, 2), (7, 1, 3), (7, 2, 2)):
        code = L.lib().ey_stem_conv_ks(L.F16, L.F16, 1, 3, 16, 16, 16, k, s, p, L.ACT_NONE, x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), 16, L.stream())
        assert code == -2, (k, s, p, code)
    torch.cuda.synchronize()
    assert bool((y == 3.0).all())


# ------------------------------------------------------------------------------------------------------------------ the block tail
def _block(C1, C2, s, w3, ws, b, dtype):
    """a ResNetBlock whose cv3 / shortcut hold (w3, b) / (ws, 0): BatchNorms set to the identity (eps 0, unit variance)."""
    from edge_yolo_amd.nn import modules as M
    blk = M.ResNetBlock(C1 if C1 else 4 * C2, C2, s)
    convs = [(blk.cv3, w3, b)] + ([(blk.shortcut[0], ws, np.zeros_like(b))] if C1 else [])
    for conv, w, bias in convs:
        conv.conv.weight.data.copy_(torch.tensor(w).view_as(conv.conv.weight))
        conv.bn.weight.data.fill_(1.0)
        conv.bn.bias.data.copy_(torch.tensor(bias))
        conv.bn.running_mean.zero_()
        conv.bn.running_var.fill_(1.0)
        conv.bn.eps = 0.0
    assert isinstance(blk.shortcut, torch.nn.Sequential) == bool(C1)
    blk = blk.cuda().eval()
    return blk.half() if dtype == torch.float16 else blk.float()


TAIL_RUNS = [(c, "fused", torch.float16) for c in rs.TAIL_CASES] + [(c, "composed", dt) for c in rs.TAIL_CASES for dt in DT]  # (the fused kernel is f16 only)
TAIL_IDS = [f"{c[0]}-{f}-{'f16' if dt == torch.float16 else 'f32'}" for c, f, dt in TAIL_RUNS]


def _tail(blk, t, x):
    """the module's own tail on given t = cv2(cv1(x)) and x -> (y, labels)."""
    return _traced(lambda: blk.tail(t, x))


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "bounded"])
@pytest.mark.parametrize("case,form,dtype", TAIL_RUNS, ids=TAIL_IDS)
def test_block_tail(case, form, dtype, exact):
    tag, B, C1, C2, s, H, W = case
    t, x, w3, ws, b = rs.tail_case(*case, exact=exact)
    if exact and C2 + C1 > 256:  # keep |y| < 512: thin the weights out (inputs |x| <= 2, weights <= 1/2)
        gen = torch.Generator().manual_seed(C1 + C2)
        dens = R.safe_density(C1 + C2, cap=800.0)
        w3 = w3 * (torch.rand(w3.shape, generator=gen) < dens).numpy().astype(np.float32)
        ws = ws * (torch.rand(ws.shape, generator=gen) < dens).numpy().astype(np.float32)
    if dtype == torch.float16:  # a half() module holds its BatchNorm bias in f16: the reference gets the value the kernel sees
        b = b.astype(np.float16).astype(np.float32)
    blk = _block(C1, C2, s, w3, ws, b, dtype)
    blk.tail_fused = form == "fused"
    tv, _ = _nhwc(t, dtype)
    xv, _ = _nhwc(x, dtype)
    got, labels = _tail(blk, tv, xv)
    if form == "fused":
        assert labels == ["resnet_tail_kernel"], labels
    else:
        assert len(labels) == (2 if C1 else 1) and "resnet_tail_kernel" not in labels, labels
    T, X = torch.tensor(t).double().cuda(), torch.tensor(x).double().cuda()
    if C1:
        wcat = torch.tensor(np.concatenate([w3, ws], 1)).double().view(4 * C2, C2 + C1, 1, 1)
        y, A, Y = R.conv_ref([T, X[..., ::s, ::s]], wcat, torch.tensor(b), 1, 1, 0, R.ACT_RELU)
    else:
        y, A, Y = R.conv_ref([T], torch.tensor(w3).double().view(4 * C2, C2, 1, 1), torch.tensor(b), 1, 1, 0, R.ACT_RELU, addz=X)
    assert tuple(got.shape) == tuple(y.shape) == (B, 4 * C2, (H - 1) // s + 1, (W - 1) // s + 1)
    if exact:
        R.assert_exact(f"{tag} {form}", labels[-1], got, y)
        return
    K = C2 + C1 + 1 + 1  # the taps, the bias, and one more accumulated term for the added map
    bnd = R.bound(y, A, Y, K, f16_out=dtype == torch.float16)
    if form == "composed" and C1:
        # the plain composition stores the shortcut conv's output in the storage type before cv3 adds it: the fp64 value of that map, rounded,
        # may be off by one unit of it (half a unit of rounding, and the fp32 sum under it may fall on the other side)
        wsd = torch.tensor(ws).double().view(4 * C2, C1, 1, 1)
        z, _, _ = R.conv_ref([X[..., ::s, ::s]], wsd, None, 1, 1, 0, R.ACT_NONE)
        bnd = bnd + (R.ulp16(z) if dtype == torch.float16 else z.abs() * 2.0 ** -23)
    R.report(f"{tag} {form}", labels[-1], got, y, bnd)


def test_block_tail_channel_slots():
    """t, x and the output as channel slots of wider buffers (NaN around the sources): the kernel reads its windows only and writes its own."""
    from edge_yolo_amd import _lib as L
    case = rs.TAIL_CASES[3]  # projection, stride 2
    tag, B, C1, C2, s, H, W = case
    t, x, w3, ws, b = rs.tail_case(*case)
    blk = _block(C1, C2, s, w3, ws, b.astype(np.float16).astype(np.float32), torch.float16)
    blk.tail_fused = True
    tv, _ = _nhwc(t, torch.float16, lead=8, extra=8)
    xv, _ = _nhwc(x, torch.float16, lead=16, extra=8)
    buf = L.empty_nhwc(B, 4 * C2 + 24, 5, 4, torch.float16, "cuda")
    buf.fill_(7.0)
    out = buf[:, 8:8 + 4 * C2]
    got, labels = _traced(lambda: blk.tail(tv, xv, out=out))
    assert labels == ["resnet_tail_kernel"] and got.data_ptr() == out.data_ptr()
    want, _ = _tail(blk, _nhwc(t, torch.float16)[0], _nhwc(x, torch.float16)[0])
    assert torch.equal(got, want) and bool(torch.isfinite(got).all())
    assert bool((buf[:, :8] == 7.0).all()) and bool((buf[:, 8 + 4 * C2:] == 7.0).all()), "the kernel wrote outside its channel slot"


def test_block_tail_refused_shapes_launch_nothing():
    from edge_yolo_amd import _lib as L
    from edge_yolo_amd.nn import modules as M
    t = L.empty_nhwc(1, 64, 2, 2, torch.float16, "cuda")
    x = L.empty_nhwc(1, 64, 2, 2, torch.float16, "cuda")
    w = torch.zeros((256, 128), dtype=torch.float16, device="cuda")
    b = torch.zeros(256, device="cuda")
    y = L.empty_nhwc(1, 256, 2, 2, torch.float16, "cuda")
    y.fill_(3.0)

    def call(dtype=L.F16, stride=1, C1=64, C2=64, xp=x.data_ptr(), res=None):
        return L.lib().ey_resnet_tail(dtype, 1, 2, 2, stride, C1, C2, t.data_ptr(), 64, xp, 64, w.data_ptr(), b.data_ptr(), res, 256, y.data_ptr(), 256, L.stream())

    assert call(dtype=L.F32) == -2 and b"resnet_tail" in L.lib().ey_last_error()  # fp32 takes the composed form
    assert call(C2=96) == -2 and call(C1=48) == -2 and call(stride=3) == -2
    assert call(C1=0) == -2  # an identity block needs its residual and takes no second source
    assert call(res=y.data_ptr()) == -2  # a projection block takes none
    torch.cuda.synchronize()
    assert bool((y == 3.0).all())
    # the module: a width outside the kernel's list, and fp32, take the composed form even when the fused one is asked for
    for c1, c2, dt in ((64, 32, torch.float16), (64, 64, torch.float32)):
        blk = M.ResNetBlock(c1, c2, 1).cuda().to(dt).eval()
        blk.tail_fused = True
        xx, _ = _nhwc(rs.pool_input("refuse", (1, c1, 3, 3)), dt)
        _, labels = _traced(lambda: blk(xx))
        assert "resnet_tail_kernel" not in labels and len(labels) == 4, labels


def test_block_forward_is_its_parts():
    """ResNetBlock.forward = cv1, cv2, then the tail above: equal bit for bit to the launches made by hand; the fused and the composed form
    of a block agree to the rounding of the shortcut map."""
    from edge_yolo_amd.nn import modules as M
    for c1, c2, s in ((64, 64, 2), (64, 64, 1), (256, 64, 1)):
        blk = M.ResNetBlock(c1, c2, s).cuda().half().eval()
        proj = isinstance(blk.shortcut, torch.nn.Sequential)
        x, _ = _nhwc(rs.pool_input(f"blk{s}", (2, c1, 7, 6)), torch.float16)
        blk.tail_fused = True
        y, labels = _traced(lambda: blk(x))
        assert len(labels) == 3 and labels[-1] == "resnet_tail_kernel", labels
        want, _ = _tail(blk, blk.cv2(blk.cv1(x)), x)
        assert torch.equal(y, want) and bool((y >= 0).all())
        blk.tail_fused = False
        y2, labels2 = _traced(lambda: blk(x))
        assert len(labels2) == (4 if proj else 3) and float((y2.float() - y.float()).abs().max()) < 2e-2


# ------------------------------------------------------------------------------------------------------------------ ey_classify_pool, wide
@pytest.mark.parametrize("half", [True, False], ids=["f16", "f32"])
@pytest.mark.parametrize("case", rs.WIDE_POOL_CASES, ids=[c[0] for c in rs.WIDE_POOL_CASES])
def test_classify_pool_wide(case, half):
    from edge_yolo_amd import _lib as L
    from edge_yolo_amd.nn import _ops
    tag, B, C1, H, W, Cout = case
    dt = torch.float16 if half else torch.float32
    x, w, b = cls_synth.pool_case(tag, B, C1, H, W, Cout, False, half)
    xv, _ = _nhwc(x, dt)
    got = _ops.classify_pool(xv, torch.tensor(w).to(dt).cuda(), torch.tensor(b).cuda(), L.ACT_SILU)
    assert got.dtype == torch.float32 and tuple(got.shape) == (B, Cout)
    got = got.cpu().numpy().astype(np.float64)
    mean, A, Y = f64c.pool64(x, w, b, True)
    bnd = f64c.pool_bound(A, Y, C1 + 1, H * W)
    err = np.abs(got - mean)
    print(f"{tag} [{'f16' if half else 'f32'}]: max err {float(err.max()):.3e} max err/bound {float((err / bnd).max()):.3f}")
    assert np.isfinite(got).all() and not (err > bnd).any(), f"{tag}: {int((err > bnd).sum())} values beyond the bound"


def test_classify_pool_still_refuses_beyond_its_limit():
    from edge_yolo_amd import _lib as L
    x = L.empty_nhwc(1, 4104, 1, 1, torch.float16, "cuda")
    w = torch.zeros((16, 4104), dtype=torch.float16, device="cuda")
    b = torch.zeros(16, device="cuda")
    out = torch.full((1, 16), 3.0, device="cuda")
    assert L.lib().ey_classify_pool(L.F16, 1, 1, 4104, 16, L.ACT_NONE, x.data_ptr(), 4104, w.data_ptr(), b.data_ptr(), out.data_ptr(), L.stream()) == -2
    torch.cuda.synchronize()
    assert bool((out == 3.0).all())
