"""-m gpu: ey_hypergraph_conv against an fp64 restatement of AdaHGConv (tests/fp64_hypergraph_ref.py) for 1-6400 tokens and every
(D, E) of the yolov13 scales, on channel windows of NaN-filled buffers; a one-hot probe that must be bit-exact; run-to-run determinism;
refusals.  Also ey_dwconv_s2 (bit-exact on dyadic data), DSConv(s=2) and ey_avgpool2 (bit-exact against torch's CPU AvgPool2d)."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from fp64_hypergraph_ref import hypergraph_fp64  # noqa: E402

# (D, E, heads): the C3AH widths of yolov13 n / s / l / x and a D that is not a multiple of 32
SHAPES = [(64, 4, 4), (128, 8, 8), (256, 8, 16), (384, 12, 24), (48, 3, 3)]
# error bars, relative to max |y|: fp32 is exact fp32 arithmetic in a different order than fp64 (a few ulps of the largest terms);
# f16 stores y and the node_proj operand A.He' in f16 (2^-11 relative each), accumulates in fp32
BAR = {torch.float32: 2e-5, torch.float16: 4e-3}


@pytest.fixture(scope="module")
def L():
    from edge_yolo_amd import _lib
    return _lib


def _module(D, E, heads, seed, context="both"):
    from edge_yolo_amd.nn.modules import AdaHGConv
    torch.manual_seed(seed)
    m = AdaHGConv(D, E, heads, context=context)
    with torch.no_grad():  # prototypes of the size nn.init gives, logits of order 1-10: softmaxes neither flat nor one-hot
        m.edge_generator.prototype_base.normal_(0, 1.0)
        for lin in (m.edge_generator.context_net, m.edge_generator.pre_head_proj, m.edge_proj[0], m.node_proj[0]):
            lin.weight.normal_(0, 1 / math.sqrt(lin.in_features))
            lin.bias.normal_(0, 0.1)
    return m.eval()


def _weights(m):
    g = m.edge_generator
    return (g.prototype_base, g.context_net.weight, g.context_net.bias, g.pre_head_proj.weight, g.pre_head_proj.bias, m.edge_proj[0].weight,
            m.edge_proj[0].bias, m.node_proj[0].weight, m.node_proj[0].bias)


def _windows(B, H, W, D, dtype, pad=8):
    """x, y: channel windows [pad, pad + D) of NaN-filled NHWC buffers with D + 2 pad channels."""
    bx = torch.full((B, H, W, D + 2 * pad), float("nan"), dtype=dtype, device="cuda")
    by = torch.full_like(bx, float("nan"))
    return bx, by, bx.permute(0, 3, 1, 2)[:, pad:pad + D], by.permute(0, 3, 1, 2)[:, pad:pad + D]


def _run(m, x, out):
    from edge_yolo_amd.nn import _ops
    return _ops.hypergraph_conv(m, x, out=out)


# N = 6400 (1280^2) at D = 64, 256 and 384 only
CASES = [(s, hw) for s in SHAPES for hw in [(1, 1), (1, 7), (5, 7), (3, 43), (40, 40), (80, 80)] if hw != (80, 80) or s[0] in (64, 256, 384)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("shape,hw", CASES)
def test_hypergraph_vs_fp64(L, dtype, shape, hw):
    D, E, heads = shape
    B, (H, W), pad = 2, hw, 8
    m = _module(D, E, heads, seed=D * 31 + E).to("cuda").to(dtype)
    bx, by, x, y = _windows(B, H, W, D, dtype, pad)
    g = torch.Generator().manual_seed(H * 1000 + W)
    xv = torch.randn(B, H * W, D, generator=g) * torch.tensor([1.0, 2.0]).view(2, 1, 1)  # two different images
    x.copy_(xv.view(B, H, W, D).permute(0, 3, 1, 2).to(dtype))
    _run(m, x, y)
    torch.cuda.synchronize()
    got = y.permute(0, 2, 3, 1).reshape(B, H * W, D).double().cpu()
    want = hypergraph_fp64(x.permute(0, 2, 3, 1).reshape(B, H * W, D), _weights(m), heads)
    assert torch.isnan(by[..., :pad]).all() and torch.isnan(by[..., pad + D:]).all(), "wrote outside the y window"
    assert torch.isfinite(got).all()
    err = float((got - want).abs().max()) / float(want.abs().max())
    assert err <= BAR[dtype], f"{dtype} D{D} E{E} {H}x{W}: err/max|y| = {err:.3g} > {BAR[dtype]}"


@pytest.mark.parametrize("context", ["mean", "max"])
def test_hypergraph_context_modes(L, context):
    m = _module(64, 4, 4, seed=7, context=context).to("cuda")
    x = torch.randn(2, 64, 9, 11, device="cuda").to(memory_format=torch.channels_last)
    y = _run(m, x, None)
    want = hypergraph_fp64(x.permute(0, 2, 3, 1).reshape(2, 99, 64), _weights(m), 4, context)
    got = y.permute(0, 2, 3, 1).reshape(2, 99, 64).double().cpu()
    assert float((got - want).abs().max()) / float(want.abs().max()) <= BAR[torch.float32]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("N", [77, 300])
def test_hypergraph_one_hot_exact(L, dtype, N):
    """Edge e's logit at token t_e is ~200 above every other token's: its softmax column is exactly one-hot in fp32 (exp(-200) = 0), so
    He_e = X[t_e].  With identity edge / node projections and zero biases, every other token's output is exactly its input (A row 0 ->
    GELU(0) = 0), and token t_e's is X[t_e] + GELU(GELU(X[t_e])) with X[t_e] = 400 on channel e and 0 elsewhere: 800 and 0, exact."""
    from edge_yolo_amd.nn.modules import AdaHGConv
    D, E, heads = 64, 4, 4
    m = AdaHGConv(D, E, heads)
    with torch.no_grad():
        g = m.edge_generator
        g.prototype_base.zero_()
        g.prototype_base[torch.arange(E), torch.arange(E)] = 8.0
        g.context_net.weight.zero_(), g.context_net.bias.zero_()
        for lin in (g.pre_head_proj, m.edge_proj[0], m.node_proj[0]):
            lin.weight.copy_(torch.eye(D)), lin.bias.zero_()
    m = m.to("cuda").to(dtype)
    gen = torch.Generator().manual_seed(N)
    x = (torch.randint(-8, 9, (2, N, D), generator=gen).float() / 8)  # |x| <= 1: logits x/2 <= 0.5
    picks = [[3, N // 2, N - 1, 130 % N], [0, 65 % N, 129 % N, N - 2]]
    for b in range(2):
        for e, t in enumerate(picks[b]):
            x[b, t] = 0
            x[b, t, e] = 400.0
    xd = x.to("cuda", dtype).permute(0, 2, 1).unsqueeze(2)  # (B, D, 1, N) NHWC
    y = _run(m, xd, None).squeeze(2).permute(0, 2, 1).float().cpu()
    want = x.clone()
    for b in range(2):
        for e, t in enumerate(picks[b]):
            want[b, t, e] = 800.0
    assert torch.equal(y, want.to(dtype).float()), float((y - want).abs().max())


def test_hypergraph_deterministic(L):
    m = _module(128, 8, 8, seed=3).to("cuda").half()
    x = torch.randn(4, 128, 40, 40, device="cuda").half().to(memory_format=torch.channels_last)
    y1 = _run(m, x, None).clone()
    y2 = _run(m, x, None)
    torch.cuda.synchronize()
    assert torch.equal(y1, y2)


def test_hypergraph_refusals(L):
    from edge_yolo_amd.nn import _ops
    m = _module(64, 4, 4, seed=1).to("cuda")
    buf = L.empty_nhwc(1, 96, 4, 4, torch.float32, "cuda")
    with pytest.raises(L.HipLibraryError, match="overlap"):
        _ops.hypergraph_conv(m, buf[:, :64], out=buf[:, 32:96])
    _ops.hypergraph_conv(m, buf[:, :64], out=L.empty_nhwc(1, 64, 4, 4, torch.float32, "cuda"))  # disjoint: fine
    big = _module(64, 17, 4, seed=1).to("cuda")
    with pytest.raises(L.HipLibraryError, match="E=17"):
        _ops.hypergraph_conv(big, torch.zeros(1, 64, 4, 4, device="cuda").to(memory_format=torch.channels_last))
    wide = _module(400, 4, 25, seed=1).to("cuda")
    with pytest.raises(L.HipLibraryError, match="D=400"):
        _ops.hypergraph_conv(wide, torch.zeros(1, 400, 2, 2, device="cuda").to(memory_format=torch.channels_last))


# ----------------------------------------------------------------------------------------------- stride-2 depthwise, avg-pool
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("C,k,hw", [(32, 3, (10, 12)), (24, 3, (9, 13)), (64, 5, (7, 7)), (16, 7, (15, 8))])
def test_dwconv_s2_exact(L, dtype, C, k, hw):
    """Dyadic weights and inputs: every tap sum is exact in fp32 and representable in f16, so the kernel equals fp64 bit for bit."""
    from edge_yolo_amd.nn import _ops
    from edge_yolo_amd.nn.modules import Conv
    gen = torch.Generator().manual_seed(C * 7 + k)
    w = torch.randint(-4, 5, (C, 1, k, k), generator=gen).float() / 16
    x = torch.randint(-8, 9, (2, C, *hw), generator=gen).float() / 8
    want = torch.nn.functional.conv2d(x.double(), w.double(), None, 2, k // 2, 1, C)
    holder = Conv(C, C, k, 2, g=C)  # a _Packed cache for the packed weights
    got = _ops.dwconv_s2(holder, x.to("cuda", dtype).to(memory_format=torch.channels_last), lambda: (w, None), k, L.ACT_NONE)
    assert torch.equal(got.double().cpu(), want.to(dtype).double())


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_dsconv_s2_module(L, dtype):
    from edge_yolo_amd.nn.modules.conv import DSConv
    torch.manual_seed(0)
    m = DSConv(32, 48, 3, 2).eval()
    with torch.no_grad():
        m.bn.running_mean.normal_(0, 0.1), m.bn.running_var.uniform_(0.5, 1.5)
    x = torch.randn(2, 32, 11, 9)
    bn = m.bn
    t = torch.nn.functional.conv2d(torch.nn.functional.conv2d(x.double(), m.dw.weight.double(), None, 2, 1, 1, 32), m.pw.weight.double())
    t = (t - bn.running_mean.double().view(1, -1, 1, 1)) / torch.sqrt(bn.running_var.double().view(1, -1, 1, 1) + bn.eps) * bn.weight.double().view(1, -1, 1, 1) \
        + bn.bias.double().view(1, -1, 1, 1)
    want = torch.nn.functional.silu(t)
    with torch.no_grad():
        got = m.to("cuda").to(dtype)(x.to("cuda", dtype)).double().cpu()
        want = want.detach()
    assert got.shape == (2, 48, 6, 5)
    tol = 1e-5 if dtype == torch.float32 else 2e-2
    assert float((got - want).abs().max()) <= tol * float(want.abs().max())


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("C,hw", [(32, (10, 12)), (19, (9, 13)), (64, (3, 2))])
def test_avgpool2_exact(L, dtype, C, hw):
    """fp32: bit-exact against torch's CPU AvgPool2d(2) (the same summation order) on random data; f16: dyadic data, exact sums."""
    from edge_yolo_amd.nn import _ops
    gen = torch.Generator().manual_seed(C)
    x = torch.randn(2, C, *hw, generator=gen) if dtype == torch.float32 else torch.randint(-64, 65, (2, C, *hw), generator=gen).float() / 16
    want = torch.nn.functional.avg_pool2d(x, 2)
    buf = L.empty_nhwc(2, C + 16, hw[0] // 2, hw[1] // 2, dtype, "cuda")
    buf.fill_(float("nan"))
    got = _ops.avgpool2(x.to("cuda", dtype).to(memory_format=torch.channels_last), out=buf[:, 8:8 + C])
    assert torch.equal(got.float().cpu(), want.to(dtype).float())
    assert torch.isnan(buf[:, :8]).all() and torch.isnan(buf[:, 8 + C:]).all()
