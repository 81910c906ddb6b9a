"""-m gpu: the three classify kernels (csrc/classify.hip) against the float64 restatements of tests/fp64_cls_ref.py.

ey_classify_pool, f16 and fp32: exact cases (integer inputs, weights in multiples of 1/4, no activation, H W a power of two) must equal
float64 bit for bit; SiLU cases on general data obey the per-element bound fp64_cls_ref.pool_bound (built like tests/fp64_ref.bound); one
case reads a channel window of a wider NaN-filled buffer.
ey_classify_linear_softmax: |gpu - float64| <= 4 E + 2 ulp(fp32) for logits and probabilities, E = the reference's own fp32 error on the
case's inputs (tests/golden/cls_ops.npz); the top-k indices equal the reference's; a case with logits near +-80; an all-equal case judged
against the tie rule (lower class index first) only.
ey_classify_transform: |255 gpu - Pillow| <= 1 + 2^-8 grey levels (f16: plus half an f16 ulp at 1.0, in grey levels), and |gpu - float64|
<= 4 E + 2 ulp with E = the error of the same expressions evaluated in fp32.  E and the achieved error are printed per case."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import cls_synth  # noqa: E402
import fp64_cls_ref as f64  # noqa: E402


@pytest.fixture(scope="module")
def cls_ops(golden_dir):
    return np.load(os.path.join(golden_dir, "cls_ops.npz"))


def _nhwc(x, dt, lead=0, extra=0):
    """(B, C, H, W) numpy -> NHWC device view, a channel window [lead, lead + C) of a NaN-filled buffer when lead or extra is set."""
    from edge_yolo_amd import _lib as L
    B, C, H, W = x.shape
    buf = L.empty_nhwc(B, lead + C + extra, H, W, dt, "cuda")
    buf.fill_(float("nan"))
    v = buf[:, lead:lead + C]
    v.copy_(torch.tensor(x).to(dt))
    return v


# ------------------------------------------------------------------------------------------------------------------ ey_classify_pool
def _pool(case, half, lead=0, extra=0):
    from edge_yolo_amd import _lib as L
    from edge_yolo_amd.nn import _ops
    tag, B, C1, H, W, Cout, exact = case
    dt = torch.float16 if half else torch.float32
    x, w, b = cls_synth.pool_case(tag, B, C1, H, W, Cout, exact, half)
    xv = _nhwc(x, dt, lead, extra)
    assert L.cstride(xv) == lead + C1 + extra
    got = _ops.classify_pool(xv, torch.tensor(w).to(dt).cuda(), torch.tensor(b).cuda(), L.ACT_NONE if exact else L.ACT_SILU)
    assert got.dtype == torch.float32 and tuple(got.shape) == (B, Cout)
    got = got.cpu().numpy().astype(np.float64)
    mean, A, Y = f64.pool64(x, w, b, not exact)
    label = f"{tag} [{'f16' if half else 'f32'}]"
    if exact:
        assert np.array_equal(mean.astype(np.float32).astype(np.float64), mean), label  # the case is exact in fp32
        print(f"{label}: exact, max |mean| {float(np.abs(mean).max()):.4g}")
        np.testing.assert_array_equal(got, mean, err_msg=label)
        return
    bnd = f64.pool_bound(A, Y, C1 + 1, H * W)
    err = np.abs(got - mean)
    print(f"{label}: max err {float(err.max()):.3e} max err/bound {float((err / bnd).max()):.3f} max |mean| {float(np.abs(mean).max()):.3g}")
    assert np.isfinite(got).all() and not (err > bnd).any(), f"{label}: {int((err > bnd).sum())} values beyond the bound (worst ratio {float((err / bnd).max()):.3f})"


@pytest.mark.parametrize("half", [True, False], ids=["f16", "f32"])
@pytest.mark.parametrize("case", cls_synth.POOL_CASES, ids=[c[0] for c in cls_synth.POOL_CASES])
def test_classify_pool(case, half):
    _pool(case, half)


@pytest.mark.parametrize("half", [True, False], ids=["f16", "f32"])
def test_classify_pool_channel_window(half):
    """the map is a window of a wider buffer with NaN on both sides: 16-byte aligned for f16 (vector loads), misaligned for fp32 (scalar loads)."""
    _pool(cls_synth.POOL_SLICED, half, lead=8 if half else 3, extra=16)


# ------------------------------------------------------------------------------------------------------------------ linear + softmax + top-k
def _check(tag, got, ref64, E):
    got = np.asarray(got, np.float64)
    err = np.abs(got - ref64)
    print(f"{tag}: E {E:.3e} achieved {float(err.max()):.3e} bound(min) {4 * E:.3e}")
    bad = err > f64.bound(E, ref64)
    assert np.isfinite(got).all() and not bad.any(), f"{tag}: {int(bad.sum())} values beyond 4E + 2ulp (E {E:.3e}, worst {float(err.max()):.3e})"


def _linear(pooled, w, b, half):
    from edge_yolo_amd.nn import _ops
    dt = torch.float16 if half else torch.float32
    out = _ops.classify_linear_softmax(torch.tensor(pooled).cuda(), torch.tensor(w).to(dt).cuda(), torch.tensor(b).cuda())
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


@pytest.mark.parametrize("tag", list(cls_synth.LINEAR_CASES))
def test_linear_softmax(cls_ops, tag):
    B, nc, half, kind = cls_synth.LINEAR_CASES[tag]
    pooled, w, b = cls_synth.linear_case(tag)
    logits, probs, topi, topp = _linear(pooled, w, b, half)
    assert logits.shape == probs.shape == (B, nc) and topi.shape == topp.shape == (B, min(nc, 5)) and topi.dtype == np.int32
    l64, p64 = f64.linear_softmax64(pooled, w, b)
    _check(tag + " logits", logits, l64, float(cls_ops[tag + "_El"]))
    _check(tag + " probs", probs, p64, float(cls_ops[tag + "_Ep"]))
    n = 1 if kind == "big" else min(nc, 5)  # (+-80: one class near 1, the others near 0: only the winner is separable)
    np.testing.assert_array_equal(topi[:, :n], cls_ops[tag + "_top"][:, :n])
    np.testing.assert_array_equal(topi, f64.rank(probs))  # the ranking rule on the kernel's own probabilities, ties included
    np.testing.assert_array_equal(topp, np.take_along_axis(probs, topi.astype(np.int64), 1))
    if kind == "big":
        assert float(np.abs(l64).max()) > 60 and abs(float(probs.sum(1).max()) - 1) < 1e-6


def test_linear_softmax_ties_rank_the_lower_class_first():
    tag, B, nc = cls_synth.LINEAR_TIE
    logits, probs, topi, topp = _linear(np.ones((B, cls_synth.C_), np.float32), np.zeros((nc, cls_synth.C_), np.float32), np.full(nc, 0.5, np.float32), False)
    assert (logits == 0.5).all() and (probs == probs[0, 0]).all() and abs(float(probs[0, 0]) - 1 / nc) < 1e-8
    assert topi.tolist() == [[0, 1, 2, 3, 4]] * B and (topp == probs[0, 0]).all()
    # two groups of equal logits: classes 70..79 lead, in ascending order
    b = np.zeros(nc, np.float32)
    b[70:] = 1.0
    _, probs, topi, _ = _linear(np.ones((B, cls_synth.C_), np.float32), np.zeros((nc, cls_synth.C_), np.float32), b, True)
    assert topi.tolist() == [[70, 71, 72, 73, 74]] * B


def test_linear_softmax_is_capturable_and_repeatable():
    from edge_yolo_amd.nn import _ops
    pooled, w, b = cls_synth.linear_case("ls_nc1000_b33")
    p, w, b = torch.tensor(pooled).cuda(), torch.tensor(w).half().cuda(), torch.tensor(b).cuda()
    eager = [t.clone() for t in _ops.classify_linear_softmax(p, w, b)]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _ops.classify_linear_softmax(p, w, b)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = _ops.classify_linear_softmax(p, w, b)
    g.replay()
    torch.cuda.synchronize()
    for a, c in zip(eager, out):
        assert torch.equal(a, c)


# ------------------------------------------------------------------------------------------------------------------ ey_classify_transform
@pytest.mark.parametrize("half", [True, False], ids=["f16", "f32"])
@pytest.mark.parametrize("case", cls_synth.TRANSFORM_CASES, ids=[c[0] for c in cls_synth.TRANSFORM_CASES])
def test_classify_transform(cls_ops, case, half):
    from edge_yolo_amd.data.augment import ClassifyTransform
    tag, h, w, S = case
    dt = torch.float16 if half else torch.float32
    rgb = cls_synth.transform_image(tag, h, w)
    bgr = np.ascontiguousarray(rgb[..., ::-1])
    got = ClassifyTransform(S).batch([bgr], "cuda", dt)
    assert tuple(got.shape) == (1, 3, S, S) and got.dtype == dt
    got = got[0].float().cpu().numpy().astype(np.float64)
    pil = cls_ops[tag + "_pil"].astype(np.float64).transpose(2, 0, 1)
    ref64 = f64.to_tensor(f64.transform(rgb, S))
    E = float(cls_ops[tag + "_E"])
    half_ulp = 255.0 * 2.0 ** -11 if half else 0.0  # half an f16 ulp at 1.0, in grey levels
    d_pil, err = float(np.abs(255.0 * got - pil).max()), np.abs(got - ref64)
    print(f"{tag} [{'f16' if half else 'f32'}]: max |255 gpu - pillow| {d_pil:.4f} levels, E {E:.3e} achieved {float(err.max()):.3e}")
    assert d_pil <= 1.0 + 2.0 ** -8 + half_ulp, tag
    bnd = f64.bound(E, ref64) + (2.0 ** -11 * np.maximum(ref64, 2.0 ** -14) if half else 0.0)  # f16: one rounding of the stored value
    assert not (err > bnd).any(), f"{tag}: {int((err > bnd).sum())} values beyond 4E + 2ulp (worst {float(err.max()):.3e})"


def test_classify_transform_batch_tensor_equals_per_image_launches():
    from edge_yolo_amd.data.augment import ClassifyTransform
    tag, h, w, S = cls_synth.TRANSFORM_CASES[0]
    a = np.ascontiguousarray(cls_synth.transform_image(tag, h, w)[..., ::-1])
    b = np.ascontiguousarray(a[::-1])
    t = ClassifyTransform(S)
    one = t.batch([a, b], "cuda", torch.float32)
    both = t.batch_tensor(torch.tensor(np.stack([a, b])).cuda(), torch.float32)
    assert torch.equal(one, both)
    keep_bgr = t.batch_tensor(torch.tensor(a[None]).cuda(), torch.float32, swap_rb=False)
    assert torch.equal(keep_bgr[0].flip(0), one[0])
