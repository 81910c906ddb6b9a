"""-m gpu: ey_adown_pool and ey_cbfuse bit for bit.

adown_pool.  `a` and `m` equal the numpy restatement of the stated order (fp32 ((x00 + x01) + x10) + x11, times 0.25f, one rounding to the
storage type; the maximum over the rounded values, window positions outside the averaged map skipped) and torch's CPU
avg_pool2d / chunk / max_pool2d, in fp32 and f16.

cbfuse.  The output equals the numpy restatement in list order (fp32 sum from source 0, one rounding).  Against the float64 sum:
  fp32   n - 1 additions in any order:                                         (n - 1) u sum|terms|,        u = 2^-24
  f16    the same fp32 accumulation, then one rounding to f16 of the result:   (n - 1) u sum|terms| + 2^-11 |y| (+ the smallest f16 subnormal step)"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import fp64_v9_ref as f64  # noqa: E402
import v9_synth as vs  # noqa: E402

U = 2.0 ** -24
DTYPES = [(torch.float32, np.float32), (torch.float16, np.float16)]


def _nhwc(a, dtype, pad=0, off=0):
    """numpy (B, C, H, W) -> a cuda NHWC view in `dtype`; pad > 0: a channel slot at offset `off` of a buffer `pad` channels wider, the rest
    filled with a sentinel.  Returns (view, buffer)."""
    from edge_yolo_amd import _lib as L
    B, C, H, W = a.shape
    buf = L.empty_nhwc(B, C + pad, H, W, dtype, "cuda")
    buf.fill_(-77.0)
    v = buf[:, off:off + C]
    v.copy_(torch.tensor(a).to(dtype))
    return v, buf


def _np(t):
    return t.float().cpu().numpy()


@pytest.mark.parametrize("dt,npdt", DTYPES, ids=["f32", "f16"])
@pytest.mark.parametrize("B,C,c_avg,H,W", vs.ADOWN_SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("negative", [False, True], ids=["", "neg"])
def test_adown_pool_exact(B, C, c_avg, H, W, dt, npdt, negative):
    from edge_yolo_amd.nn import _ops as ops
    x = vs.exact_input(f"adown{B}_{C}_{H}_{W}", (B, C, H, W), dt == torch.float16, negative=negative)
    xv, _ = _nhwc(x, dt)
    a, m = ops.adown_pool(xv, c_avg)
    torch.cuda.synchronize()
    wa, wm = f64.adown_pool_stated(x, c_avg, npdt)
    assert tuple(a.shape) == wa.shape and np.array_equal(_np(a), wa.astype(np.float32))
    A = F.avg_pool2d(torch.tensor(x).to(dt), 2, 1, 0, False, True)
    assert np.array_equal(_np(a), A[:, :c_avg].float().numpy())
    if c_avg == C:
        assert m is None and wm is None
        return
    assert tuple(m.shape) == wm.shape == (B, C - c_avg, H // 2, W // 2)
    assert np.array_equal(_np(m), wm.astype(np.float32))
    assert np.array_equal(_np(m), F.max_pool2d(A[:, c_avg:].float(), 3, 2, 1).numpy())
    if negative:
        assert (_np(m) < 0).all() and (_np(a) < 0).all()  # a skipped window position never contributes a zero


@pytest.mark.parametrize("dt,npdt", DTYPES, ids=["f32", "f16"])
def test_adown_pool_channel_slots(dt, npdt):
    """x, a and m as channel slots of wider buffers: the bytes outside the slots stay unchanged."""
    from edge_yolo_amd import _lib as L
    from edge_yolo_amd.nn import _ops as ops
    B, C, c_avg, H, W = 2, 32, 16, 7, 10
    x = vs.exact_input("adown_slots", (B, C, H, W), dt == torch.float16)
    xv, xbuf = _nhwc(x, dt, pad=24, off=8)
    abuf = L.empty_nhwc(B, c_avg + 16, H - 1, W - 1, dt, "cuda").fill_(-55.0)
    mbuf = L.empty_nhwc(B, C - c_avg + 8, H // 2, W // 2, dt, "cuda").fill_(-33.0)
    xb0 = xbuf.clone()
    a, m = ops.adown_pool(xv, c_avg, a=abuf[:, 8:8 + c_avg], m=mbuf[:, 8:])
    torch.cuda.synchronize()
    wa, wm = f64.adown_pool_stated(x, c_avg, npdt)
    assert a.data_ptr() == abuf[:, 8:].data_ptr() and m.data_ptr() == mbuf[:, 8:].data_ptr()
    assert np.array_equal(_np(abuf[:, 8:8 + c_avg]), wa.astype(np.float32)) and np.array_equal(_np(mbuf[:, 8:]), wm.astype(np.float32))
    assert (abuf[:, :8] == -55.0).all() and (abuf[:, 8 + c_avg:] == -55.0).all() and (mbuf[:, :8] == -33.0).all()
    assert torch.equal(xbuf, xb0)


def test_adown_pool_refusals():
    from edge_yolo_amd import _lib as L
    from edge_yolo_amd.nn import _ops as ops
    x = L.empty_nhwc(1, 16, 4, 4, torch.float16, "cuda")
    with pytest.raises(ValueError):
        ops.adown_pool(x[:, 4:12], 8)  # a slot that starts 8 bytes into a pixel
    with pytest.raises(ValueError):
        ops.adown_pool(x, 8, a=L.empty_nhwc(1, 8, 4, 4, torch.float16, "cuda"))  # wrong size
    with pytest.raises(ValueError):
        ops.adown_pool(x, 16, m=L.empty_nhwc(1, 8, 2, 2, torch.float16, "cuda"))
    code = L.lib().ey_adown_pool(L.F16, 1, 4, 4, 16, 0, x.data_ptr(), 16, x.data_ptr(), 16, None, 0, None)
    assert code != 0 and b"c_avg" in L.lib().ey_last_error()
    code = L.lib().ey_adown_pool(L.F16, 1, 4, 4, 16, 8, x.data_ptr(), 16, x.data_ptr(), 16, None, 0, None)
    assert code != 0  # a split without an output for the pooled half


# ---------------------------------------------------------------------------------------------------------------- cbfuse
def _cbfuse_case(tag, B, C, sizes, half):
    return [vs.exact_input(f"{tag}{i}", (B, C, h, w), half) for i, (h, w) in enumerate(sizes)]


def _check_cbfuse(srcs, got, dt, npdt):
    want = f64.cbfuse_stated(srcs, npdt)
    assert got.shape == want.shape and np.array_equal(got, want.astype(np.float32))
    y64, T = f64.cbfuse64(srcs)
    bnd = (len(srcs) - 1) * U * T
    if dt == torch.float16:
        bnd = bnd + 2.0 ** -11 * np.abs(y64) + 2.0 ** -25
    err = np.abs(got.astype(np.float64) - y64)
    print(f"cbfuse n={len(srcs)} {np.dtype(npdt).name}: max err {err.max():.3e}, bound {bnd.max():.3e}")
    assert (err <= bnd).all()


CBFUSE_SIZES = {
    "odd": [(9, 13), (5, 7), (3, 4), (2, 2), (1, 1), (9, 13)],  # not power-of-two ratios; target 9x13 (the last)
    "pow2": [(32, 32), (16, 16), (8, 8), (4, 4), (2, 2), (32, 32)],
}


@pytest.mark.parametrize("dt,npdt", DTYPES, ids=["f32", "f16"])
@pytest.mark.parametrize("n", [1, 2, 6])
@pytest.mark.parametrize("which", list(CBFUSE_SIZES))
def test_cbfuse_exact(which, n, dt, npdt):
    from edge_yolo_amd.nn import _ops as ops
    sizes = CBFUSE_SIZES[which][-n:] if n < 6 else CBFUSE_SIZES[which]
    if n == 2:
        sizes = [CBFUSE_SIZES[which][1], CBFUSE_SIZES[which][-1]]  # one resized source and the target
    srcs = _cbfuse_case(f"cbf_{which}{n}", 2, 16, sizes, dt == torch.float16)
    y = ops.cbfuse([_nhwc(s, dt)[0] for s in srcs])
    torch.cuda.synchronize()
    _check_cbfuse(srcs, _np(y), dt, npdt)
    if n == 1:
        assert np.array_equal(_np(y), srcs[0].astype(npdt).astype(np.float32))  # identity


@pytest.mark.parametrize("dt,npdt", DTYPES, ids=["f32", "f16"])
def test_cbfuse_sources_are_slices_of_cblinear_outputs(dt, npdt):
    """Sources that are channel slices of wider buffers (what CBLinear returns): unequal pixel strides, an output slot; nothing else is written."""
    from edge_yolo_amd import _lib as L
    from edge_yolo_amd.nn import _ops as ops
    B, C = 2, 8
    sizes, pads, offs = [(3, 4), (5, 7), (9, 13)], [24, 56, 0], [16, 8, 0]
    srcs = _cbfuse_case("cbf_slices", B, C, sizes, dt == torch.float16)
    views = [_nhwc(s, dt, pad=p, off=o)[0] for s, p, o in zip(srcs, pads, offs)]
    assert len({L.cstride(v) for v in views}) == 3
    obuf = L.empty_nhwc(B, C + 8, 9, 13, dt, "cuda").fill_(-11.0)
    y = ops.cbfuse(views, out=obuf[:, 8:])
    torch.cuda.synchronize()
    _check_cbfuse(srcs, _np(y), dt, npdt)
    assert (obuf[:, :8] == -11.0).all()
    with pytest.raises(ValueError):
        ops.cbfuse(views + [views[-1][:, :, :, :]] * 4)  # 7 sources
