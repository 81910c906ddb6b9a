"""-m gpu: SCDown's pointwise 1x1 + SiLU and the depthwise 3x3 stride-2 conv behind it as one kernel (ey_scdown; reference block.py:1174-1206):
bit-identical to the two launches (ey_conv2d + ey_dwconv_s2) on channel windows of wider buffers, within the fp64 bound of the fused
chain (the helper and bound of tests/test_gpu_pw3.py), refused -- with nothing launched -- outside its gate, and taken by yolov10n three
times per forward."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import synthdata as synth  # noqa: E402
import v10_synth as vs  # noqa: E402
from gpu_util import load_synth, to_dev  # noqa: E402
from gpu_util import _traced, tuned  # noqa: E402
import fp64_ref as R  # noqa: E402

SENTINEL = -77.0


def _mod(c1, c2, k=3, dtype=torch.float16):
    from edge_yolo_amd.nn import modules as M
    m = M.SCDown(c1, c2, k, 2)
    load_synth(m, f"scd{c1}_{c2}")
    return to_dev(m, dtype)


def _windows(b, h, w, c1, c2, dtype=torch.float16, x_off=8):
    """x: a channel slice at a non-zero offset of a wider NHWC buffer; y: an interior slot of a wider buffer filled with a sentinel."""
    from edge_yolo_amd import _lib as L
    xbuf = L.empty_nhwc(b, c1 + 16, h, w, dtype, "cuda")
    xbuf.copy_((synth.synth_images(b, h, w, seed=h + w, c=c1 + 16) - 0.5).to(dtype))
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    ybuf = L.empty_nhwc(b, c2 + 16, ho, wo, dtype, "cuda")
    ybuf.fill_(SENTINEL)
    return xbuf[:, x_off:x_off + c1], ybuf, ybuf[:, 8:8 + c2]


def _composed(m, x, out=None):
    from edge_yolo_amd.nn import _ops
    from edge_yolo_amd import _lib as L
    return _ops.dwconv_s2(m.cv2, m.cv1(x), m.cv2.folded, m.cv2.conv.kernel_size[0], L.ACT_NONE, out=out)


@pytest.mark.parametrize("b,h,w,c1,c2", vs.SCDOWN_SHAPES, ids=str)
def test_scdown_bitwise_and_fp64(b, h, w, c1, c2):
    from edge_yolo_amd.nn import _ops
    m = _mod(c1, c2)
    x, ybuf, out = _windows(b, h, w, c1, c2)
    got, ker = _traced(lambda: _ops.scdown(m.cv1, m.cv2, x, out=out))
    assert got is out and ker == ["scdown_kernel"], ker
    assert bool((ybuf[:, :8] == SENTINEL).all()) and bool((ybuf[:, 8 + c2:] == SENTINEL).all())  # the neighbouring slots are untouched
    _, ybuf2, out2 = _windows(b, h, w, c1, c2)
    with tuned(scdown=0):
        two, ker2 = _traced(lambda: m(x, out=out2))
    assert len(ker2) == 2 and "scdown_kernel" not in ker2, ker2
    assert torch.equal(got, two), f"max |diff| {float((got.float() - two.float()).abs().max())}"
    assert torch.equal(ybuf, ybuf2)
    via_module, ker3 = _traced(lambda: m(x))  # the module takes the fused kernel by itself
    assert ker3 == ["scdown_kernel"] and torch.equal(via_module, two)
    # fp64 at every shape: the C2-channel map between the two convs is kept as f16 in LDS
    (w1, b1), (w2, b2) = m.cv1.folded(), m.cv2.folded()
    R.check_chain(f"scdown {b}x{h}x{w} {c1}->{c2}", ker[0], got, [x], [R.stage(w1.half(), b1, 1, 1, 0, R.ACT_SILU), R.stage(w2.half(), b2, 3, 2, 1, R.ACT_NONE, dw=True)])


def test_refusals_launch_nothing_and_the_module_composes():
    from edge_yolo_amd.nn import _ops
    cases = []
    m32 = _mod(16, 64, dtype=torch.float32)  # f32 input
    cases.append(("f32", m32, _windows(1, 6, 8, 16, 64, torch.float32)[0]))
    cases.append(("k=5", _mod(16, 64, k=5), _windows(1, 6, 8, 16, 64)[0]))  # an unsupported k
    cases.append(("C2=32", _mod(16, 32), _windows(2, 9, 13, 16, 32)[0]))  # a channel count outside the gate
    cases.append(("misaligned", _mod(16, 64), _windows(1, 6, 8, 16, 64, x_off=4)[0]))  # a view that starts 8 bytes into a 16-byte unit
    for what, m, x in cases:
        got, ker = _traced(lambda: _ops.scdown(m.cv1, m.cv2, x))
        assert got is None and ker == [], (what, ker)
        y, ker = _traced(lambda: m(x))
        assert len(ker) == 2 and "scdown_kernel" not in ker, (what, ker)
        assert torch.equal(y, _composed(m, x)), what
    # the C ABI itself refuses before anything is launched: called directly with k = 5, with f32 and with an odd pixel stride
    from edge_yolo_amd import _lib as L
    m = _mod(16, 64)
    x, _, out = _windows(1, 6, 8, 16, 64)
    w1, b1 = _ops._conv_pack(m.cv1, x, 16, 1)[:2]
    _composed(m, x)
    w2, b2 = m.cv2._cache[_ops._dev_key(x, "dw2")]

    def call(dtype=L.dtype_code(torch.float16), k=3, xcs=L.cstride(x), c2=64):
        return L.lib().ey_scdown(dtype, 1, 6, 8, 16, c2, k, x.data_ptr(), xcs, w1.data_ptr(), b1.data_ptr(), L.ACT_SILU, w2.data_ptr(), b2.data_ptr(), L.ACT_NONE,
                                 out.data_ptr(), L.cstride(out), L.stream())

    assert call() == 0
    for kw in (dict(k=5), dict(k=7), dict(dtype=L.dtype_code(torch.float32)), dict(xcs=L.cstride(x) + 4), dict(c2=32)):
        with pytest.raises(NotImplementedError):
            L.check(call(**kw), "ey_scdown")
    with tuned(scdown=0):
        with pytest.raises(NotImplementedError):
            L.check(call(), "ey_scdown")
    torch.cuda.synchronize()


def test_fused_kernel_is_capturable_and_deterministic():
    from edge_yolo_amd.nn import _ops
    m = _mod(64, 128)
    x, _, out = _windows(2, 40, 24, 64, 128)
    want = _ops.scdown(m.cv1, m.cv2, x).clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            _ops.scdown(m.cv1, m.cv2, x, out=out)
    torch.cuda.current_stream().wait_stream(s)
    for _ in range(2):
        out.fill_(SENTINEL)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want)


def test_yolov10n_takes_the_fused_kernel_three_times():
    import edge_yolo_amd
    tag = "yolov10n_64x96"
    y = edge_yolo_amd.YOLO(vs.MODEL_CASES[tag][0])
    y.model.load_state_dict(vs.model_weights(tag, y.model.state_dict()))
    model = y.model.to("cuda").fuse().half().eval()
    x = vs.model_images(tag).to("cuda", torch.float16)
    (pred, _), ker = _traced(lambda: model(x))
    assert ker.count("scdown_kernel") == 3 and "conv_direct_kernel" not in ker, ker
    with tuned(scdown=0):
        (pred2, _), ker2 = _traced(lambda: model(x))
    assert ker2.count("scdown_kernel") == 0 and len(ker2) == len(ker) + 3
    assert sum(k.startswith("dwconv_s2_kernel") for k in ker2) == 3
    assert torch.equal(pred, pred2)
