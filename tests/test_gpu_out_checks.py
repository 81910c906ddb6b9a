"""-m gpu: every wrapper of nn/_ops.py that takes out= checks it before anything is launched.  The post-processing wrappers (dense buffers,
workspace=, tracker state) have their own table at the end of the file.  Each network op runs on the smallest legal input
(B = 1, 8 channels or the op's minimum width, a 4x4 map, f16).  A wrong spatial shape, a wrong dtype and an NCHW-contiguous tensor of the
right logical shape raise ValueError and record no launch; a good channel slot of a wider buffer gives the bits of the freshly allocated
output and leaves its neighbours alone.  The ops that require 16-byte slots refuse a window starting at element 4; the fused ops that fall
back on misaligned outputs (scdown, ghost_conv, dsb_pair) return None there."""
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

F16 = torch.float16
SENTINEL = 1234.0


def _x(c=8, h=4, w=4):
    from edge_yolo_amd import _lib as L
    t = L.empty_nhwc(1, c, h, w, F16, torch.device("cuda:0"))
    t.copy_(torch.randn(1, c, h, w, generator=torch.Generator().manual_seed(c * 100 + h)).mul(0.5))
    return t


def _img(h=8, w=8):
    return torch.rand(1, 3, h, w, generator=torch.Generator().manual_seed(7)).half().cuda()


def _conv(*a, **k):
    from edge_yolo_amd.nn.modules.conv import Conv
    return Conv(*a, **k).eval()


def _holder():
    from edge_yolo_amd.nn.modules.conv import _Packed
    return _Packed()


# ---- one builder per op: returns fn(out) -> the op's output; flags: "slot" (16-byte channel slots required), "none" (None when misaligned)
def _conv2d():
    from edge_yolo_amd import _lib as L
    from edge_yolo_amd.nn import _ops
    m, x = _conv(8, 8, 1), _x()
    return lambda out: _ops.conv2d(m, [x], m.folded, 1, 1, 0, L.ACT_SILU, out=out)


def _conv2d_direct():
    from edge_yolo_amd import _lib as L
    from edge_yolo_amd.nn import _ops
    m, x = _conv(8, 8, 1), _x()
    return lambda out: _ops.conv2d_direct(m, x, m.folded, 1, 1, 0, 1, L.ACT_SILU, out=out)


def _conv_pw_chain():
    from edge_yolo_amd import _lib as L
    from edge_yolo_amd.nn import _ops
    m1, m2, x = _conv(40, 64, 1), _conv(64, 8, 1), _x(40)
    return lambda out: _ops.conv_pw_chain(m1, x, m1.folded, L.ACT_SILU, m2.folded, L.ACT_NONE, out)


def _stem_conv():
    from edge_yolo_amd import _lib as L
    from edge_yolo_amd.nn import _ops
    m, x = _conv(3, 16, 3, 2), _img()
    return lambda out: _ops.stem_conv(m, x, m.folded, L.ACT_SILU, F16, out=out)


def _stem_conv_ks():
    from edge_yolo_amd import _lib as L
    from edge_yolo_amd.nn import _ops
    m, x = _conv(3, 16, 6, 2, 2), _img()
    return lambda out: _ops.stem_conv_ks(m, x, m.folded, 6, 2, 2, L.ACT_SILU, F16, out=out)


def _maxpool2d():
    from edge_yolo_amd.nn import _ops
    x = _x()
    return lambda out: _ops.maxpool2d(x, 2, 2, out=out)


def _maxpool3x3s2():
    from edge_yolo_amd.nn import _ops
    x = _x()
    return lambda out: _ops.maxpool3x3s2(x, out=out)


def _resnet_stem():
    from edge_yolo_amd import _lib as L
    from edge_yolo_amd.nn import _ops
    m, x = _conv(3, 64, 7, 2, 3, act=nn.ReLU()), _img()
    return lambda out: _ops.resnet_stem(m, x, m.folded, L.ACT_RELU, out=out)


def _resnet_tail():
    from edge_yolo_amd.nn import _ops
    g = torch.Generator().manual_seed(3)
    w, b = torch.randn(256, 64, 1, 1, generator=g) * 0.1, torch.randn(256, generator=g) * 0.1
    m, t, x = _holder(), _x(64), _x(256)
    return lambda out: _ops.resnet_tail(m, t, x, lambda: (w, b), 1, True, out=out)


def _pw_conv3s2():
    from edge_yolo_amd.nn import _ops
    from gpu_util import tuned
    cv2, c3, a, b = _conv(16, 64, 1), _conv(64, 64, 3, 2), _x(8), _x(8) * 0.5

    def fn(out):
        with tuned(pw3_min_px=0):  # dispatched from 100000 pixels on: the tuning knob lets a 4x4 map take the kernel, as in tests/test_gpu_pw3.py
            return _ops.pw_conv3s2(cv2, c3, [a, b], out=out)

    return fn


def _scdown():
    from edge_yolo_amd.nn import _ops
    cv1, cv2, x = _conv(8, 64, 1), _conv(64, 64, 3, 2, g=64, act=False), _x()
    return lambda out: _ops.scdown(cv1, cv2, x, out=out)


def _ghost_conv():
    from edge_yolo_amd.nn import _ops
    cv1, cv2, x = _conv(8, 8, 1), _conv(8, 8, 5, 1, None, 8), _x()
    return lambda out: _ops.ghost_conv(cv1, cv2, x, out=out)


def _stem_pair():
    from edge_yolo_amd.nn import _ops
    m0, m1, x = _conv(3, 16, 3, 2), _conv(16, 32, 3, 2), _img()
    return lambda out: _ops.stem_pair(m0, m1, x, out=out)


def _dwconv():
    from edge_yolo_amd import _lib as L
    from edge_yolo_amd.nn import _ops
    m, x = _conv(8, 8, 3, 1, g=8), _x()
    return lambda out: _ops.dwconv(m, x, m.folded, 3, L.ACT_SILU, out=out)


def _dwconv_s2():
    from edge_yolo_amd import _lib as L
    from edge_yolo_amd.nn import _ops
    m, x = _conv(8, 8, 3, 2, g=8), _x()
    return lambda out: _ops.dwconv_s2(m, x, m.folded, 3, L.ACT_NONE, out=out)


def _dsb_pair():
    from edge_yolo_amd.nn import _ops
    from edge_yolo_amd.nn.modules.conv import DSConv
    cv1, cv2, x = DSConv(32, 32, 3).eval(), DSConv(32, 32, 5).eval(), _x(32)
    return lambda out: _ops.dsb_pair(cv1, cv2, x, True, out=out)


def _dsconv():
    from edge_yolo_amd import _lib as L
    from edge_yolo_amd.nn import _ops
    from edge_yolo_amd.nn.modules.conv import DSConv
    m, x = DSConv(8, 8, 3).eval(), _x()
    return lambda out: _ops.dsconv(m, x, m._dw_folded, m._pw_folded, 3, L.ACT_SILU, out=out)


def _dwt_haar():
    from edge_yolo_amd.nn import _ops
    x = _x()
    return lambda out: _ops.dwt_haar(x, out=out)


def _dwt():
    from edge_yolo_amd.nn import _ops
    x, taps = _x(), torch.rand(4, 4, 4, generator=torch.Generator().manual_seed(5)).half().float().cuda()
    return lambda out: _ops.dwt(x, taps, 4, out=out)


def _linear_attention():
    from edge_yolo_amd.nn import _ops
    qkv = _x(96)
    return lambda out: _ops.linear_attention(qkv, 2, out=out)


def _softmax_attention():
    from edge_yolo_amd.nn import _ops
    qkv = _x(128)
    return lambda out: _ops.softmax_attention(qkv, 1, 32, 64, 32 ** -0.5, out=out)


def _area_attention():
    from edge_yolo_amd.nn import _ops
    q, k, v = _x(32), _x(32, 4, 4) * 0.5, _x(32) * 2
    return lambda out: _ops.area_attention(q, k, v, 1, 2, 32 ** -0.5, out=out)


def _flash_attention():
    from edge_yolo_amd.nn import _ops
    q, k, v = _x(32), _x(32) * 0.5, _x(32) * 2
    return lambda out: _ops.flash_attention(q, k, v, 1, 32 ** -0.5, out=out)


def _scale_add_channels():
    from edge_yolo_amd.nn import _ops
    x, t, gamma = _x(), _x() * 0.25, torch.linspace(0.5, 1.5, 8).cuda()
    return lambda out: _ops.scale_add_channels(x, gamma, t, out=out)


def _avgpool2():
    from edge_yolo_amd.nn import _ops
    x = _x()
    return lambda out: _ops.avgpool2(x, out=out)


def _adown_a():
    from edge_yolo_amd.nn import _ops
    x = _x(16)
    return lambda out: _ops.adown_pool(x, 8, a=out)[0]


def _adown_m():
    from edge_yolo_amd.nn import _ops
    x = _x(16)
    return lambda out: _ops.adown_pool(x, 8, m=out)[1]


def _cbfuse():
    from edge_yolo_amd.nn import _ops
    a, b = _x(8, 2, 2), _x()
    return lambda out: _ops.cbfuse([a, b], out=out)


def _dysample():
    from edge_yolo_amd.nn import _ops
    from edge_yolo_amd.nn.modules.dysample import DySample
    m, x = DySample(16, groups=2).eval(), _x(16)
    return lambda out: _ops.dysample(m, x, out=out)


def _max_sigmoid_attn():
    from edge_yolo_amd.nn import _ops
    e, p = _x(32), _x(32) * 0.5
    guide = torch.randn(1, 3, 32, generator=torch.Generator().manual_seed(9)).half().cuda()
    bias = torch.zeros(1, device="cuda")
    return lambda out: _ops.max_sigmoid_attn(e, p, guide, bias, None, 1, out=out)


def _deconv2x2():
    from edge_yolo_amd.nn.modules.classic import ConvTranspose2d
    m, x = ConvTranspose2d(8, 8, 2, 2, 0).eval(), _x()
    return lambda out: m(x, out=out)


def _hypergraph_conv():
    from edge_yolo_amd.nn import _ops
    from edge_yolo_amd.nn.modules.block import AdaHGConv
    m, x = AdaHGConv(32, 8, 4).eval(), _x(32)
    return lambda out: _ops.hypergraph_conv(m, x, out=out)


def _dwconv_gate():
    from edge_yolo_amd import _lib as L
    from edge_yolo_amd.nn import _ops
    m, conv, x = _holder(), nn.Conv2d(8, 8, 3, 1, 1, groups=8), _x()
    return lambda out: _ops.dwconv_gate(m, x, conv, L.DWG_PLAIN, out=out)


def _sigmoid_gate():
    from edge_yolo_amd.nn import _ops
    x, g = _x(), _x() * 2
    return lambda out: _ops.sigmoid_gate(x, g, out=out)


def _gelu():
    from edge_yolo_amd.nn import _ops
    x = _x()
    return lambda out: _ops.gelu(x, out=out)


def _cmlp():
    from edge_yolo_amd.nn import _ops
    m, fc1, fc2, x = _holder(), nn.Conv2d(8, 16, 3, 1, 1, groups=8), nn.Conv2d(16, 8, 3, 1, 1, groups=8), _x()
    return lambda out: _ops.cmlp(m, x, fc1, fc2, out=out)


def _layernorm_channels():
    from edge_yolo_amd.nn import _ops
    m, ln, x = _holder(), nn.LayerNorm(8), _x()
    return lambda out: _ops.layernorm_channels(m, x, ln, out=out)


def _layernorm_pool():
    from edge_yolo_amd.nn import _ops
    m, ln, x = _holder(), nn.LayerNorm(8), _x()
    return lambda out: _ops.layernorm_channels(m, x, ln, pool=True, out=out)


def _unpool2_layernorm():
    from edge_yolo_amd.nn import _ops
    m, ln, t = _holder(), nn.LayerNorm(8), _x(8, 2, 2)
    up = nn.ConvTranspose2d(8, 8, 2, 2, groups=8, bias=False)
    return lambda out: _ops.unpool2_layernorm(m, t, up, ln, 4, 4, out=out)


OPS = {
    "conv2d": (_conv2d, ""), "conv2d_direct": (_conv2d_direct, ""), "conv_pw_chain": (_conv_pw_chain, ""), "stem_conv": (_stem_conv, ""),
    "stem_conv_ks": (_stem_conv_ks, ""), "maxpool2d": (_maxpool2d, "slot"), "maxpool3x3s2": (_maxpool3x3s2, "slot"), "resnet_stem": (_resnet_stem, "slot"),
    "resnet_tail": (_resnet_tail, "slot"), "pw_conv3s2": (_pw_conv3s2, ""), "scdown": (_scdown, "none"), "ghost_conv": (_ghost_conv, "none"),
    "stem_pair": (_stem_pair, ""), "dwconv": (_dwconv, ""), "dwconv_s2": (_dwconv_s2, ""), "dsb_pair": (_dsb_pair, "none"), "dsconv": (_dsconv, ""),
    "dwt_haar": (_dwt_haar, ""), "dwt": (_dwt, ""), "linear_attention": (_linear_attention, ""), "softmax_attention": (_softmax_attention, ""),
    "area_attention": (_area_attention, ""), "flash_attention": (_flash_attention, ""), "scale_add_channels": (_scale_add_channels, ""),
    "avgpool2": (_avgpool2, ""), "adown_pool_a": (_adown_a, "slot"), "adown_pool_m": (_adown_m, "slot"), "cbfuse": (_cbfuse, "slot"),
    "dysample": (_dysample, ""), "max_sigmoid_attn": (_max_sigmoid_attn, ""), "deconv2x2": (_deconv2x2, ""), "hypergraph_conv": (_hypergraph_conv, ""),
    "dwconv_gate": (_dwconv_gate, ""), "sigmoid_gate": (_sigmoid_gate, ""), "gelu": (_gelu, ""), "cmlp": (_cmlp, ""),
    "layernorm_channels": (_layernorm_channels, ""), "layernorm_channels_pool": (_layernorm_pool, ""), "unpool2_layernorm": (_unpool2_layernorm, ""),
}


def _refused(fn, out):
    """fn(out) must raise ValueError before it launches anything."""
    from edge_yolo_amd import profiling
    with profiling.trace() as t:
        with pytest.raises(ValueError, match="NHWC view|multiples of 8"):
            fn(out)
    assert t.records == [], [r[0] for r in t.records]


@pytest.mark.parametrize("name", sorted(OPS))
def test_out_is_checked(name):
    from edge_yolo_amd import _lib as L
    from edge_yolo_amd import profiling
    build, flag = OPS[name]
    with torch.no_grad():
        fn = build()
        y0 = fn(None)
        assert y0 is not None, "the smallest legal input must take the kernel under test"
        torch.cuda.synchronize()
        B, C, H, W = y0.shape
        dev = y0.device
        assert y0.dtype == F16 and L.is_nhwc_view(y0)

        _refused(fn, L.empty_nhwc(B, C, H + 1, W, F16, dev))  # wrong spatial shape
        _refused(fn, L.empty_nhwc(B, C, H, W, torch.float32, dev))  # wrong dtype
        nchw = torch.empty((B, C, H, W), dtype=F16, device=dev)  # the right logical shape in NCHW memory
        assert not L.is_nhwc_view(nchw)
        _refused(fn, nchw)

        def wide():
            return L.empty_nhwc(B, C + 16, H, W, F16, dev).fill_(SENTINEL)

        if flag:  # a channel window starting 8 bytes into a pixel
            buf = wide()
            with profiling.trace() as t:
                if flag == "slot":
                    with pytest.raises(ValueError, match="multiples of 8"):
                        fn(buf[:, 4:4 + C])
                else:
                    assert fn(buf[:, 4:4 + C]) is None
            assert t.records == []
            torch.cuda.synchronize()
            assert bool((buf == SENTINEL).all())

        buf = wide()
        slot = buf[:, 8:8 + C]
        y1 = fn(slot)
        torch.cuda.synchronize()
        assert y1 is not None and y1.data_ptr() == slot.data_ptr() and tuple(y1.shape) == (B, C, H, W)
        assert torch.equal(y1, y0), "a channel slot must receive the bits of the freshly allocated output"
        assert bool((buf[:, :8] == SENTINEL).all()) and bool((buf[:, 8 + C:] == SENTINEL).all()), "the neighbouring channels were written"


# ---- the post-processing wrappers: dense (non-NHWC) out= buffers, workspace= and one tracker state entry, checked by _dense / _workspace.
# One builder per op -> (call, spec): call(bufs) runs the op on its smallest legal input with the caller's buffers of `bufs` (label -> tensor; a
# label that is missing is left to the wrapper) and returns the outputs as a list; spec: label -> (shape, dtype) of the buffer that is right.
def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _rand(*shape, seed=1):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed)).cuda()


def _bits(n, h, w, seed=2):
    return (torch.rand(n, h, w, generator=torch.Generator().manual_seed(seed)) > 0.4).to(torch.uint8).cuda()


def _post_process_mask():
    from edge_yolo_amd.nn import _ops
    proto, coef = _rand(1, 4, 4, 8).sub(0.5).permute(0, 3, 1, 2), _rand(1, 2, 2, 8, seed=3).sub(0.5).permute(0, 3, 1, 2)
    rows = torch.tensor([[0, 0], [0, 3]], dtype=torch.int32).cuda()
    boxes = torch.tensor([[0.0, 0.0, 8.0, 8.0], [1.0, 2.0, 7.0, 6.0]]).cuda()
    return (lambda b: [_ops.process_mask(proto, [coef], rows, boxes, 2, out=b.get("out"))]), {"out": ((2, 8, 8), torch.uint8)}


def _post_scale_masks():
    from edge_yolo_amd.nn import _ops
    masks = _bits(2, 8, 8)[:, None]
    return (lambda b: [_ops.scale_masks(masks, (12, 10), out=b.get("out"))]), {"out": ((2, 1, 12, 10), torch.float32)}


def _post_kpt_iou():
    from edge_yolo_amd.nn import _ops
    pred, gt = _rand(2, 2, 3).mul(8), _rand(2, 2, 3, seed=4).mul(8)
    gt[:, :, 2] = 1.0
    area, sigma = torch.tensor([30.0, 50.0]).cuda(), torch.tensor([0.05, 0.1]).cuda()
    return (lambda b: [_ops.kpt_iou(pred, [0, 2], gt, [0, 2], area, sigma, out=b.get("out"))[0]]), {"out": ((4,), torch.float32)}


def _post_kpts_decode_rows():
    from edge_yolo_amd.nn import _ops
    levels = [(_x(6), 8.0, 0)]  # K = 2 keypoints of (x, y, visibility) on a 4x4 map
    index, count = torch.tensor([[5, 11]], dtype=torch.int32).cuda(), torch.tensor([2], dtype=torch.int32).cuda()
    return (lambda b: [_ops.kpts_decode_rows(levels, (2, 3), index, count, out=b.get("out"))]), {"out": ((1, 2, 2, 3), torch.float32)}


def _post_classify_pool():
    from edge_yolo_amd import _lib as L
    from edge_yolo_amd.nn import _ops
    x, w, bias = _x(), _rand(16, 8).sub(0.5).half(), _rand(16, seed=5)  # f16 takes Cout in multiples of 16
    return (lambda b: [_ops.classify_pool(x, w, bias, L.ACT_SILU, out=b.get("out"))]), {"out": ((1, 16), torch.float32)}


def _post_classify_transform():
    from edge_yolo_amd.nn import _ops
    images = (_rand(1, 8, 8, 3) * 255).to(torch.uint8)
    return (lambda b: [_ops.classify_transform(images, 4, F16, out=b.get("out"))]), {"out": ((1, 3, 4, 4), F16)}


def _some_or_all(b, spec, labels, make=tuple):
    """None when `b` names none of `labels`, else all of them: the caller's where given, a right one (zeros) elsewhere."""
    if not any(k in b for k in labels):
        return None
    return make((k, b[k] if k in b else torch.zeros(spec[k][0], dtype=spec[k][1], device=_dev())) for k in labels)


def _post_mask_prompt():
    from edge_yolo_amd import _lib as L
    from edge_yolo_amd.nn import _ops
    masks = _bits(2, 8, 8)
    spec = {"full": ((2,), torch.float32), "keep": ((2,), torch.uint8), "inter": ((1, 2), torch.float32), "iou": ((1, 2), torch.float32),
            "best": ((1, 1), torch.int32), "hit": ((1, 2), torch.uint8)}
    outs = list(spec)
    spec["workspace"] = ((int(L.lib().ey_mask_prompt_workspace_bytes(1, 8, 8, 1)),), torch.uint8)  # exactly what the entry point asks for

    def call(b):
        got = _ops.mask_prompt(masks, [0, 2], [(8, 8)], bboxes=[[1, 1, 6, 6]], points=[[3, 4]], labels=[1], out=_some_or_all(b, spec, outs, dict), workspace=b.get("workspace"))
        return [got[k] for k in outs]

    return call, spec


def _post_bytetrack_update():
    import fp64_track_ref as ref
    from edge_yolo_amd import _lib as L
    from edge_yolo_amd.nn import _ops
    rows = torch.zeros((1, 4, 6)).cuda()  # one stream, room for 4 detections, 8 track slots
    rows[0, :2] = torch.tensor([[10.0, 12.0, 30.0, 40.0, 0.9, 0.0], [50.0, 20.0, 80.0, 70.0, 0.8, 1.0]]).cuda()
    count = torch.tensor([2], dtype=torch.int32).cuda()
    spec = {"out_rows": ((1, 4, 8), torch.float32), "ids": ((1, 4), torch.int32), "counts": ((1,), torch.int32), "state_kf": ((1, 8, 72), torch.float64),
            "workspace": ((int(L.lib().ey_bytetrack_workspace_bytes(1, 4, 8)),), torch.uint8)}

    def call(b):
        state = _ops.bytetrack_state(1, 8, _dev())  # a fresh tracker each time: the call advances it
        if "state_kf" in b:
            state["kf"] = b["state_kf"]
        out = _some_or_all(b, spec, ("out_rows", "ids", "counts"), lambda kv: tuple(t for _, t in kv))
        return list(_ops.bytetrack_update(rows, count, state, ref.DEFAULTS, out=out, workspace=b.get("workspace"))) + [state[k] for k in sorted(state)]

    return call, spec


POST_OPS = {"process_mask": _post_process_mask, "scale_masks": _post_scale_masks, "kpt_iou": _post_kpt_iou, "kpts_decode_rows": _post_kpts_decode_rows,
            "classify_pool": _post_classify_pool, "classify_transform": _post_classify_transform, "mask_prompt": _post_mask_prompt,
            "bytetrack_update": _post_bytetrack_update}
OTHER_DTYPE = {torch.float32: torch.int32, torch.int32: torch.float32, torch.uint8: torch.int8, torch.float64: torch.float32, F16: torch.float32}


@pytest.mark.parametrize("name", sorted(POST_OPS))
def test_dense_buffers_are_checked(name):
    from edge_yolo_amd import profiling
    with torch.no_grad():
        call, spec = POST_OPS[name]()
        y0 = [t.clone() for t in call({})]
        torch.cuda.synchronize()
        for label, (shape, dt) in spec.items():
            bad = {"dtype": torch.zeros(shape, dtype=OTHER_DTYPE[dt], device=_dev()),
                   "shape": torch.zeros(shape + (1,), dtype=dt, device=_dev()),  # the same elements under one more axis
                   "too small": torch.zeros((shape[0] - 1,) + shape[1:], dtype=dt, device=_dev())}
            for why, t in bad.items():
                with profiling.trace() as rec:
                    with pytest.raises(ValueError, match=label.replace("state_", "")):
                        call({label: t})
                assert rec.records == [], (label, why, [r[0] for r in rec.records])
        mine = {label: torch.zeros(shape, dtype=dt, device=_dev()) for label, (shape, dt) in spec.items()}
        y1 = call(mine)
        torch.cuda.synchronize()
        for label in spec:
            if not label.startswith(("state", "workspace")):
                assert any(t.data_ptr() == mine[label].data_ptr() for t in y1), f"{label}: the caller's buffer was not the one written"
        assert len(y1) == len(y0)
        for a, b in zip(y0, y1):
            assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)), \
                "the caller's buffers must receive the bits of the call that allocates its own"
