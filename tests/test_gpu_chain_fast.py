"""-m gpu: the register-weight executor of tiled block programs (csrc/block.hip: block_chain_kernel, tunable chain_fast) against the
executor it replaces (block_tile_kernel) and the one-launch-per-conv form: byte-equal results, the executor each launch took,
views, the fallback for programs it does not take, and replay with other tensors.

The chains are C2PSA_LinearAttention's own ([cv1 -> qkv] and [proj -> ffn -> ffn -> cv2]) written out here with every tensor a
channel slice of a wider buffer: inputs inside NaN, outputs (t included: the tail writes x2 over its second half) inside a sentinel."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import block_cases as BC  # noqa: E402
from gpu_util import _traced, load_synth, to_dev, tuned  # noqa: E402
from test_gpu_block_exact import Run  # noqa: E402

F16 = torch.float16
SENT = 5.0
TAGS = ("C2PSA_LinearAttention.cv1_qkv", "C2PSA_LinearAttention.proj_ffn_cv2")
_MODS = {}


def _module(c1):
    """one module per width, shared by the cases (never modified)"""
    if c1 not in _MODS:
        from edge_yolo_amd.nn import modules as M
        m = M.C2PSA_LinearAttention(c1, c1, 1)
        load_synth(m, "c2psa")
        _MODS[c1] = to_dev(m, F16)
    return _MODS[c1]


def _view(B, ch, H, W, fill, vals=None, pad=24, off=8):
    """(buffer, view): channels [off, off + ch) of a (ch + pad)-channel NHWC buffer filled with `fill`"""
    from edge_yolo_amd import _lib as L
    buf = L.empty_nhwc(B, ch + pad, H, W, F16, "cuda")
    buf.fill_(fill)
    t = buf[:, off:off + ch]
    if vals is not None:
        t.copy_(vals)
    return buf, t


def _outside_untouched(buf, view, fill):
    lo, C = (view.data_ptr() - buf.data_ptr()) // 2, view.shape[1]
    keep = torch.cat([buf[:, :lo], buf[:, lo + C:]], 1)
    return bool(torch.isnan(keep).all()) if fill != fill else bool((keep == fill).all())


def _chains(mh):
    """the two chains in wrapper code, as C2PSA_LinearAttention._forward_chained states them, with caller-supplied outputs"""
    from edge_yolo_amd import _lib as L
    from edge_yolo_amd.nn import _ops
    from edge_yolo_amd.nn.modules.conv import fold_bn
    blk, c = mh.m[0], mh.c
    at = blk.attn
    qkv_w = lambda: fold_bn(at.qkv.weight, at.qkv.bias, None)  # noqa: E731
    proj_w = lambda: (at.proj.weight.detach().float(), at.proj.bias.detach().float() if at.proj.bias is not None else None)  # noqa: E731

    def head(t_out, q_out):
        def fn(x0):
            t = mh.cv1(x0, out=t_out)
            return [t, _ops.conv2d(at, [t[:, c:]], qkv_w, 1, 1, 0, L.ACT_NONE, out=q_out, tag="qkv")]
        return fn

    def tail(o_out):
        def fn(y, t):
            b = t[:, c:]
            x1 = _ops.conv2d(at, [y], proj_w, 1, 1, 0, L.ACT_NONE, res=b, tag="proj")
            blk.ffn[1](blk.ffn[0](x1), out=b, res=x1)
            return [mh.cv2(t, out=o_out)]
        return fn
    return head, tail


def _run_form(mh, x, yv, form, B, H, W):
    """One form ("fast" / "tile" = the chains with chain_fast 1 / 0, "conv" = one launch per conv) on fresh views.
    Returns (t after the head, qkv, x2, o, executors, buffers to check)."""
    from edge_yolo_amd.nn import _block
    c1, c = 2 * mh.c, mh.c
    head, tail = _chains(mh)
    xb, xd = _view(B, c1, H, W, float("nan"), x)
    tb, t = _view(B, c1, H, W, SENT)
    qb, q = _view(B, 3 * c, H, W, SENT)
    yb, y = _view(B, c, H, W, float("nan"), yv, pad=16)
    ob, o = _view(B, c1, H, W, SENT)
    ex = []
    if form == "conv":
        _, labels = _traced(lambda: head(t, q)(xd))
        t_head = t.clone()
        _, l2 = _traced(lambda: tail(o)(y, t))
        assert not any(lab.startswith("block_") for lab in labels + l2), labels + l2
    else:
        with tuned(chain_fast=1 if form == "fast" else 0):
            hc, tc = _block.BlockCache(TAGS[0], tiled=True), _block.BlockCache(TAGS[1], tiled=True)
            got, labels = _traced(lambda: hc.run(head(t, q), [xd], [t, q]))
            assert got is not None and labels == [f"block_tile_kernel<{TAGS[0]}>"], labels
            ex.append(_block.last_executor())
            t_head = t.clone()
            got, labels = _traced(lambda: tc.run(tail(o), [y, t], [o]))
            assert got is not None and labels == [f"block_tile_kernel<{TAGS[1]}>"], labels
            ex.append(_block.last_executor())
    torch.cuda.synchronize()
    bufs = [(xb, xd, float("nan")), (tb, t, SENT), (qb, q, SENT), (yb, y, float("nan")), (ob, o, SENT)]
    return t_head, q, t[:, c:], o, ex, bufs


def _inputs(c1, B, H, W):
    g = BC.gen("chain_fast", c1, B, H, W)
    x = torch.randn((B, c1, H, W), generator=g).half()
    yv = torch.randn((B, c1 // 2, H, W), generator=g).half()
    return x, yv


@pytest.mark.parametrize("B,H,W", [(1, 5, 7), (1, 8, 8), (3, 13, 17), (2, 20, 20)])
@pytest.mark.parametrize("c1", [128, 256])
def test_executors_agree_bit_for_bit(c1, B, H, W):
    """Both chains forced on with chain_fast = 1 and 0, and one launch per conv, on the same data: t, qkv, x2 (read back from
    t[:, c:]) and the output are torch.equal across the three forms; chain_fast = 1 ran block_chain_kernel, chain_fast = 0
    block_tile_kernel; inputs are slices of NaN buffers, outputs slices of sentinel buffers whose other channels stay untouched.
    35 pixels = one partial tile, 64 = exactly one, 221 = 3 x 64 + 29 (ragged last tile, image stride), 400 = the workload's map."""
    mh = _module(c1)
    x, yv = _inputs(c1, B, H, W)
    res = {f: _run_form(mh, x, yv, f, B, H, W) for f in ("fast", "tile", "conv")}
    assert res["fast"][4] == ["fast", "fast"], res["fast"][4]
    assert res["tile"][4] == ["tile", "tile"], res["tile"][4]
    for form, r in res.items():
        for k, g in zip(("t", "qkv", "x2", "o"), r[:4]):
            assert not bool(torch.isnan(g).any()), f"{form} {k}: NaN (read outside a view)"
        for buf, view, fill in r[5]:
            assert _outside_untouched(buf, view, fill), f"{form}: wrote outside a view"
    for k, a, b_, d in zip(("t", "qkv", "x2", "o"), res["fast"][:4], res["tile"][:4], res["conv"][:4]):
        assert torch.equal(a, b_), f"c{c1} b{B} {H}x{W} {k}: register-weight executor differs from block_tile_kernel"
        assert torch.equal(a, d), f"c{c1} b{B} {H}x{W} {k}: register-weight executor differs from the per-conv form"


def test_wide_chain_falls_back_to_tile_kernel():
    """c1 = 512 (c = 256): no plan (LDS budget, fragment list): chain_fast = 1 still runs block_tile_kernel, equal to the per-conv form"""
    mh = _module(512)
    B, H, W = 2, 13, 17
    x, yv = _inputs(512, B, H, W)
    fast = _run_form(mh, x, yv, "fast", B, H, W)
    conv = _run_form(mh, x, yv, "conv", B, H, W)
    assert fast[4] == ["tile", "tile"], fast[4]
    for k, a, d in zip(("t", "qkv", "x2", "o"), fast[:4], conv[:4]):
        assert torch.equal(a, d), f"c512 {k}: chain differs from the per-conv form"


def test_addz_chain_falls_back_to_tile_kernel():
    """a recorded chain with an addz stage is not eligible: old executor, exact result (= the per-conv form, which is exact too)"""
    from edge_yolo_amd.nn import _block
    r = Run(BC.BY_NAME["c_addz_in_chain"])
    ins, ov = r.dev_inputs(), r.out_views()
    got = r.launch(ins, ov)
    assert r.cache.progs[-1].fast_plan is None and _block.last_executor() == "tile"
    r.check(got, ins, ov)
    per_conv, labels = _traced(lambda: r.fn()(*r.dev_inputs()))
    assert all(lab.startswith("conv_") for lab in labels), labels
    assert all(torch.equal(a, b) for a, b in zip(got, per_conv))


def test_recorded_fast_program_serves_other_tensors():
    """One recorded program, run by block_chain_kernel, with other tensors: other data at other addresses into caller-supplied
    outputs while the recording's inputs hold NaN; fresh outputs; inputs at another byte offset of their storage record a second
    program (which is fast as well).  C2PSA's tail at c = 128, 13x17: exact data, bit-identical to fp64."""
    from edge_yolo_amd.nn import _block
    c = BC.BY_NAME["c_tail_inplace_c128"]
    r = Run(c)
    ins0, ov0 = r.dev_inputs(), r.out_views()
    got0 = r.launch(ins0, ov0)
    prog = r.cache.progs[-1]
    assert prog.fast_plan is not None and _block.last_executor() == "fast"
    r.check(got0, ins0, ov0, what=" record")
    in1 = BC.make(c, variant=1)[0]
    ins1, ov1 = r.dev_inputs(in1), r.out_views()
    for t in ins0:
        t.fill_(float("nan"))
    assert prog.matches(ins1) and all(a.data_ptr() != b.data_ptr() for a, b in zip(ins0, ins1))
    got1 = r.launch(ins1, ov1, pass_outs=True)
    assert len(r.cache.progs) == 1 and _block.last_executor() == "fast"
    assert all(g.data_ptr() == ov1[k][1].data_ptr() for g, k in zip(got1, c["outs"]))
    r.check(got1, ins1, ov1, inputs=in1, what=" replay other data")
    in2 = BC.make(c, variant=2)[0]
    ins2 = r.dev_inputs(in2)
    got2 = r.launch(ins2)
    assert _block.last_executor() == "fast" and all(a.data_ptr() != b.data_ptr() for a, b in zip(got1, got2))
    r.check(got2, ins2, None, inputs=in2, what=" replay fresh outs")
    ins3 = r.dev_inputs(in1, shifted=True)
    assert not prog.matches(ins3)
    got3 = r.launch(ins3)
    assert len(r.cache.progs) == 2 and r.cache.progs[-1].fast_plan is not None and _block.last_executor() == "fast"
    r.check(got3, ins3, None, inputs=in1, what=" re-recorded at another offset")
    with tuned(chain_fast=0):  # the same program on the old executor: the tunable decides per launch
        ins4 = r.dev_inputs(in2)
        got4 = r.launch(ins4)
        assert _block.last_executor() == "tile"
        r.check(got4, ins4, None, inputs=in2, what=" chain_fast=0")
