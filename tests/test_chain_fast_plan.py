"""ey_block_fast_plan (csrc/block.hip) is a pure host function of a compiled block program: which pointwise chains the
register-weight executor takes and which keep block_tile_kernel.  No GPU: the stages carry made-up (aligned) addresses."""
import ctypes

import pytest

from edge_yolo_amd import _lib as L

W_PTR, B_PTR = 0x10000, 0x20000  # weights / bias: only their alignment is looked at
T0 = 0x1000000                    # chain-internal tensors (absolute pointers), 1 MiB apart


def _stage(cin, cout, src, y, res=None, addz=None, H=20, W=20, act=L.ACT_SILU, k=1, bias=True):
    """src / res / addz / y: (ext index or -1, address or byte offset, pixel stride); src may be a list of two"""
    st = L.BlockStage()
    st.op = L.BLK_CONV
    st.H, st.W, st.Ho, st.Wo = H, W, H, W
    st.k, st.stride, st.act, st.ngroup, st.out_scale = k, 1, act, 1, 1.0
    srcs = src if isinstance(src, list) else [src]
    cins = cin if isinstance(cin, list) else [cin]
    st.nsrc = len(srcs)
    for j, ((e, a, cs), c) in enumerate(zip(srcs, cins)):
        st.src[j], st.src_ext[j], st.src_cs[j], st.src_C[j], st.src_img[j] = a, e, cs, c, H * W * cs
    st.w, st.bias = W_PTR, (B_PTR if bias else None)
    st.Cout = cout
    st.y, st.y_ext, st.y_cs, st.y_img = y[1], y[0], y[2], H * W * y[2]
    if res is not None:
        st.has_res, st.res, st.res_ext, st.res_cs, st.res_img = 1, res[1], res[0], res[2], H * W * res[2]
    if addz is not None:
        st.has_addz, st.addz, st.addz_ext, st.addz_cs, st.addz_img, st.addz_H, st.addz_W = 1, addz[1], addz[0], addz[2], 100 * addz[2], 10, 10
    return st


def _plan(stages):
    n = len(stages)
    arr = (L.BlockStage * n)(*stages)
    out = (L.BlockStage * n)()
    L.check(L.lib().ey_block_compile(arr, n, ctypes.addressof(out), ctypes.sizeof(out)), "ey_block_compile")
    plan = ctypes.create_string_buffer(L.lib().ey_block_fast_plan_bytes())
    return bool(L.lib().ey_block_tileable(out, n)), bool(L.lib().ey_block_fast_plan(out, n, plan, len(plan))), plan


def _tail(c, **kw):
    """C2PSA's proj(+b) -> ffn -> ffn(+x1, over b) -> cv2: ext 0 = y, ext 1 = t = [a | b], ext 2 = out"""
    x1, f = (-1, T0, c), (-1, T0 + (1 << 20), 2 * c)
    b = (1, 2 * c, 2 * c)
    return [_stage(c, c, (0, 0, c), x1, res=b, act=L.ACT_NONE, bias=False, **kw), _stage(c, 2 * c, x1, f, **kw),
            _stage(2 * c, c, f, b, res=x1, act=L.ACT_NONE, **kw), _stage(2 * c, 2 * c, (1, 0, 2 * c), (2, 0, 2 * c), **kw)]


def _head(c, **kw):
    """cv1 -> qkv: ext 0 = x, ext 1 = t, ext 2 = qkv"""
    return [_stage(2 * c, 2 * c, (0, 0, 2 * c), (1, 0, 2 * c), **kw), _stage(c, 3 * c, (1, 2 * c, 2 * c), (2, 0, 3 * c), act=L.ACT_NONE, **kw)]


@pytest.mark.parametrize("name,stages,tileable,fast", [
    ("tail c128", _tail(128), True, True),
    ("head c128", _head(128), True, True),
    ("tail c64", _tail(64), True, True),
    ("head c64", _head(64), True, True),
    ("tail c128 on a 5x7 map", _tail(128, H=5, W=7), True, True),
    ("tail c256: LDS budget / no instantiated fragment list", _tail(256), True, False),
    ("head c256", _head(256), True, False),
    ("tail c32: 32-channel convs are no instantiated list", _tail(32), True, False),
    ("a lone conv is no instantiated list", [_stage(128, 128, (0, 0, 128), (1, 0, 128))], True, False),
    ("addz stage", [_stage(256, 256, (0, 0, 256), (1, 0, 256), addz=(3, 0, 256)), _stage(128, 384, (1, 256, 256), (2, 0, 384))], True, False),
    ("source channels not a multiple of 32", [_stage([200, 56], 256, [(0, 0, 200), (3, 0, 56)], (1, 0, 256)), _stage(128, 384, (1, 256, 256), (2, 0, 384))], True, False),
    ("two sources of 128", [_stage([128, 128], 256, [(0, 0, 128), (3, 0, 128)], (1, 0, 256)), _stage(128, 384, (1, 256, 256), (2, 0, 384))], True, True),
    ("in place over the stage's own source", [_stage(256, 256, (0, 0, 256), (0, 0, 256)), _stage(128, 384, (0, 256, 256), (2, 0, 384))], True, False),
    ("3x3 stage: not a pointwise chain at all", [_stage(256, 256, (0, 0, 256), (1, 0, 256), k=3), _stage(128, 384, (1, 256, 256), (2, 0, 384))], False, False),
])
def test_fast_plan_accepts_and_refuses(name, stages, tileable, fast):
    got_tileable, got_fast, _ = _plan(stages)
    assert (got_tileable, got_fast) == (tileable, fast), name


def test_fast_plan_small_buffer_and_tunable():
    n = 2
    arr = (L.BlockStage * n)(*_head(128))
    out = (L.BlockStage * n)()
    L.check(L.lib().ey_block_compile(arr, n, ctypes.addressof(out), ctypes.sizeof(out)), "ey_block_compile")
    small = ctypes.create_string_buffer(16)
    assert L.lib().ey_block_fast_plan(out, n, small, len(small)) == 0
    assert L.lib().ey_tune_get(b"chain_fast") == 1
    L.check(L.lib().ey_tune_set(b"chain_fast", 0), "ey_tune_set")
    try:
        assert L.lib().ey_tune_get(b"chain_fast") == 0
    finally:
        L.check(L.lib().ey_tune_set(b"chain_fast", 1), "ey_tune_set")
