"""The helpers every wrapper of nn/_ops.py goes through, on CPU tensors (no launch is made): the NHWC output check `_out`, the dense buffer checks
`_dense` / `_dense_out`, the workspace, offsets and ctypes-array helpers of the post-processing ops, the alignment predicate `_aligned16`, the
optional-pointer helpers and the table behind ey_conv_last_variant."""
import pytest
import torch

import edge_yolo_amd  # noqa: F401
from edge_yolo_amd import _lib as L
from edge_yolo_amd.nn import _ops

CPU = torch.device("cpu")


def _nhwc(B, C, H, W, dtype=torch.float16):
    return L.empty_nhwc(B, C, H, W, dtype, CPU)


def test_out_allocates_an_nhwc_tensor():
    y = _ops._out("op: out=", None, (2, 8, 3, 5), torch.float16, CPU)
    assert tuple(y.shape) == (2, 8, 3, 5) and y.dtype == torch.float16 and L.is_nhwc_view(y) and L.cstride(y) == 8


def test_out_hands_back_a_matching_view_and_slot():
    y = _nhwc(1, 8, 4, 4)
    assert _ops._out("op: out=", y, (1, 8, 4, 4), torch.float16, CPU) is y
    wide = _nhwc(1, 24, 4, 4)
    slot = wide[:, 8:16]
    assert _ops._out("op: out=", slot, (1, 8, 4, 4), torch.float16, CPU, slot=True) is slot


@pytest.mark.parametrize("bad, why", [
    (lambda: _nhwc(1, 8, 4, 5), "spatial shape"),
    (lambda: _nhwc(1, 16, 4, 4), "channels"),
    (lambda: _nhwc(1, 8, 4, 4, torch.float32), "dtype"),
    (lambda: torch.empty((1, 8, 4, 4), dtype=torch.float16), "NCHW-contiguous"),
    (lambda: torch.empty((8, 4, 4), dtype=torch.float16), "3 dimensions"),
])
def test_out_error_names_wanted_and_given(bad, why):
    t = bad()
    with pytest.raises(ValueError) as e:
        _ops._out("some_op: out=", t, (1, 8, 4, 4), torch.float16, CPU)
    msg = str(e.value)
    assert "some_op: out=" in msg and "NHWC view" in msg, why
    assert str((1, 8, 4, 4)) in msg and str(tuple(t.shape)) in msg, why  # both shapes
    assert "torch.float16" in msg and str(t.dtype) in msg and msg.count("torch.float") == 2, why  # both dtypes


def test_out_slot_requires_sixteen_byte_windows_of_eight_channels():
    wide = _nhwc(1, 24, 4, 4)
    with pytest.raises(ValueError, match="multiples of 8"):  # window starting at element 4: 8 bytes into a pixel
        _ops._out("op: out=", wide[:, 4:12], (1, 8, 4, 4), torch.float16, CPU, slot=True)
    with pytest.raises(ValueError, match="multiples of 8"):  # 4 channels
        _ops._out("op: out=", wide[:, 8:12], (1, 4, 4, 4), torch.float16, CPU, slot=True)
    with pytest.raises(ValueError, match="multiples of 8"):  # pixel stride of 12 elements = 24 bytes
        _ops._out("op: out=", _nhwc(1, 12, 4, 4)[:, :8], (1, 8, 4, 4), torch.float16, CPU, slot=True)
    assert _ops._out("op: out=", wide[:, 4:12], (1, 8, 4, 4), torch.float16, CPU) is not None  # a plain output may sit anywhere


I32 = torch.int32


def test_dense_hands_back_a_matching_tensor():
    t = torch.zeros((3, 2), dtype=I32)
    assert _ops._dense(t, "op: rows", I32, (3, 2), CPU) is t
    assert _ops._dense(t, "op: rows", (torch.uint8, I32), (3, 2), CPU) is t  # one of a set of dtypes
    assert _ops._dense(t, "op: rows", I32, (_ops._AtLeast(3), 2), CPU) is t  # "at least n rows" takes n ...
    more = torch.zeros((4, 2), dtype=I32)
    assert _ops._dense(more, "op: rows", I32, (_ops._AtLeast(3), 2), CPU) is more  # ... and n + 1
    assert _ops._dense(more, "op: rows", I32, (_ops._ANY, 2), CPU) is more
    empty = torch.zeros((0, 2), dtype=I32)
    assert _ops._dense(empty, "op: rows", I32, (_ops._ANY, 2), CPU) is empty
    assert _ops._dense(t, "op: rows", I32, (3, 2), None) is t  # wherever it lives
    with pytest.raises(ValueError, match="op: rows .* on cuda:0, got torch.int32 \\(3, 2\\) on cpu"):
        _ops._dense(t, "op: rows", I32, (3, 2), torch.device("cuda:0"))  # (only the device is compared: nothing touches it)


def test_dense_out_allocates_fills_and_hands_back():
    y = _ops._dense_out("op: out=", None, torch.float32, (2, 3, 4), CPU)
    assert tuple(y.shape) == (2, 3, 4) and y.dtype == torch.float32 and y.is_contiguous() and y.device == CPU
    for fill in (-1, 0):
        y = _ops._dense_out("op: out=", None, I32, (2, 5), CPU, fill=fill)
        assert tuple(y.shape) == (2, 5) and y.dtype == I32 and bool((y == fill).all())
    y = _ops._dense_out("op: out=", None, torch.uint8, (_ops._AtLeast(7),), CPU)  # a lower bound allocates exactly the bound
    assert tuple(y.shape) == (7,) and y.dtype == torch.uint8
    mine = torch.full((2, 6), 9, dtype=I32)
    assert _ops._dense_out("op: out=", mine, I32, (2, _ops._AtLeast(5)), CPU, fill=-1) is mine and bool((mine == 9).all())  # a caller's tensor is not filled
    with pytest.raises(ValueError, match="op: out="):
        _ops._dense_out("op: out=", mine, I32, (2, 7), CPU)


@pytest.mark.parametrize("bad, why", [
    (lambda: torch.zeros((3, 2), dtype=torch.int64), "dtype"),
    (lambda: torch.zeros((3, 4), dtype=I32), "trailing extent"),
    (lambda: torch.zeros((2, 2), dtype=I32), "too few rows"),
    (lambda: torch.zeros((3, 2, 1), dtype=I32), "rank"),
    (lambda: torch.zeros((3, 4), dtype=I32)[:, ::2], "non-contiguous slice"),
    (lambda: [[0, 0]] * 3, "not a tensor"),
])
def test_dense_error_names_wanted_and_given(bad, why):
    t = bad()
    with pytest.raises(ValueError) as e:
        _ops._dense(t, "some_op: rows", I32, (_ops._AtLeast(3), 2), CPU)
    msg = str(e.value)
    assert "some_op: rows" in msg and "contiguous int32" in msg and "(>=3, 2)" in msg, why  # the op, the argument, what is wanted
    if torch.is_tensor(t):
        assert f"got {t.dtype} {tuple(t.shape)}" in msg, why  # what was given
        assert ("not contiguous" in msg) == (not t.is_contiguous()), why
    else:
        assert "got list" in msg, why


def test_workspace_allocates_and_checks():
    ws = _ops._workspace("op", None, 0, CPU)
    assert ws.dtype == torch.uint8 and ws.numel() >= 16 and ws.is_contiguous()
    assert _ops._workspace("op", None, 100, CPU).numel() == 100
    buf = torch.zeros(64 + 16, dtype=torch.uint8)
    lead = -buf.data_ptr() % 16
    exact = buf[lead:lead + 64]  # 64 bytes on a 16-byte boundary
    assert exact.data_ptr() % 16 == 0 and _ops._workspace("op", exact, 64, CPU) is exact
    for bad, why in ((exact[:63], "one byte too few"), (exact.view(torch.int8), "not uint8"), (buf[lead:lead + 64].view(torch.int32), "not uint8"),
                     (buf[lead::2], "strided"), (exact.view(8, 8), "not flat"), (list(range(64)), "not a tensor")):
        with pytest.raises(ValueError, match="op: workspace"):
            _ops._workspace("op", bad, 64 if why == "one byte too few" else 8, CPU)
    misaligned = buf[lead + 1:lead + 1 + 64]
    with pytest.raises(ValueError, match="16-byte"):
        _ops._workspace("op", misaligned, 64, CPU, align=16)
    assert _ops._workspace("op", misaligned, 64, CPU, align=1) is misaligned


def test_pair_offsets_packs_and_honours_out_off():
    pred_off, gt_off, out_off, sizes, end = _ops._pair_offsets("op", [0, 2, 2, 5], (0, 1, 3, 3))  # image 1 has no predictions, image 2 no ground truth
    assert (pred_off, gt_off) == ([0, 2, 2, 5], [0, 1, 3, 3]) and sizes == [2, 0, 0]
    assert out_off == [0, 2, 2] and end == 2
    assert _ops._pair_offsets("op", [0, 2, 4], [0, 1, 4])[2:] == ([0, 2], [2, 6], 8)
    assert _ops._pair_offsets("op", [0, 2, 4], [0, 1, 4], out_off=[7, 0])[2:] == ([7, 0], [2, 6], 9)  # explicit offsets, in any order
    assert _ops._pair_offsets("op", [0, 2, 2], [0, 1, 4], out_off=[3, -5])[2:] == ([3, -5], [2, 0], 5)  # an image without a matrix: its offset is ignored
    assert _ops._pair_offsets("op", [0], [0])[2:] == ([], [], 0)  # B == 0


@pytest.mark.parametrize("args", [
    ([0, 2, 4], [0, 1]),  # lists of different length
    ([1, 2], [0, 1]),  # a first entry other than 0
    ([0, 2], [1, 2]),
    ([], [0]),
    ([0, 2, 4], [0, 1, 4], [0, -1]),  # a negative offset of an image that has a matrix
    ([0, 2, 4], [0, 1, 4], [0]),  # len(out_off) != B
])
def test_pair_offsets_refusals(args):
    with pytest.raises(ValueError, match="some_op: "):
        _ops._pair_offsets("some_op", *args)


def test_ctypes_arrays_are_never_empty():
    import ctypes
    for make, ctype in ((_ops._ia, ctypes.c_int), (_ops._la, ctypes.c_long), (_ops._fa, ctypes.c_float), (_ops._pa, ctypes.c_void_p)):
        a = make([])
        assert len(a) == 1 and a._type_ is ctype and not a[0]
        assert len(make(iter([]))) == 1  # (a generator too)
    assert list(_ops._ia(v for v in (3, -1))) == [3, -1] and list(_ops._la([2 ** 40])) == [2 ** 40] and list(_ops._fa([0.5, 2.0])) == [0.5, 2.0]
    t = torch.zeros(4)
    p = _ops._pa([t, None, t[1:]])
    assert len(p) == 3 and p[0] == t.data_ptr() and p[1] is None and p[2] == t.data_ptr() + 4  # None -> NULL


def test_nms_out_triple():
    rows, count, index = _ops._nms_out(2, 5, 7, CPU)
    assert (tuple(rows.shape), rows.dtype) == ((2, 5, 7), torch.float32) and (tuple(count.shape), count.dtype) == ((2,), I32)
    assert (tuple(index.shape), index.dtype) == ((2, 5), I32)


def test_aligned16_on_offsets_and_strides():
    wide = _nhwc(2, 24, 3, 3)
    assert wide.data_ptr() % 16 == 0
    assert _ops._aligned16(wide) and _ops._aligned16(wide[:, 8:16]) and _ops._aligned16(wide[:, 16:])
    assert not _ops._aligned16(wide[:, 4:12])  # offset of 4 f16 elements = 8 bytes
    assert not _ops._aligned16(wide[:, 1:9]) and not _ops._aligned16(wide[:, 3:11])  # odd offsets
    assert not _ops._aligned16(wide[:, :12]) and _ops._aligned16(wide[:, :12], channels=False)  # 12 channels: only the count fails
    odd = _nhwc(1, 20, 3, 3)  # pixel stride 20 elements = 40 bytes
    assert not _ops._aligned16(odd[:, :8]) and not _ops._aligned16(odd[:, :8], channels=False)
    assert _ops._aligned16(odd[:, :8], channels=False, width=8) and _ops._aligned16(wide[:, 4:12], channels=False, width=8)
    assert not _ops._aligned16(wide[:, 2:10], channels=False, width=8)  # 4 bytes in
    f32 = _nhwc(1, 12, 3, 3, torch.float32)  # 48-byte pixels: element size counts
    assert _ops._aligned16(f32[:, 4:12]) and not _ops._aligned16(f32[:, 2:10])
    seven = _nhwc(1, 7, 3, 3)  # odd stride
    assert not _ops._aligned16(seven, channels=False) and not _ops._aligned16(seven, channels=False, width=8)


def test_optional_pointers():
    t = _nhwc(1, 16, 2, 2)[:, 8:]
    assert _ops._p(None) is None and _ops._p(t) == t.data_ptr()
    assert _ops._pcs(None) == (None, 0) and _ops._pcs(t) == (t.data_ptr(), 16)


# one code of each range of ey_conv_last_variant -> the kernel name tests/test_gpu_conv_exact.py expects for it (case id behind each row)
VARIANTS = [
    (13081, "f16", "conv_igemm_kernel<f16,8,1>"),  # igemm_mt1
    (13082, "f32", "conv_igemm_kernel<f32,8,2>"),  # igemm_mt2
    (12511, "f16", "conv_ws_kernel<f16,5,1,1>"),  # ws_k1_mt1
    (12223, "f32", "conv_ws_kernel<f32,2,2,3>"),  # ws_k3_mt2_s2
    (11051, "f16", "conv3_halo_kernel<f16,5,1>"),  # halo_s1
    (10048, "f16", "conv_small_kernel<f16,4,8>"),  # small_nt4
    (9040, "f16", "conv3p_kernel<4>"),  # c3p_64
    (8441, "f16", "conv3s_kernel<4,4,1>"),  # c3s_s1_mt4
    (8122, "f16", "conv3s_kernel<1,2,2>"),  # c3s_s2_nt1
    (7022, "f16", "conv3r_kernel<2,2>"),  # c3r_s2
    (6041, "f32", "conv3_tile_kernel<f32,4,1>"),  # tile_s1_nt4
    (5083, "f16", "conv_pwr_kernel<f16,8,3>"),  # pwr_nt8_two
    (4050, "f16", "conv_pw_kernel<f16,5>"),  # pw_nt5 (reference variant)
    (3162, "f16", "conv_pwn_kernel<f16,16,2>"),  # pwn_ks16_ntw2
    (3000, "f32", "conv_pwn_kernel<f32,0,0>"),  # the lowest code of the lowest range still has a name
]


@pytest.mark.parametrize("code, tn, name", VARIANTS)
def test_conv_variant_table(code, tn, name):
    assert _ops._conv_variant(code, tn) == name


def test_conv_variant_table_is_sorted_and_refuses_lower_codes():
    floors = [f for f, _ in _ops._CONV_VARIANTS]
    assert floors == sorted(floors, reverse=True) and len(set(floors)) == len(floors)
    for code in (2999, 0, -1):
        with pytest.raises(AssertionError, match="without reporting its kernel"):
            _ops._conv_variant(code, "f16")
