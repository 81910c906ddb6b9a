"""-m gpu: ey_maxpool2d (nn.MaxPool2d(2, 1 | 2) behind an explicit nn.ZeroPad2d, and the zero-padded copy k = 1) against torch on the CPU:
max_pool2d(F.pad(x, pad), k, s) of the same values.  A maximum of finite values is exact in any format, so the outputs must be BIT-IDENTICAL
(inputs are finite and hold no negative zero).  The padded cells are zeros that take part in the maximum: on an all-negative map the border
outputs are 0.  Input and output are channel slots of wider NHWC buffers; what lies outside the output slot must stay untouched."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from gpu_util import _traced  # noqa: E402

DT = [torch.float16, torch.float32]
# (name, k, s, (left, right, top, bottom), H, W, all-negative input)
CASES = [
    ("k2s2_2x2", 2, 2, (0, 0, 0, 0), 2, 2, False),
    ("k2s2_5x7", 2, 2, (0, 0, 0, 0), 5, 7, False),   # an odd last row and column are dropped
    ("k2s2_8x8", 2, 2, (0, 0, 0, 0), 8, 8, False),
    ("k2s1_pad_1x1", 2, 1, (0, 1, 0, 1), 1, 1, False),  # max(x, 0)
    ("k2s1_pad_3x5", 2, 1, (0, 1, 0, 1), 3, 5, False),
    ("k2s1_pad_4x4_negative", 2, 1, (0, 1, 0, 1), 4, 4, True),
    ("k2s1_3x5", 2, 1, (0, 0, 0, 0), 3, 5, False),
    ("k2s2_pad_all_5x7", 2, 2, (1, 2, 2, 1), 5, 7, True),
    ("k1_pad_3x5", 1, 1, (0, 1, 0, 1), 3, 5, False),
    ("k1_pad_all_4x4", 1, 1, (2, 1, 1, 3), 4, 4, True),
    ("k2s2_41x67", 2, 2, (0, 0, 0, 0), 41, 67, False),  # more than one workgroup
]
B = 2


def _input(name, c, H, W, negative, dtype):
    gen = torch.Generator().manual_seed(sum(map(ord, name)) + c)
    x = torch.randn((B, c, H, W), generator=gen)
    if negative:
        x = -x.abs() - 0.125
    x = x.to(dtype)
    x[x == 0] = 1.0  # no zero of either sign in the data: the only zeros are the padding
    return x


@pytest.mark.parametrize("dtype", DT, ids=["f16", "f32"])
@pytest.mark.parametrize("c", [8, 24])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_bit_identical_to_torch(case, c, dtype):
    from edge_yolo_amd import _lib as L
    from edge_yolo_amd.nn import _ops as ops
    name, k, s, pad, H, W, negative = case
    x = _input(name, c, H, W, negative, dtype)
    want = F.max_pool2d(F.pad(x.float(), pad), k, s).to(dtype)
    if name == "k2s1_pad_1x1":
        assert torch.equal(want, x.float().clamp_min(0).to(dtype))
    if negative and k == 2:
        assert bool((want[:, :, -1, :] == 0).all()) and bool((want[:, :, :, -1] == 0).all())  # the zero padding wins on the border
    xin = L.empty_nhwc(B, c + 16, H, W, dtype, "cuda")
    xin.fill_(99.0)  # (larger than any datum: a read outside the slot would show)
    xin[:, 8:8 + c] = x.cuda()
    Ho, Wo = want.shape[2:]
    buf = L.empty_nhwc(B, c + 24, Ho, Wo, dtype, "cuda")
    buf.fill_(7.0)
    out = buf[:, 16:16 + c]
    got, labels = _traced(lambda: ops.maxpool2d(xin[:, 8:8 + c], k, s, pad, out=out))
    assert labels == ["maxpool_kernel" if k == 2 else "zeropad_kernel"], labels
    assert got.data_ptr() == out.data_ptr() and tuple(got.shape) == tuple(want.shape)
    assert torch.equal(got.cpu(), want), f"{name}: {int((got.cpu() != want).sum())} of {want.numel()} elements differ"
    assert bool((buf[:, :16] == 7.0).all()) and bool((buf[:, 16 + c:] == 7.0).all()), "the kernel wrote outside its channel slot"
    fresh = ops.maxpool2d(xin[:, 8:8 + c], k, s, pad)  # and without out=: a buffer of its own
    assert torch.equal(fresh.cpu(), want)


def test_modules_pair_is_one_launch_and_equals_two():
    """ZeroPad2d((0, 1, 0, 1)) + MaxPool2d(2, 1, 0): the lazy pad hands the pool its padding (one launch); not lazy it is a padded copy and a
    pool (two launches).  Both equal torch."""
    from edge_yolo_amd.nn.modules import MaxPool2d, ZeroPad2d
    x = _input("pair", 16, 6, 5, True, torch.float16)
    want = F.max_pool2d(F.pad(x.float(), (0, 1, 0, 1)), 2, 1).half()
    zp, mp = ZeroPad2d((0, 1, 0, 1)), MaxPool2d(2, 1, 0)
    two, labels = _traced(lambda: mp(zp(x.cuda())))
    assert labels == ["zeropad_kernel", "maxpool_kernel"] and torch.equal(two.cpu(), want)
    zp.lazy = True
    one, labels = _traced(lambda: mp(zp(x.cuda())))
    assert labels == ["maxpool_kernel"] and torch.equal(one.cpu(), want)


def test_refusals():
    from edge_yolo_amd import _lib as L
    from edge_yolo_amd.nn import _ops as ops
    x = L.empty_nhwc(1, 8, 6, 6, torch.float16, "cuda")
    x.zero_()
    for k, s in ((3, 2), (2, 3), (1, 2)):
        with pytest.raises(NotImplementedError):
            ops.maxpool2d(x, k, s)
    y = L.empty_nhwc(1, 8, 2, 2, torch.float16, "cuda")
    assert L.lib().ey_maxpool2d(L.F16, 1, 6, 6, 8, 3, 2, 0, 0, 0, 0, x.data_ptr(), 8, y.data_ptr(), 8, L.stream()) == -2  # EY_EUNSUPPORTED
    with pytest.raises(NotImplementedError):
        ops.maxpool2d(L.empty_nhwc(1, 12, 4, 4, torch.float16, "cuda"), 2, 2)  # C % 8
