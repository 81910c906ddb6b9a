"""Convolution modules of the detection path, HIP-backed.

Same constructor signatures, attribute names and state_dict keys as the reference's
ultralytics/nn/modules/conv.py (`Conv` :41-59, `DSConv` :87-104, `DWConv` :124-129, `Concat` :345-355,
`autopad` :32-38), so a reference state_dict loads unchanged.  `nn.Conv2d` / `nn.BatchNorm2d` children are
parameter containers only; they are never called.  forward() packs (BN-folded) weights for the HIP kernels on
first use and launches through the C ABI (`_lib`).  Extra keyword arguments of forward (`out=`, `res=`) let the
composite blocks write straight into concat buffers and fuse residual adds; positional use is drop-in.
"""
import ctypes
import math

import torch
import torch.nn as nn

from .. import _ops as ops
from ... import _lib as L

__all__ = ("Conv", "DWConv", "DSConv", "RepConv", "GhostConv", "Concat", "Upsample", "autopad")


def autopad(k, p=None, d=1):
    """'same' padding (reference conv.py:32-38)."""
    if d > 1:
        k = d * (k - 1) + 1 if isinstance(k, int) else [d * (x - 1) + 1 for x in k]
    if p is None:
        p = k // 2 if isinstance(k, int) else [x // 2 for x in k]
    return p


def _act_code(act):
    if isinstance(act, nn.SiLU):
        return L.ACT_SILU
    if isinstance(act, nn.ReLU):
        return L.ACT_RELU
    if isinstance(act, nn.Sigmoid):
        return L.ACT_SIGMOID
    if isinstance(act, nn.Identity):
        return L.ACT_NONE
    raise NotImplementedError(f"activation {type(act).__name__} has no HIP epilogue (SiLU/ReLU/Sigmoid/Identity do)")


class _Packed(nn.Module):
    """Mixin: per-(dtype, device) cache of packed device weights; dropped whenever parameters move or reload."""

    def __init__(self):
        super().__init__()
        self._cache = {}
        self.register_load_state_dict_post_hook(lambda m, _keys: m._cache.clear())

    def _apply(self, fn, *a, **k):
        self._cache = {}
        return super()._apply(fn, *a, **k)

    def _packed(self, key, build):
        v = self._cache.get(key)
        if v is None:
            with torch.no_grad():
                v = self._cache[key] = build()
        return v


def fold_bn(w, b, bn):
    """fuse_conv_and_bn (reference utils/torch_utils.py:238-265) on fp32 copies: returns (w', b')."""
    w = w.detach().float()
    b = torch.zeros(w.shape[0], device=w.device) if b is None else b.detach().float()
    if bn is None:
        return w, b
    s = bn.weight.detach().float() / torch.sqrt(bn.running_var.detach().float() + bn.eps)
    return w * s.view(-1, 1, 1, 1), s * b + (bn.bias.detach().float() - bn.running_mean.detach().float() * s)


class Conv(_Packed):
    """Conv2d + BatchNorm + activation (reference conv.py:41-59): args (c1, c2, k, s, p, g, d, act)."""

    default_act = nn.SiLU()

    def __init__(self, c1, c2, k=1, s=1, p=None, g=1, d=1, act=True):
        super().__init__()
        self.conv = nn.Conv2d(c1, c2, k, s, autopad(k, p, d), groups=g, dilation=d, bias=False)
        self.bn = nn.BatchNorm2d(c2)
        self.act = self.default_act if act is True else act if isinstance(act, nn.Module) else nn.Identity()

    # -- fuse(): fold BN into the conv parameters like BaseModel.fuse does (tasks.py:214-242)
    def fuse_bn(self):
        if hasattr(self, "bn"):
            w, b = fold_bn(self.conv.weight, self.conv.bias, self.bn)
            dt = self.conv.weight.dtype
            self.conv.weight = nn.Parameter(w.to(dt), requires_grad=False)
            self.conv.bias = nn.Parameter(b.to(dt), requires_grad=False)
            del self.bn
            self._cache = {}

    def folded(self):
        return fold_bn(self.conv.weight, self.conv.bias, getattr(self, "bn", None))

    def forward(self, x, out=None, res=None):
        c = self.conv
        w, b = None, None
        k, s, p, d, g = c.kernel_size[0], c.stride[0], c.padding[0], c.dilation[0], c.groups
        if c.kernel_size[0] != c.kernel_size[1] or c.stride[0] != c.stride[1] or d != 1:
            raise NotImplementedError("non-square kernels / dilation are outside the EdgeLine-YOLO detection path")
        act = _act_code(self.act)
        if (g == 1 and k == 3 and s == 2 and p == 1 and c.in_channels <= 4 and c.out_channels % 16 == 0 and res is None
                and torch.is_tensor(x) and x.dim() == 4 and x.is_contiguous() and not L.is_nhwc_view(x)):
            # network stem: read the planar NCHW image directly, write NHWC
            return ops.stem_conv(self, x, self.folded, act, x.dtype, out=out)
        if (g == 1 and (k, s, p) in ops.STEM_KS and c.in_channels <= 4 and c.out_channels % 16 == 0 and res is None
                and torch.is_tensor(x) and x.dim() == 4 and x.is_contiguous() and not L.is_nhwc_view(x)):
            # the stems of YOLOv5 (6x6 stride 2, pad 2) and YOLOv3 (3x3 stride 1): planar NCHW image in, NHWC out, as above
            return ops.stem_conv_ks(self, x, self.folded, k, s, p, act, x.dtype, out=out)
        if g == 1:
            return ops.conv2d(self, [x], self.folded, k, s, p, act, out=out, res=res)
        if g == c.in_channels == c.out_channels and s == 1 and k in (3, 5, 7) and p == k // 2 and res is None:
            return ops.dwconv(self, x, self.folded, k, act, out=out)
        cg, og = c.in_channels // g, c.out_channels // g
        if res is None and cg % 8 == 0 and og % 8 == 0:
            # grouped conv on the MFMA implicit GEMM: one launch, group i reads input channels [i*cg, (i+1)*cg) with weight set i and
            # writes output channels [i*og, (i+1)*og)
            x = L.as_nhwc(ops.as_tensor(x))
            if ops.igemm_ok([x[:, :cg]], k, s, p):
                B, _, H, W = x.shape
                Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
                if out is None:
                    out = L.empty_nhwc(B, c.out_channels, Ho, Wo, x.dtype, x.device)
                ops.conv2d(self, [x[:, :cg]], self._group_sets, k, s, p, act, out=out[:, :og], ngroup=g, src_gstride=cg, y_gstride=og, w_sets=g,
                           tag="grp")
                return out
        return ops.conv2d_direct(self, x, self.folded, k, s, p, g, act, out=out, res=res)

    def _group_sets(self):
        w, b = self.folded()
        og = w.shape[0] // self.conv.groups
        return [(w[i * og:(i + 1) * og], b[i * og:(i + 1) * og]) for i in range(self.conv.groups)]

    forward_fuse = forward


class DWConv(Conv):
    """Depth-wise convolution (reference conv.py:124-129)."""

    def __init__(self, c1, c2, k=1, s=1, d=1, act=True):
        super().__init__(c1, c2, k, s, g=math.gcd(c1, c2), d=d, act=act)


class GhostConv(nn.Module):
    """Ghost convolution (reference conv.py:180-193): cat(y, cv2(y)) with y = cv1(x), cv1 = Conv(c1, c2 / 2, k, s, g=g), cv2 a depthwise 5x5 Conv
    on y, both with the same activation.  The pointwise form (k = s = g = 1) on f16 is ONE launch (ops.ghost_conv: y stays in LDS, the concat
    is two channel windows of one store pass, and `res=` -- the shortcut of a GhostBottleneck -- is added in the same pass).  Every other form
    -- fp32, the 3x3 stride-2 downsampling layers, a shape the kernel refuses, the tunable ghost = 0 -- writes cv1 straight into the first
    half of the output buffer and runs cv2 from there into the second half on the existing kernels: no cat.  `out=` may be a slot of a concat
    buffer and may be `res` itself."""

    def __init__(self, c1, c2, k=1, s=1, g=1, act=True):
        super().__init__()
        c_ = c2 // 2
        self.cv1 = Conv(c1, c_, k, s, None, g, act=act)
        self.cv2 = Conv(c_, c_, 5, 1, None, c_, act=act)

    def _cv2_folded_f16(self):
        w, b = self.cv2.folded()
        return w.half().float(), b

    def forward(self, x, out=None, res=None):
        c = self.cv1.conv
        c_ = c.out_channels
        if c.kernel_size == (1, 1) and c.stride == (1, 1) and c.groups == 1:
            y = ops.ghost_conv(self.cv1, self.cv2, x, out=out, res=res)
            if y is not None:
                return y
        B, _, H, W = x.shape  # x may be a VirtualCat
        k, s, p = c.kernel_size[0], c.stride[0], c.padding[0]
        Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
        if out is not None and (not L.is_nhwc_view(out) or tuple(out.shape) != (B, 2 * c_, Ho, Wo) or out.dtype != x.dtype):
            raise ValueError(f"GhostConv: out= must be an NHWC view of shape {(B, 2 * c_, Ho, Wo)} {x.dtype}")
        # with a residual the two halves go to a buffer of their own: out= may be res, and cv2 reads cv1's output before anything is added
        t = out if out is not None and res is None else L.empty_nhwc(B, 2 * c_, Ho, Wo, x.dtype, x.device)
        self.cv1(x, out=t[:, :c_])
        if x.dtype == torch.float16 and c_ % 8:
            # a hidden width ey_dwconv does not take (4, 12, 20 ...): the generic direct kernel, with the depthwise weights rounded to f16 as
            # ey_dwconv and ey_ghost_conv hold them -- the same sums in the same order, so the f16 result does not depend on the path
            ops.conv2d_direct(self.cv2, t[:, :c_], self._cv2_folded_f16, 5, 1, 2, c_, _act_code(self.cv2.act), out=t[:, c_:], tag="f16w")
        else:
            self.cv2(t[:, :c_], out=t[:, c_:])
        if res is None:
            return t
        return ops.cbfuse([t, res], out=out)  # fp32 sum of the two maps, one rounding (= an f16 add)


class RepConv(_Packed):
    """RepVGG-style conv of the YOLOv9 RepBottleneck (reference conv.py:196-297): act(conv1 3x3 + conv2 1x1 [+ bn identity]), each branch a
    Conv(act=False).  The three branches are linear in x, so the HIP path always runs ONE 3x3 conv on the reference's
    `get_equivalent_kernel_bias` weights, folded in fp32 when they are packed -- before `fuse_convs()` (from conv1 / conv2 / bn) and after it
    (from the single `conv` it leaves)."""

    default_act = nn.SiLU()

    def __init__(self, c1, c2, k=3, s=1, p=1, g=1, d=1, act=True, bn=False, deploy=False):
        super().__init__()
        assert k == 3 and p == 1
        self.g, self.c1, self.c2 = g, c1, c2
        self.act = self.default_act if act is True else act if isinstance(act, nn.Module) else nn.Identity()
        self.bn = nn.BatchNorm2d(num_features=c1) if bn and c2 == c1 and s == 1 else None
        self.conv1 = Conv(c1, c2, k, s, p=p, g=g, act=False)
        self.conv2 = Conv(c1, c2, 1, s, p=(p - k // 2), g=g, act=False)

    def get_equivalent_kernel_bias(self):
        """3x3 kernel + zero-padded 1x1 kernel + identity kernel, and the sum of their biases, BatchNorms folded, in fp32 (reference :228-269)."""
        k3, b3 = self.conv1.folded()
        k1, b1 = self.conv2.folded()
        k, b = k3 + nn.functional.pad(k1, [1, 1, 1, 1]), b3 + b1
        if getattr(self, "bn", None) is not None:
            cg = self.c1 // self.g
            kid = torch.zeros((self.c1, cg, 3, 3), dtype=torch.float32, device=k.device)
            kid[torch.arange(self.c1), torch.arange(self.c1) % cg, 1, 1] = 1.0
            kid, bid = fold_bn(kid, None, self.bn)
            k, b = k + kid, b + bid
        return k, b

    def folded(self):
        if hasattr(self, "conv"):
            return self.conv.weight.detach().float(), self.conv.bias.detach().float()
        return self.get_equivalent_kernel_bias()

    def fuse_convs(self):
        """Leave a single `conv` with bias and drop conv1, conv2 and bn (reference :271-297)."""
        if hasattr(self, "conv"):
            return
        with torch.no_grad():
            kernel, bias = self.get_equivalent_kernel_bias()
        c, dt = self.conv1.conv, self.conv1.conv.weight.dtype
        self.conv = nn.Conv2d(c.in_channels, c.out_channels, c.kernel_size, c.stride, c.padding, c.dilation, c.groups, bias=True).requires_grad_(False)
        self.conv.weight.data = kernel.to(dt)
        self.conv.bias.data = bias.to(dt)
        for name in ("conv1", "conv2", "nm", "bn", "id_tensor"):
            if hasattr(self, name):
                delattr(self, name)
        self._cache = {}

    def forward(self, x, out=None, res=None):
        if self.g != 1:
            raise NotImplementedError("RepConv with groups != 1 is outside the built path (the YOLOv9 YAMLs never use it)")
        c = self.conv if hasattr(self, "conv") else self.conv1.conv
        return ops.conv2d(self, [x], self.folded, 3, c.stride[0], 1, _act_code(self.act), out=out, res=res)

    forward_fuse = forward


class DSConv(_Packed):
    """Depthwise-separable conv: dw kxk -> pw 1x1 -> BN -> SiLU (reference conv.py:87-104).  BaseModel.fuse does
    not touch it (tasks.py:224), so its BatchNorm stays a module; it is folded into the packed pw weights here."""

    def __init__(self, c_in, c_out, k=3, s=1, p=None, d=1, bias=False):
        super().__init__()
        if p is None:
            p = (d * (k - 1)) // 2
        self.dw = nn.Conv2d(c_in, c_in, kernel_size=k, stride=s, padding=p, dilation=d, groups=c_in, bias=bias)
        self.pw = nn.Conv2d(c_in, c_out, 1, 1, 0, bias=bias)
        self.bn = nn.BatchNorm2d(c_out)
        self.act = nn.SiLU()

    def _dw_folded(self):
        return fold_bn(self.dw.weight, None, None)[0], (self.dw.bias.detach().float() if self.dw.bias is not None else None)

    def _pw_folded(self):
        return fold_bn(self.pw.weight, self.pw.bias, self.bn)

    def forward(self, x, out=None, res=None):
        k, s, d = self.dw.kernel_size[0], self.dw.stride[0], self.dw.dilation[0]
        if s == 2 and d == 1 and self.dw.padding[0] == k // 2 and k in (3, 5, 7) and self.dw.stride[1] == 2:
            # DSConv(c, c, k, 2) (yolov13 layers 5 and 7): stride-2 depthwise (rounded to the storage type like the reference's
            # intermediate tensor), then the pointwise 1x1 + BN + SiLU on the MFMA conv
            t = ops.dwconv_s2(self, x, self._dw_folded, k, L.ACT_NONE)
            return ops.conv2d(self, [t], self._pw_folded, 1, 1, 0, L.ACT_SILU, out=out, res=res, tag="pw")
        if s != 1 or d != 1 or self.dw.padding[0] != k // 2:
            raise NotImplementedError("DSConv with dilation != 1 or a stride other than 1 and 2 is outside the detection path")
        y = ops.dsconv(self, x, self._dw_folded, self._pw_folded, k, L.ACT_SILU, out=out, res=res)  # one fused kernel
        if y is not None:
            return y
        t = ops.dwconv(self, x, self._dw_folded, k, L.ACT_NONE, tag="dw")
        return ops.conv2d(self, [t], self._pw_folded, 1, 1, 0, L.ACT_SILU, out=out, res=res, tag="pw")


class Concat(nn.Module):
    """Channel concat (reference conv.py:345-355).  Stand-alone it copies slices on the device and returns a tensor;
    inside a DetectionModel whose consumer starts with a 1x1 conv (`lazy=True`, set by the graph builder) it returns a
    VirtualCat that the conv reads in place."""

    lazy = False

    def __init__(self, dimension=1):
        super().__init__()
        self.d = dimension

    def forward(self, x):
        if self.d != 1:
            raise NotImplementedError("Concat along dim != 1")
        if self.lazy:
            parts = []
            for t in x:
                parts += t.parts if isinstance(t, ops.VirtualCat) else [(t, 0)]
            if len(parts) <= 2:
                return ops.VirtualCat(parts)
        return ops.concat(x)


class Upsample(nn.Module):
    """nn.Upsample(None, 2, 'nearest') of the YAMLs (layers 11, 14)."""

    def __init__(self, size=None, scale_factor=None, mode="nearest"):
        super().__init__()
        if size is not None or int(scale_factor) != 2 or mode != "nearest":
            raise NotImplementedError("only nearest x2 upsampling is on the detection path")
        self.scale_factor, self.mode = scale_factor, mode

    lazy = False

    def forward(self, x):
        if self.lazy and torch.is_tensor(x):
            return ops.VirtualCat([(x, 1)])
        return ops.upsample2x(x)
