"""The torch rows the YAMLs of the classic families name directly, HIP-backed: `nn.MaxPool2d`, `nn.ZeroPad2d` (yolov3-tiny) and
`nn.ConvTranspose2d` (yolov6).  (SPP of yolov3-spp is in block.py, next to SPPF.)  The three are subclasses of the torch modules: constructor signatures, state_dict keys and the layer
`type` a model reports stay torch's; forward() launches through the C ABI instead of calling torch.
"""
import torch
import torch.nn as nn

from .. import _ops as ops
from .conv import _Packed

__all__ = ("MaxPool2d", "ZeroPad2d", "ConvTranspose2d", "ZeroPadded")


def _pair(v):
    return (int(v), int(v)) if isinstance(v, int) else tuple(int(a) for a in v)


class ZeroPadded:
    """What a lazy ZeroPad2d hands to the MaxPool2d behind it: the unpadded map and the padding (left, right, top, bottom).  The pool reads
    the padding as zeros in its own launch; the padded map is never written."""

    def __init__(self, x, pad):
        self.x, self.pad = x, pad


class ZeroPad2d(nn.ZeroPad2d):
    """nn.ZeroPad2d((left, right, top, bottom)).  Stand-alone it is the zero-padded copy (ey_maxpool2d with a 1x1 window).  Inside a
    DetectionModel whose only reader of it is the MaxPool2d on the next row (`lazy = True`, set by the graph builder; yolov3-tiny rows
    11-12) it launches nothing and hands a ZeroPadded on."""

    lazy = False

    def __init__(self, padding):
        super().__init__(padding)
        if len(self.padding) != 4 or min(self.padding) < 0:
            raise NotImplementedError(f"ZeroPad2d: padding {self.padding}; non-negative (left, right, top, bottom) is built")

    def forward(self, x):
        pad = tuple(int(p) for p in self.padding)
        if self.lazy and torch.is_tensor(x):
            return ZeroPadded(x, pad)
        return ops.maxpool2d(x, 1, 1, pad)


class MaxPool2d(nn.MaxPool2d):
    """nn.MaxPool2d(2, stride 1 or 2, padding 0) on ey_maxpool2d, floor output size.  Fed by a lazy ZeroPad2d it pools the zero-padded map in
    the same launch: the padded cells are zeros that take part in the maximum, as in the reference."""

    def __init__(self, kernel_size, stride=None, padding=0, dilation=1, return_indices=False, ceil_mode=False):
        super().__init__(kernel_size, stride, padding, dilation, return_indices, ceil_mode)
        k, s, p, d = _pair(self.kernel_size), _pair(self.stride), _pair(self.padding), _pair(self.dilation)
        if k != (2, 2) or s not in ((1, 1), (2, 2)) or p != (0, 0) or d != (1, 1) or self.return_indices or self.ceil_mode:
            raise NotImplementedError(f"MaxPool2d({self.extra_repr()}): the pooling kernel is built for a 2x2 window, stride 1 or 2, no padding of its "
                                      "own (nn.ZeroPad2d in front pads with zeros), no dilation, floor mode, no indices")

    def forward(self, x, out=None):
        s = _pair(self.stride)[0]
        if isinstance(x, ZeroPadded):
            return ops.maxpool2d(x.x, 2, s, x.pad, out=out)
        return ops.maxpool2d(x, 2, s, out=out)


class ConvTranspose2d(nn.ConvTranspose2d, _Packed):  # (torch's class first: its name is the layer type a model reports)
    """nn.ConvTranspose2d(c1, c2, 2, 2, 0) of the YOLOv6 neck on ey_deconv2x2 (one GEMM launch with a scatter epilogue; channels multiples of 8
    up to 384).  The packed weight is cached per (dtype, device) and dropped whenever the parameters move or reload."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, output_padding=0, groups=1, bias=True, dilation=1):
        super().__init__(in_channels, out_channels, kernel_size, stride, padding, output_padding, groups, bias, dilation)
        if (self.kernel_size != (2, 2) or self.stride != (2, 2) or self.padding != (0, 0) or self.output_padding != (0, 0) or self.groups != 1
                or self.dilation != (1, 1)):
            raise NotImplementedError(f"ConvTranspose2d({self.extra_repr()}): the kernel is built for a dense kernel 2, stride 2, padding 0")

    def forward(self, x, out=None):
        return ops.deconv2x2(self, x, self, out=out)
