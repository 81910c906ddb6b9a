"""DySample, the content-aware upsampler of the newer YOLOv13 YAMLs (reference ultralytics/nn/modules/dysample.py:20-93), HIP-backed.

Same constructor signature, asserts, attribute names and state_dict keys (`init_pos`, `offset.weight`, `offset.bias`, `scope.weight`) as
the reference, so its state_dict loads unchanged.  The `nn.Conv2d` children are parameter containers only.  forward() packs the
offset / scope weights as [8 groups][C] matrices on first use and runs ey_dysample: one launch computes the offsets of a pixel tile
and gathers the four output pixels of every input pixel; the offset map and the sampling grid are never written.
"""
import torch
import torch.nn as nn

from .. import _ops as ops
from .conv import _Packed

__all__ = ("DySample", "pl_to_dense")


def pl_to_dense(w, b=None, scale=2):
    """The 'pl' style as an 'lp'-shaped 1x1 conv.  'pl' runs its conv on pixel_shuffle(x) and un-shuffles the result; since
    pixel_shuffle(x)[c', s h + i, s w + j] = x[s^2 c' + s i + j, h, w], row r of the (R, C / s^2) weight becomes the s^2 rows
    r s^2 + q of an (R s^2, C) weight that read channel c only where c % s^2 == q:  W'[r s^2 + q, c] = W[r, c // s^2] [c % s^2 == q].
    The bias is repeated the same way.  Returns (W', b') (b' None without a bias)."""
    s2 = scale * scale
    w = w.reshape(w.shape[0], -1)
    rows, cq = w.shape
    dense = w.new_zeros(rows, s2, cq, s2)
    for q in range(s2):
        dense[:, q, :, q] = w
    return dense.reshape(rows * s2, cq * s2), (None if b is None else b.repeat_interleave(s2))


class DySample(_Packed):
    """DySample(in_channels, scale=2, style='lp', groups=4, dyscope=False): (B, C, H, W) -> (B, C, 2H, 2W)."""

    def __init__(self, in_channels, scale=2, style="lp", groups=4, dyscope=False):
        super().__init__()
        self.scale = scale
        self.style = style
        self.groups = groups
        assert style in ["lp", "pl"]
        if scale != 2:
            raise NotImplementedError(f"DySample: scale={scale} (the HIP kernel is built for scale=2)")
        if groups not in (2, 4, 8):
            raise NotImplementedError(f"DySample: groups={groups} (the HIP kernel is built for groups 2, 4 and 8)")
        if self.style == "lp":
            assert (2 * groups) % scale ** 2 == 0, f"'lp' shuffles 2 * groups = {2 * groups} offset maps by {scale}: not a multiple of {scale ** 2}"
        if style == "pl":
            assert in_channels >= scale ** 2 and in_channels % scale ** 2 == 0
        assert in_channels >= groups and in_channels % groups == 0
        self.in_channels = in_channels
        if style == "pl":
            c, out_channels = in_channels // scale ** 2, 2 * groups
        else:
            c, out_channels = in_channels, 2 * groups * scale ** 2
        self.offset = nn.Conv2d(c, out_channels, 1)
        nn.init.normal_(self.offset.weight, 0, 0.001)
        nn.init.constant_(self.offset.bias, 0)
        if dyscope:
            self.scope = nn.Conv2d(c, out_channels, 1, bias=False)
            nn.init.constant_(self.scope.weight, 0.0)
        self.register_buffer("init_pos", self._init_pos().to(dtype=self.offset.weight.dtype))

    def _init_pos(self):
        """(1, 2 * groups * scale^2, 1, 1): channel xy * G s^2 + grp * s^2 + i * s + j holds the centre of output sub-pixel (i, j) relative to
        the input pixel's centre, in input pixels: (j - (s - 1) / 2) / s for x, (i - (s - 1) / 2) / s for y (+-0.25 at scale 2)."""
        s, g = self.scale, self.groups
        c = (torch.arange(s, dtype=torch.float32) - (s - 1) / 2) / s
        px = c.view(1, 1, s).expand(g, s, s)  # varies with j
        py = c.view(1, s, 1).expand(g, s, s)  # varies with i
        return torch.stack([px, py]).reshape(1, -1, 1, 1).clone()

    def dense_weights(self):
        """fp32 (offset weight (8G, C), bias (8G,), scope weight (8G, C) or None): the matrices ey_dysample takes, both styles."""
        w, b = self.offset.weight.detach().float().flatten(1), self.offset.bias.detach().float()
        s = self.scope.weight.detach().float().flatten(1) if hasattr(self, "scope") else None
        if self.style == "pl":
            w, b = pl_to_dense(w, b, self.scale)
            if s is not None:
                s = pl_to_dense(s, None, self.scale)[0]
        return w, b, s

    def forward(self, x, out=None):
        return ops.dysample(self, x, out=out)
