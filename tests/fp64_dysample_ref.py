"""DySample (scale 2) restated in float64 torch, in pixel coordinates.  F.grid_sample(align_corners=False, padding_mode="border") on
the reference's normalised grid 2 (w + 0.5 + O_x) / W - 1 un-normalises to ((g + 1) W - 1) / 2 = w + O_x, so:

    O[b, n, h, w] = (W_off[n] . x[b, :, h, w] + bias[n]) * 0.25 + init_pos[n]                                   (no scope)
    O[b, n, h, w] = (W_off[n] . x[b, :, h, w] + bias[n]) * sigmoid(W_scope[n] . x[b, :, h, w]) * 0.5 + init_pos[n]
    n = xy * 4G + grp * 4 + i * 2 + j;   ix = clamp(w + O_x, 0, W-1), iy = clamp(h + O_y, 0, H-1)
    y[b, c, 2h+i, 2w+j] = bilinear blend of x[b, c] at (iy, ix), the upper neighbour index clamped to the map, c in group grp

Weights are the dense (8G, C) matrices ('pl' modules: after pl_to_dense).  Everything float64, no GPU, no reference import."""
import torch


def offsets(x, w, b, s, init_pos, parts=False):
    """x (B,C,H,W), w / s (8G,C), b / init_pos (8G,) -> O (B,8G,H,W).  parts=True: also lin, the scope logits (or None) and
    sum |terms| of both products (the magnitudes an error bound needs)."""
    x, w, b, pos = x.double(), w.double(), b.double(), init_pos.double().flatten()
    lin = torch.einsum("nc,bchw->bnhw", w, x) + b[None, :, None, None]
    sc = None
    if s is not None:
        sc = torch.einsum("nc,bchw->bnhw", s.double(), x)
        o = lin * torch.sigmoid(sc) * 0.5 + pos[None, :, None, None]
    else:
        o = lin * 0.25 + pos[None, :, None, None]
    if not parts:
        return o
    mag = torch.einsum("nc,bchw->bnhw", w.abs(), x.abs()) + b.abs()[None, :, None, None]
    smag = None if s is None else torch.einsum("nc,bchw->bnhw", s.double().abs(), x.abs())
    return o, lin, sc, mag, smag


def _to_out(t, B, H, W):
    """(B, G, Cg, 2(i), 2(j), H, W) -> (B, G*Cg, 2H, 2W)"""
    return t.permute(0, 1, 2, 5, 3, 6, 4).reshape(B, -1, 2 * H, 2 * W)


def sample(x, o, groups, parts=False):
    """x (B,C,H,W), o (B,8G,H,W) -> y (B,C,2H,2W).  parts=True: also (iy0, ix0) of every (b, grp, i, j, h, w) and the largest |corner|
    per output element."""
    x, o = x.double(), o.double()
    B, C, H, W = x.shape
    G = groups
    o = o.view(B, 2, G, 2, 2, H, W)
    ix = (torch.arange(W, dtype=torch.float64).view(1, 1, 1, 1, 1, W) + o[:, 0]).clamp(0, W - 1)
    iy = (torch.arange(H, dtype=torch.float64).view(1, 1, 1, 1, H, 1) + o[:, 1]).clamp(0, H - 1)
    x0, y0 = ix.floor().long(), iy.floor().long()
    x1, y1 = (x0 + 1).clamp(max=W - 1), (y0 + 1).clamp(max=H - 1)
    lx, ly = ix - x0, iy - y0
    xg = x.reshape(B, G, C // G, H * W)

    def corner(yy, xx):
        idx = (yy * W + xx).reshape(B, G, 1, -1).expand(B, G, C // G, 4 * H * W)
        return xg.gather(3, idx).view(B, G, C // G, 2, 2, H, W)

    v00, v01, v10, v11 = corner(y0, x0), corner(y0, x1), corner(y1, x0), corner(y1, x1)
    lx, ly = lx.unsqueeze(2), ly.unsqueeze(2)
    y = _to_out((1 - lx) * (1 - ly) * v00 + lx * (1 - ly) * v01 + (1 - lx) * ly * v10 + lx * ly * v11, B, H, W)
    if not parts:
        return y
    vmax = _to_out(torch.stack([v00.abs(), v01.abs(), v10.abs(), v11.abs()]).amax(0), B, H, W)
    return y, y0, x0, vmax


def gather_at(t, y0, x0, groups):
    """t (B,C,H,W) read at the (y0, x0) that sample(parts=True) returned -> (B,C,2H,2W): t[b, c, y0, x0] of every output element."""
    B, C, H, W = t.shape
    G = groups
    idx = (y0 * W + x0).reshape(B, G, 1, -1).expand(B, G, C // G, 4 * H * W)
    return _to_out(t.reshape(B, G, C // G, H * W).gather(3, idx).view(B, G, C // G, 2, 2, H, W), B, H, W)


def per_group_to_out(t, channels):
    """t (B,G,2,2,H,W), one value per (group, output pixel) -> (B,C,2H,2W) with the group's value on each of its C/G channels."""
    B, G, _, _, H, W = t.shape
    return _to_out(t.unsqueeze(2).expand(B, G, channels // G, 2, 2, H, W), B, H, W)


def dysample(x, w, b, s, init_pos, groups):
    return sample(x, offsets(x, w, b, s, init_pos), groups)
