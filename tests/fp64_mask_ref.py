"""float64 restatements for the segment task, written from the definitions (not copied from the reference):

process_mask64: v = sum_k coef_k proto_k on the low-resolution grid; crop (column c kept where c >= x1/s and c < x2/s, row r where
r >= y1/s and r < y2/s, the box scaled by 1/s IN fp32 as the reference and the kernel do -- the comparisons are part of the definition);
bilinear align_corners=False to (s mh, s mw): source coordinate (dst + 0.5)/s - 0.5 clamped at 0, upper neighbour clamped to the map;
bit = v > 0.  Also returns the magnitude sum sum_k |coef_k proto_k| carried through the same crop and blend and the largest |corner v| of
every output pixel: the error bound of an fp32 evaluation is
    E = 1.05 * [(nm + 2) u blend(sum|coef proto|) + 8 u max|corner v|],  u = 2^-24
(nm + 2 roundings of the dot product at the corners, each weighted as the blend weighs them; the blend itself is three fp32 lerps).

deconv64: y[b, co, 2i+di, 2j+dj] = bias[co] + sum_ci x[b, ci, i, j] W[ci, co, di, dj] and the sum of |terms| (|bias| included).
"""
import numpy as np

U = 2.0 ** -24


def _axis(n_out, n_in, s):
    src = np.maximum((np.arange(n_out, dtype=np.float64) + 0.5) / s - 0.5, 0.0)
    i0 = np.floor(src).astype(np.int64)
    i0 = np.minimum(i0, n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    return i0, i1, src - i0


def process_mask64(proto, coef, boxes, s):
    """proto [nm,mh,mw], coef [n,nm], boxes [n,4] xyxy (input pixels) -> dict(v, mag, corner, bits), each [n, s mh, s mw]."""
    proto = np.asarray(proto, np.float64)
    coef = np.asarray(coef, np.float64)
    nm, mh, mw = proto.shape
    n = coef.shape[0]
    v = np.einsum("nk,khw->nhw", coef, proto)
    mag = np.einsum("nk,khw->nhw", np.abs(coef), np.abs(proto))
    b = np.asarray(boxes, np.float32) * np.float32(1.0 / s)  # fp32 on purpose (see the module docstring)
    c = np.arange(mw, dtype=np.float32)[None, None, :]
    r = np.arange(mh, dtype=np.float32)[None, :, None]
    x1, y1, x2, y2 = (b[:, i][:, None, None] for i in range(4))
    keep = (c >= x1) & (c < x2) & (r >= y1) & (r < y2)
    v = v * keep
    mag = mag * keep
    if s == 1:
        return dict(v=v, mag=mag, corner=np.abs(v), bits=(v > 0).astype(np.uint8))
    y0, y1i, ly = _axis(mh * s, mh, s)
    x0, x1i, lx = _axis(mw * s, mw, s)
    ly, lx = ly[None, :, None], lx[None, None, :]

    def blend(t):
        a, bq = t[:, y0][:, :, x0], t[:, y0][:, :, x1i]
        cq, d = t[:, y1i][:, :, x0], t[:, y1i][:, :, x1i]
        return (1 - ly) * ((1 - lx) * a + lx * bq) + ly * ((1 - lx) * cq + lx * d), np.maximum(np.maximum(np.abs(a), np.abs(bq)), np.maximum(np.abs(cq), np.abs(d)))

    V, corner = blend(v)
    M, _ = blend(mag)
    return dict(v=V, mag=M, corner=corner, bits=(V > 0).astype(np.uint8))


def mask_bound(ref, nm):
    return 1.05 * ((nm + 2) * U * ref["mag"] + 8 * U * ref["corner"])


def check_bits(got, ref, nm, boxes=None, cap=1e-3):
    """got uint8 [n,h,w] against process_mask64's result: equal wherever |v| > E; returns (undecided pixels, pixels with v != 0 or mag != 0)
    and asserts the share of undecided in-box pixels stays under `cap`."""
    E = mask_bound(ref, nm)
    decided = np.abs(ref["v"]) > E
    bad = decided & (got != ref["bits"])
    assert not bad.any(), f"{int(bad.sum())} pixels differ from the fp64 bits outside the bound, first at {np.argwhere(bad)[0].tolist()}"
    inbox = ref["mag"] > 0
    # a pixel with mag == 0 has v == 0 exactly in any arithmetic (every term is zero or cropped): it must be 0
    assert not (got[~inbox] != 0).any(), "non-zero bit where every term is zero"
    und = int((~decided & inbox).sum())
    tot = int(inbox.sum())
    assert und <= cap * max(tot, 1), f"{und} of {tot} in-box pixels are within the bound of zero (cap {cap})"
    return und, tot


def deconv64(x, w, bias):
    """x [B,Cin,H,W], w [Cin,Cout,2,2], bias [Cout] -> (y, mag) [B,Cout,2H,2W] in float64."""
    x, w, bias = np.asarray(x, np.float64), np.asarray(w, np.float64), np.asarray(bias, np.float64)
    B, _, H, W = x.shape
    co = w.shape[1]
    y = np.zeros((B, co, 2 * H, 2 * W))
    mag = np.zeros_like(y)
    for di in range(2):
        for dj in range(2):
            y[:, :, di::2, dj::2] = np.einsum("bihw,io->bohw", x, w[:, :, di, dj]) + bias[None, :, None, None]
            mag[:, :, di::2, dj::2] = np.einsum("bihw,io->bohw", np.abs(x), np.abs(w[:, :, di, dj])) + np.abs(bias)[None, :, None, None]
    return y, mag
