"""float64 restatement of mask assembly at the original resolution, written from the definition (not copied from the reference):

    v    = coef_n . proto                                   on the proto grid
    v    = v[top:bottom, left:right]                        scale_masks' crop (top, bottom, left, right come with the case)
    V    = bilinear(v -> (H0, W0)), align_corners=False     any ratio: source coordinate max((in / out)(dst + 0.5) - 0.5, 0) -- dst itself when
                                                            in == out --, lower index floor(src) clamped to in - 1, upper neighbour clamped too
    bit  = V > 0 and ox >= x1 and ox < x2 and oy >= y1 and oy < y2      the box in ORIGINAL-image pixels, compared in fp32 (part of the definition)

Also returns the magnitude sum sum_k |coef_k proto_k| carried through the same crop and blend, the largest |corner v| of every output
pixel and the in-box predicate.  The error bound of an fp32 evaluation is
    E = 1.05 * [(nm + 2) u blend(sum|coef proto|) + 8 u max|corner v| + 2 (ex + ey) max|corner v|],   u = 2^-24,
    e = 4 u max(source coordinate, 1)
(nm + 2 roundings of the dot product at the corners, each weighted as the blend weighs them; the blend's own roundings; the fp32 source
coordinate: a shift d of a blend weight moves the blend by at most 2 d max|corner|)."""
import numpy as np

U = 2.0 ** -24


def axis(n_out, n_in):
    """-> lower index, upper index, upper weight, source coordinate of every target coordinate (float64)."""
    o = np.arange(n_out, dtype=np.float64)
    src = o.copy() if n_in == n_out else np.maximum((n_in / n_out) * (o + 0.5) - 0.5, 0.0)
    i0 = np.minimum(np.floor(src).astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    return i0, i1, np.clip(src - i0, 0.0, 1.0), src


def process_mask_native64(proto, coef, boxes, geo):
    """proto [nm,mh,mw], coef [n,nm], boxes [n,4] xyxy (original pixels), geo = (top, bottom, left, right, H0, W0)
    -> dict(v, mag, corner, bits, inbox, eps), each [n, H0, W0] (eps [H0, W0])."""
    proto, coef = np.asarray(proto, np.float64), np.asarray(coef, np.float64)
    top, bottom, left, right, h0, w0 = (int(g) for g in geo)
    assert top < bottom and left < right, "empty crop"
    p = proto[:, top:bottom, left:right]
    v = np.einsum("nk,khw->nhw", coef, p)
    mag = np.einsum("nk,khw->nhw", np.abs(coef), np.abs(p))
    y0, y1, ly, sy = axis(h0, bottom - top)
    x0, x1, lx, sx = axis(w0, right - left)
    ly, lx = ly[None, :, None], lx[None, None, :]

    def blend(t):
        a, b = t[:, y0][:, :, x0], t[:, y0][:, :, x1]
        c, d = t[:, y1][:, :, x0], t[:, y1][:, :, x1]
        return (1 - ly) * ((1 - lx) * a + lx * b) + ly * ((1 - lx) * c + lx * d), np.maximum(np.maximum(np.abs(a), np.abs(b)), np.maximum(np.abs(c), np.abs(d)))

    V, corner = blend(v)
    M, _ = blend(mag)
    bx = np.asarray(boxes, np.float32).reshape(-1, 4)
    ox = np.arange(w0, dtype=np.float32)[None, None, :]
    oy = np.arange(h0, dtype=np.float32)[None, :, None]
    bx1, by1, bx2, by2 = (bx[:, i][:, None, None] for i in range(4))
    inbox = (ox >= bx1) & (ox < bx2) & (oy >= by1) & (oy < by2)  # fp32 on purpose; a NaN corner compares false
    eps = 4 * U * (np.maximum(sy, 1.0)[:, None] + np.maximum(sx, 1.0)[None, :])
    return dict(v=V, mag=M, corner=corner, bits=((V > 0) & inbox).astype(np.uint8), inbox=inbox, eps=eps)


def mask_bound(ref, nm):
    return 1.05 * ((nm + 2) * U * ref["mag"] + 8 * U * ref["corner"] + 2 * ref["eps"][None] * ref["corner"])


def check_bits(got, ref, nm, cap=1e-3):
    """got uint8 [n,H0,W0] against process_mask_native64's result: 0 outside the box, equal to the fp64 bits wherever |V| > E inside;
    returns (undecided, in-box pixels) and asserts the undecided share of the in-box pixels stays under `cap`."""
    got = np.asarray(got)
    assert got.shape == ref["bits"].shape, f"shape {got.shape}, expected {ref['bits'].shape}"
    inbox = ref["inbox"]
    assert not (got[~inbox] != 0).any(), "a set byte outside the box"
    decided = np.abs(ref["v"]) > mask_bound(ref, nm)
    bad = decided & inbox & (got != ref["bits"])
    assert not bad.any(), f"{int(bad.sum())} pixels differ from the fp64 bits outside the bound, first at {np.argwhere(bad)[0].tolist()}"
    und, tot = int((~decided & inbox).sum()), int(inbox.sum())
    assert und <= cap * max(tot, 1), f"{und} of {tot} in-box pixels are within the bound of zero (cap {cap})"
    return und, tot
