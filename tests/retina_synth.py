"""Cases and input draws for masks at the original resolution (ey_process_mask_native, retina_masks=True), shared by
tests/golden/make_golden_retina.py and the tests.

OP_CASES: (mh, mw, H0, W0, nm, N, coefficient levels, byte offset of the output slice) -- the smallest shapes at which each mechanism of
the kernel can go wrong: identity, up- and downscale, an exact and a non-integer ratio, a column crop (17x33 -> 40x33 keeps columns
9..23), one cropped row (16x16 -> 61x64 keeps rows 0..14), a one-column crop over many bands (8x8 -> 300x7), more than one 256-column
tile (8x8 -> 5x301), a large non-integer ratio, N = 0 and N = 301, 1 / 3 / 4 levels, nm 8 / 32 / 40 / 64, aligned and unaligned offsets."""
import zlib

import numpy as np

import seg_synth

OP_CASES = [(2, 3, 2, 3, 8, 17, 1, 16), (2, 3, 7, 9, 32, 17, 3, 5), (5, 7, 3, 4, 40, 17, 4, 16), (16, 24, 9, 13, 64, 17, 1, 7),
            (16, 24, 16, 24, 32, 301, 3, 16), (16, 24, 64, 96, 32, 17, 3, 3), (16, 24, 37, 91, 40, 17, 4, 32), (17, 33, 40, 33, 8, 17, 1, 16),
            (16, 16, 61, 64, 64, 1, 3, 16), (8, 8, 300, 7, 32, 17, 1, 1), (8, 8, 5, 301, 8, 17, 3, 16), (40, 24, 333, 170, 32, 17, 4, 64),
            (5, 7, 3, 4, 32, 0, 3, 16)]
# the crop (top, bottom, left, right) scale_masks takes of each case's proto grid
GEOMETRY = {(2, 3, 2, 3): (0, 2, 0, 3), (2, 3, 7, 9): (0, 2, 0, 2), (5, 7, 3, 4): (0, 5, 0, 6), (16, 24, 9, 13): (0, 16, 0, 23),
            (16, 24, 16, 24): (0, 16, 0, 24), (16, 24, 64, 96): (0, 16, 0, 24), (16, 24, 37, 91): (3, 12, 0, 24), (17, 33, 40, 33): (0, 17, 9, 23),
            (16, 16, 61, 64): (0, 15, 0, 16), (8, 8, 300, 7): (0, 8, 3, 4), (8, 8, 5, 301): (3, 4, 0, 8), (40, 24, 333, 170): (0, 40, 1, 22)}
DYADIC = [(2, 3, 2, 3), (16, 24, 16, 24), (16, 24, 64, 96)]  # identity and power-of-two ratios: the blend weights are dyadic only there
MODEL_SHAPES = [(70, 150), (131, 90)]  # originals of the 64x96 model run: one wider, one taller than the input


def case_id(c):
    return f"{c[0]}x{c[1]}_to_{c[2]}x{c[3]}_nm{c[4]}_N{c[5]}_L{c[6]}_o{c[7]}"


def gauss(r, shape, half):
    return seg_synth._gauss(r, shape, half)


def boxes_for(r, n, h0, w0):
    """n boxes (xyxy, ORIGINAL-image pixels): on whole pixels (the >= / < ties), fractional, zero area, one pixel, larger than the image
    (negative corners), wholly outside -- seg_synth.boxes_for at ratio 1."""
    return seg_synth.boxes_for(r, n, h0, w0, 1)


def golden_case(case, half):
    """One image of an op case as utils.ops.process_mask_native takes it -> protos [nm,mh,mw], masks_in [n,nm], boxes [n,4] (numpy fp32),
    shape (H0, W0).  n is the case's N, at most 17."""
    mh, mw, h0, w0, nm, n = case[:6]
    n = min(n, 17)
    r = np.random.default_rng([zlib.crc32(repr((case[:6], bool(half))).encode()), 11])
    return gauss(r, (nm, mh, mw), half), gauss(r, (n, nm), half), boxes_for(r, n, h0, w0), (h0, w0)


def golden_tag(case, half):
    return f"pmn_{case[0]}x{case[1]}_{case[2]}x{case[3]}_nm{case[4]}_n{min(case[5], 17)}_{'f16' if half else 'f32'}"


def pack(bits):
    """uint8 0 / 1 array -> (packed bytes, shape), 8 pixels per byte."""
    b = np.asarray(bits, np.uint8)
    return np.packbits(b.reshape(-1)), np.array(b.shape, np.int64)


def unpack(packed, shape):
    n = int(np.prod(shape))
    return np.unpackbits(packed)[:n].reshape(tuple(int(v) for v in shape))
