"""Synthetic weights, inputs and cases for the classify task, shared by tests/golden/make_golden_cls.py and the tests.  Everything is drawn
from seeded generators keyed by a case tag, so the generator (which runs the reference and Pillow) and the tests (which do not) build
bit-identical inputs."""
import zlib

import numpy as np
import torch

import synthdata as synth

GAIN = 1.9
NAME = "yolo11{}-cls.yaml"
SCALES = "nsmlx"
C_ = 1280  # width of the Classify head's conv (reference head.py:462)


def state_dict(own, gain=GAIN, prefix=""):
    return {k: synth.synth_tensor(prefix + k, tuple(v.shape) if hasattr(v, "shape") else tuple(v), gain=gain) for k, v in own.items()}


def _rng(tag, seed=0):
    return np.random.default_rng([zlib.crc32(tag.encode()), seed])


def _f16(a):
    return a.astype(np.float16).astype(np.float32)


# ---- the Classify head on a small map: (tag, c1, c2, input shape)
HEAD_CASE = ("cls_head", 64, 10, (2, 64, 3, 5))


def case_input(tag, shape):
    return torch.tensor(_rng(tag, 7).normal(0.0, 1.0, shape), dtype=torch.float32)


# ---- ey_classify_pool: (tag, B, C1, H, W, Cout, exact)
# exact: integer inputs in [-2, 2], weights and biases in multiples of 1/4, no activation, H W a power of two -> every sum, and the division,
# is exact in fp32 in any order.  Otherwise SiLU on general data.  C1 = 8 is the half-filled MFMA k-step, 768 the 32-pixel LDS tile
# (several tiles at 8x8 and 20x20); Cout = 48 and 160 end inside a workgroup's 128 channels, 1280 is the head's own width.
POOL_CASES = [
    ("cp_x_b1_c8_1x1", 1, 8, 1, 1, 48, True),
    ("cp_x_b3_c256_2x2", 3, 256, 2, 2, 1280, True),
    ("cp_x_b33_c768_8x8", 33, 768, 8, 8, 160, True),
    ("cp_b1_c256_7x7", 1, 256, 7, 7, 1280, False),
    ("cp_b3_c8_9x9", 3, 8, 9, 9, 160, False),
    ("cp_b33_c768_20x20", 33, 768, 20, 20, 48, False),
]
POOL_SLICED = ("cp_sliced_b3_c256_7x7", 3, 256, 7, 7, 160, False)


def pool_case(tag, B, C1, H, W, Cout, exact, half):
    """-> x (B, C1, H, W), w (Cout, C1), bias (Cout,) float32 numpy (f16-representable x and w when half)."""
    r = _rng(tag, 1)
    if exact:
        x = r.integers(-2, 3, (B, C1, H, W)).astype(np.float32)
        w = (r.integers(-4, 5, (Cout, C1)) / 4.0).astype(np.float32)
        b = (r.integers(-8, 9, Cout) / 4.0).astype(np.float32)
        return x, w, b
    x = r.normal(0.0, 1.0, (B, C1, H, W)).astype(np.float32)
    lim = (3.0 * GAIN / C1) ** 0.5
    w = r.uniform(-lim, lim, (Cout, C1)).astype(np.float32)
    b = r.normal(0.0, 0.1, Cout).astype(np.float32)
    return (_f16(x), _f16(w), b) if half else (x, w, b)


# ---- ey_classify_linear_softmax: tag -> (B, nc, half, kind)
LINEAR_NC = [1, 2, 5, 6, 80, 1000, 1001, 8192]
LINEAR_CASES = {f"ls_nc{nc}_b{B}": (B, nc, B == 33, "plain") for nc in LINEAR_NC for B in (1, 33)}
LINEAR_CASES["ls_big_nc80_b3"] = (3, 80, False, "big")  # logits near +-80: exp(l - max) must not overflow
LINEAR_CASES["ls_nc80_b130"] = (130, 80, True, "plain")  # four images per workgroup
LINEAR_TIE = ("ls_tie_nc80_b2", 2, 80)  # all logits equal: judged against the tie rule only
LINEAR_FULL = [t for t, c in LINEAR_CASES.items() if c[1] <= 80 and c[0] <= 33]  # cases whose fp32 reference rows are kept in the golden


LINEAR_SEED = {"ls_nc1001_b1": 3}  # seeds the generator had to move: two of the first six probabilities of a row closer than twice the bound


def linear_case(tag):
    """-> pooled (B, 1280), w (nc, 1280), bias (nc,) float32 numpy (f16-representable w when half)."""
    B, nc, half, kind = LINEAR_CASES[tag]
    r = _rng(tag, LINEAR_SEED.get(tag, 2))
    pooled = r.normal(0.0, 0.5, (B, C_)).astype(np.float32)
    w = r.normal(0.0, 0.05, (nc, C_)).astype(np.float32)
    b = r.normal(0.0, 0.1, nc).astype(np.float32)
    if kind == "big":
        w *= np.float32(40.0)
    return pooled, (_f16(w) if half else w), b


# ---- ey_classify_transform: (tag, h, w, S): downscale in both orientations, upscale, identity, and the crop roundings: n - S = 1, 17 (the
# first nine shapes: origins 0, 8) and 3, 5 (the last two: origins 2, 2)
TRANSFORM_CASES = [
    ("ct_37x53_16", 37, 53, 16), ("ct_53x37_16", 53, 37, 16), ("ct_480x640_224", 480, 640, 224), ("ct_33x33_32", 33, 33, 32), ("ct_20x31_32", 20, 31, 32),
    ("ct_225x227_224", 225, 227, 224), ("ct_100x301_64", 100, 301, 64), ("ct_7x9_8", 7, 9, 8), ("ct_64x64_64", 64, 64, 64),
    ("ct_32x35_32", 32, 35, 32), ("ct_32x37_32", 32, 37, 32),
]


def transform_image(tag, h, w):
    """-> (h, w, 3) uint8 RGB image (the tests hand its channel-reversed, BGR, form to the kernel)."""
    if h == 480:  # a smooth ramp: compresses well in the golden and shows a shifted tap at once
        return (np.add.outer(np.arange(h), np.arange(w))[..., None] * np.array([1, 2, 3]) % 256).astype(np.uint8)
    return _rng(tag, 3).integers(0, 256, (h, w, 3), dtype=np.uint8)


def resized(h, w, S):
    return (int(S * h / w), S) if w <= h else (S, int(S * w / h))


def crop_origin(n, S):
    return int(round((n - S) / 2.0))


# ---- the end-to-end validation case (tests/golden/clsval_case.npz)
VAL_NC, VAL_SHAPE, VAL_BATCHES = 10, (4, 64, 64), 2


def val_images(i):
    B, H, W = VAL_SHAPE
    return synth.synth_images(B, H, W, seed=20 + i)


def host_probs(tag, B, nc):
    """random probability rows for the validator's host bookkeeping."""
    p = _rng(tag, 4).random((B, nc)).astype(np.float32)
    return p / p.sum(1, keepdims=True)
