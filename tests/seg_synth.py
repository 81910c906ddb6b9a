"""Synthetic weights and mask-assembly cases for the segment task, shared by tests/golden/make_golden_seg.py and the tests.
synthdata.synth_tensor sizes a 4-d weight by shape[1] * k * k, which for the [Cin, Cout, 2, 2] weight of Proto.upsample
(nn.ConvTranspose2d) is 4 Cout: every output pixel of a k2/s2 transposed conv sums Cin terms (one tap), so that rule would halve the
signal.  The weight is drawn here with variance gain / Cin instead; every other key goes through synthdata unchanged."""
import zlib

import numpy as np
import torch

import synthdata as synth

GAIN = 1.9  # as make_golden.py for the n scale
NAME = "yolo11{}-seg.yaml"
SCALES = "nsmlx"
SEG_ARGS = ["nc", 32, 256]  # the Segment row of yolo11-seg.yaml: [nc, nm, npr]


def synth_tensor(name, shape, gain=GAIN):
    if name.endswith("upsample.weight") and len(shape) == 4:
        r = np.random.default_rng([zlib.crc32(name.encode()), 0])
        b = (3.0 * gain / shape[0]) ** 0.5
        return torch.tensor(r.uniform(-b, b, shape), dtype=torch.float32)
    return synth.synth_tensor(name, tuple(shape), gain=gain)


def state_dict(own, gain=GAIN, prefix=""):
    """own: a module's / model's state_dict (or {key: shape}).  Returns synthetic tensors of the same shapes."""
    return {k: synth_tensor(prefix + k, tuple(v.shape) if hasattr(v, "shape") else tuple(v), gain) for k, v in own.items()}


def edgeline_seg_cfg(load):
    """yolo11-test.yaml (EdgeLine) as a dict with its last row swapped to Segment; load = the caller's YAML reader (path-free here)."""
    d = dict(load)
    d["head"] = [list(r) for r in d["head"]]
    d["head"][-1] = [d["head"][-1][0], 1, "Segment", list(SEG_ARGS)]
    return d


# ---- module-level cases: (tag, constructor args, input shapes)
PROTO_CASES = [("proto_c16_32_8_5x7", (16, 32, 8), (2, 16, 5, 7)), ("proto_c64_64_32_3x4", (64, 64, 32), (1, 64, 3, 4))]
SEGMENT_CASE = ("segment_n", dict(nc=80, nm=32, npr=64, ch=(64, 128, 256)), [(1, 64, 8, 12), (1, 128, 4, 6), (1, 256, 2, 3)])


def case_input(tag, shape):
    r = np.random.default_rng([zlib.crc32(tag.encode()), 7])
    return torch.tensor(r.normal(0.0, 1.0, shape), dtype=torch.float32)


# ---- process_mask cases of seg_ops.npz: gaussian inputs; `half` = drawn representable in f16
def _gauss(r, shape, half):
    a = r.normal(0.0, 1.0, shape).astype(np.float32)
    return a.astype(np.float16).astype(np.float32) if half else a


def boxes_for(r, n, ih, iw, s):
    """n boxes (xyxy, network-input pixels) cycling through the kinds that matter: on exact multiples of s (the >= / < ties), fractional,
    zero area, covering one low-resolution pixel, larger than the image (negative corners), wholly outside."""
    out = np.zeros((n, 4), np.float32)
    mh, mw = ih // s, iw // s
    for i in range(n):
        kind = i % 6
        if kind == 0:  # multiples of s
            x1, x2 = sorted(r.integers(0, mw + 1, 2) * s)
            y1, y2 = sorted(r.integers(0, mh + 1, 2) * s)
            if x1 == x2:
                x2 = min(x1 + s, iw)
            if y1 == y2:
                y2 = min(y1 + s, ih)
        elif kind == 1:  # fractional
            x1, x2 = sorted(r.uniform(0, iw, 2))
            y1, y2 = sorted(r.uniform(0, ih, 2))
        elif kind == 2:  # zero area
            x1 = x2 = float(r.uniform(0, iw))
            y1, y2 = sorted(r.uniform(0, ih, 2))
        elif kind == 3:  # one low-resolution pixel
            c, q = int(r.integers(0, mw)), int(r.integers(0, mh))
            x1, x2, y1, y2 = c * s - 0.25 * s, c * s + 0.5 * s, q * s - 0.25 * s, q * s + 0.5 * s
        elif kind == 4:  # larger than the image
            x1, y1, x2, y2 = -3.5 * s, -1.0 * s, iw + 2.25 * s, ih + 7.0 * s
        else:  # wholly outside
            x1, y1, x2, y2 = iw + 1.0, ih + 2.0, iw + 9.0, ih + 11.0
        out[i] = (x1, y1, x2, y2)
    return out


PM_GOLDEN = [("pm_s1_f32", 1, False, 32, 9, 13, 7), ("pm_s2_f32", 2, False, 32, 17, 33, 9), ("pm_s4_f32", 4, False, 32, 16, 24, 12),
             ("pm_s1_f16", 1, True, 8, 5, 7, 6), ("pm_s2_f16", 2, True, 40, 16, 24, 8), ("pm_s4_f16", 4, True, 32, 17, 33, 11)]


def pm_golden_case(tag, s, half, nm, mh, mw, n):
    """-> protos [nm,mh,mw], masks_in [n,nm], boxes [n,4] (numpy fp32), shape (ih, iw)."""
    r = np.random.default_rng([zlib.crc32(tag.encode()), 3])
    return _gauss(r, (nm, mh, mw), half), _gauss(r, (n, nm), half), boxes_for(r, n, mh * s, mw * s, s), (mh * s, mw * s)


def nms_pred(nc=4, nm=32, a=200, imgsz=96):
    """(1, 4+nc+nm, A) prediction with mask coefficients behind the classes."""
    p = synth.synth_pred(1, nc, a, seed=5, imgsz=imgsz, dense=True)
    r = np.random.default_rng([zlib.crc32(b"nms_coef"), 5])
    return torch.cat([p, torch.tensor(r.normal(0, 1, (1, nm, a)), dtype=torch.float32)], 1)
