"""Synthetic weights, inputs and cases for the YOLOv9 (GELAN) tests, shared by tests/golden/make_golden_v9.py and the tests.  Everything is
drawn from seeded generators keyed by a case tag, so the generator (which runs the reference) and the tests (which do not) build bit-identical
inputs."""
import zlib

import numpy as np
import torch

import synthdata as synth

GAIN = 1.9
FILES = ["yolov9t.yaml", "yolov9s.yaml", "yolov9m.yaml", "yolov9c.yaml", "yolov9e.yaml", "yolov9c-seg.yaml", "yolov9e-seg.yaml"]
PARAMS = {"yolov9t.yaml": 2128720, "yolov9s.yaml": 7318368, "yolov9m.yaml": 20216160, "yolov9c.yaml": 25590912, "yolov9e.yaml": 58206592,
          "yolov9c-seg.yaml": 27897120}  # (yolov9e-seg.yaml: whatever the reference reports, structure_v9.json)
TASK = {f: "segment" if "-seg" in f else "detect" for f in FILES}


def state_dict(own, gain=GAIN, prefix=""):
    """Seeded tensors for every key of `own` (a state_dict, or {key: shape}).  A CBLinear (a `conv` with a bias and no BatchNorm beside it)
    gets a quarter of the usual amplitude: yolov9e's main branch sums up to five of their outputs into each of its maps, five times over, and
    at full amplitude the activations grow past what f16 holds."""
    out = {}
    for k, v in own.items():
        t = synth.synth_tensor(prefix + k, tuple(v.shape) if hasattr(v, "shape") else tuple(v), gain=gain)
        stem = k.rsplit(".", 1)[0]
        if stem.endswith("conv") and stem + ".bias" in own and stem[:-4] + "bn.weight" not in own and k.rsplit(".", 1)[1] in ("weight", "bias"):
            t = t * 0.25
        out[k] = t
    return out


def pack_keys(keys):
    """state_dict keys -> {"suffixes": [[two-component suffixes], ...], "groups": [[module path, suffix set], ...]}: consecutive keys of one
    module path (all but the last two components: a Conv's `conv.weight` and five `bn.*` keys share one) become one group.  Lossless, order
    kept; a sixth of the size of the plain list."""
    suffixes, groups = [], []
    for k in keys:
        parts = k.split(".")
        n = 2 if len(parts) > 2 else 1
        path, suf = ".".join(parts[:-n]), ".".join(parts[-n:])
        if groups and groups[-1][0] == path:
            groups[-1][1].append(suf)
        else:
            groups.append([path, [suf]])
    for g in groups:
        if g[1] not in suffixes:
            suffixes.append(g[1])
        g[1] = suffixes.index(g[1])
    return {"suffixes": suffixes, "groups": groups}


def unpack_keys(packed):
    return [f"{path}.{suf}" if path else suf for path, i in packed["groups"] for suf in packed["suffixes"][i]]


def _rng(tag, seed=0):
    return np.random.default_rng([zlib.crc32(tag.encode()), seed])


def case_input(tag, shape):
    return torch.tensor(_rng(tag, 7).normal(0.0, 1.0, shape), dtype=torch.float32)


# ---- modules on small maps: (tag, class name, constructor args, constructor kwargs, input shape)
MODULE_CASES = [
    ("repconv", "RepConv", (16, 16), {}, (2, 16, 5, 7)),
    ("repconv_bn", "RepConv", (16, 16), {"bn": True}, (2, 16, 5, 7)),
    ("repncspelan4", "RepNCSPELAN4", (32, 48, 32, 16, 2), {}, (2, 32, 5, 7)),
    ("elan1", "ELAN1", (32, 32, 32, 16), {}, (1, 32, 6, 5)),
    ("repncspelan4_pad", "RepNCSPELAN4", (32, 40, 24, 12, 2), {}, (2, 32, 5, 7)),  # widths 12 and 6 (yolov9m has 180 / 90 / 60): zero-padded slots
    ("elan1_pad", "ELAN1", (32, 32, 24, 20), {}, (1, 32, 6, 5)),
    ("sppelan", "SPPELAN", (32, 48, 16), {}, (2, 32, 5, 7)),
    ("aconv", "AConv", (16, 32), {}, (2, 16, 7, 9)),
    ("adown", "ADown", (32, 32), {}, (2, 32, 9, 7)),
]
CBLINEAR_CASE = ("cblinear", (32, [8, 16, 24]), (1, 32, 5, 7))
# CBFuse: idx picks one slice of each tuple input; the last input is the target.  Shapes are those of each tuple's members.
CBFUSE_CASE = ("cbfuse", [1, 1], [[(1, 16, 2, 3), (1, 8, 2, 3)], [(1, 24, 5, 4), (1, 8, 5, 4)]], (1, 8, 9, 7))


def cbfuse_inputs():
    tag, idx, tuples, last = CBFUSE_CASE
    xs = [tuple(case_input(f"{tag}{i}_{j}", s) for j, s in enumerate(t)) for i, t in enumerate(tuples)]
    return xs + [case_input(tag + "_last", last)]


# ---- the model cases: tag -> (file, (B, H, W), weight gain).  yolov9e's main branch has residual RepBottlenecks on maps no BatchNorm has
# normalised (the CBFuse sums); at the usual gain its activations grow layer by layer into the thousands, so it gets a smaller one.
MODEL_CASES = {
    "yolov9t_64x96": ("yolov9t.yaml", (2, 64, 96), GAIN),
    "yolov9e_64": ("yolov9e.yaml", (2, 64, 64), 1.3),
    "yolov9c_seg_64x96": ("yolov9c-seg.yaml", (1, 64, 96), GAIN),
    "yolov9m_64x96": ("yolov9m.yaml", (1, 64, 96), GAIN),  # hidden widths 60 / 90 / 180: the zero-padded slots
}

# ---- ey_adown_pool shapes (tests/test_gpu_gelan_exact.py): (B, C, c_avg, H, W)
ADOWN_SHAPES = [(1, 16, 8, 2, 2), (2, 16, 8, 3, 5), (1, 32, 8, 8, 8), (2, 64, 32, 17, 33), (1, 16, 16, 9, 7)]
# ---- the nearest rule: (in, out) pairs checked against torch.nn.functional.interpolate
NEAREST_PAIRS = [(5, 9), (3, 9), (2, 9), (7, 13), (4, 13), (2, 13), (1, 9), (9, 9), (3, 36), (5, 36)]


def exact_input(tag, shape, half, negative=False):
    """fp32 values (f16-representable when half) ~ N(0, 1); negative: all below zero."""
    a = _rng(tag, 1).normal(0.0, 1.0, shape).astype(np.float32)
    if negative:
        a = -np.abs(a) - 0.125
    return a.astype(np.float16).astype(np.float32) if half else a
