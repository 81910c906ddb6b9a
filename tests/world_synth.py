"""Synthetic weights, inputs and text for the YOLO-World tests, shared by tests/golden/make_golden_world.py and the tests.  Everything is drawn
from seeded generators keyed by a case tag, so the generator (which runs the reference) and the tests (which do not) build bit-identical
inputs."""
import zlib

import numpy as np
import torch

import synthdata as synth

GAIN = 1.9
NAME = "yolov8{}-worldv2.yaml"
SCALES = "nsmlx"
EMBED = 512
N_PARAMS = 3695183  # yolov8n-worldv2 at nc=80


def state_dict(own, gain=GAIN, prefix=""):
    """Seeded tensors for every key of `own` but the text buffer (the build keeps `txt_feats` in state_dict, the reference does not)."""
    out = {}
    for k, v in own.items():
        if k == "txt_feats":
            continue
        shape = tuple(v.shape) if hasattr(v, "shape") else tuple(v)
        if k.endswith("gl.weight"):  # unit-variance rows: the projected guide of a unit-norm text is O(1) per channel, so the gates spread over (0, 1)
            out[k] = torch.tensor(_rng(prefix + k).normal(0.0, 1.0, shape), dtype=torch.float32)
        else:  # (the contrastive head's BatchNorm is called `norm`: same statistics rule as every `bn`)
            out[k] = synth.synth_tensor(prefix + k.replace(".norm.", ".bn."), shape, gain=gain)
    return out


def _rng(tag, seed=0):
    return np.random.default_rng([zlib.crc32(tag.encode()), seed])


def text(tag, n, embed=EMBED):
    """(n, embed) fp32 text embeddings, not normalised (set_classes normalises)."""
    return torch.tensor(_rng(tag, 3).normal(0.0, 1.0, (n, embed)), dtype=torch.float32)


def names(n):
    return [f"thing{i}" for i in range(n)]


def case_input(tag, shape):
    return torch.tensor(_rng(tag, 7).normal(0.0, 1.0, shape), dtype=torch.float32)


# ---- modules on small maps: (tag, constructor kwargs, input shape, texts)
ATTN_CASES = [
    ("msa_nh2", dict(c1=64, c2=64, nh=2, ec=64, gc=512, scale=False), (2, 64, 5, 7), 5),
    ("msa_nh3_scale", dict(c1=96, c2=96, nh=3, ec=96, gc=512, scale=True), (1, 96, 3, 4), 17),
]
C2FATTN_CASE = ("c2fattn", dict(c1=48, c2=64, n=2, ec=32, nh=1, gc=512), (2, 48, 5, 7), 5)
HEAD_CASE = ("world_head", dict(nc=80, embed=512, with_bn=True, ch=(64, 128, 256)), [(1, 64, 8, 12), (1, 128, 4, 6), (1, 256, 2, 3)], 7)

# ---- the model case: B = 2 at 64x96, a 5-text vocabulary set after construction; and the second vocabulary the predict test switches to
MODEL_TAG, MODEL_SHAPE, MODEL_TEXTS, OTHER_TEXTS = "yolov8n_worldv2_64x96", (2, 64, 96), 5, 9


def normalized(t):
    """what set_classes stores: rows divided by their L2 norm (reference tasks.py:650), shaped (1, n, embed)."""
    t = t.float()
    return (t / t.norm(p=2, dim=-1, keepdim=True)).reshape(1, -1, t.shape[-1])


# ---- ey_max_sigmoid_attn shapes (tests/test_gpu_world_exact.py): maps, heads, texts
MAPS = [(1, 1), (1, 9), (5, 7), (17, 33)]
HEADS = [1, 2, 3, 5, 10]
TEXTS = [1, 5, 15, 16, 17, 80, 257]


def attn_case(tag, B, H, W, nh, n, Bg, half):
    """-> e, p (B, C, H, W), g (Bg, n, C), bias (nh,), scale (nh,) fp32 (f16-representable when half).  Dots are O(1) after the division by
    sqrt(32): e ~ N(0, 1), g ~ N(0, 1)."""
    r = _rng(tag, 1)
    C = 32 * nh

    def t(shape, sd=1.0):
        a = r.normal(0.0, sd, shape).astype(np.float32)
        return torch.tensor(a.astype(np.float16).astype(np.float32) if half else a)

    return t((B, C, H, W)), t((B, C, H, W)), t((Bg, n, C)), t((nh,), 0.5), torch.tensor(r.uniform(0.5, 1.5, nh).astype(np.float32))
