"""Synthetic weights for the LGL models (yolov13*-DSC3K2_LGL.yaml), shared by tests/golden/make_golden_v13_lgl.py and the tests.
synthdata.synth_tensor gives every key without '.bn.' in its name N(0, 0.1) statistics; the LGL block's BatchNorms and LayerNorms are
called norm / norm1 / norm2, so their running_var would come out negative (NaN in the reference) and their scales near zero, and its
nn.Linear weights (2-D) would ignore the fan-in.  The override below applies to keys of an LGL block (those containing '.lgl.', or all
keys with lgl=True for a block built on its own); every other key goes through synthdata unchanged."""
import numpy as np
import torch

import synthdata as synth

GAIN = 0.5  # the reference's fp32 forward stays within 1.2e-6 of its fp64 forward per layer at this gain; at 1.0 y is already 1.4e-3 off


def tensor(name, shape, gain=GAIN, lgl=None):
    shape = tuple(shape)
    if lgl is None:
        lgl = ".lgl." in name
    if lgl:
        parts = name.split(".")
        leaf, owner = parts[-1], (parts[-2] if len(parts) > 1 else "")
        r = synth._rng("lgl:" + name, 0)
        if leaf == "running_var" or (leaf == "weight" and owner in ("norm", "norm1", "norm2")):
            return torch.tensor(r.uniform(0.5, 1.5, shape), dtype=torch.float32)
        if leaf == "weight" and len(shape) == 2:
            b = (3.0 * gain / shape[1]) ** 0.5
            return torch.tensor(r.uniform(-b, b, shape), dtype=torch.float32)
        return synth.synth_tensor(name, shape, gain=0.5)
    return synth.synth_tensor(name, shape, gain=gain)


def state_dict(shapes, gain=GAIN):
    return {k: tensor(k, s, gain) for k, s in shapes.items()}


# module-level cases of v13_lgl_ops.npz: (tag, weight-name prefix, class, args, kwargs, input shape (B,C,H,W), all keys are LGL keys).
# Maps 6x10, 5x7 (both odd: partial pool windows, un-pool + bilinear), 1x1, 2x3, 9x16; batches 1 and 2.
_SA = dict(mlp_ratio=4.0, qkv_bias=True, sr_ratio=2)
_UNIT = (32, 3, 7, 1, True, None, 2, 4.0, 0.0, 0.0)
CASES = [
    ("localagg16_6x10", "localagg16", "LocalAgg", (16,), {}, (2, 16, 6, 10), True),
    ("localagg16_1x1", "localagg16", "LocalAgg", (16,), {}, (1, 16, 1, 1), True),
    ("localagg32_5x7", "localagg32", "LocalAgg", (32,), {}, (1, 32, 5, 7), True),
    ("localagg32_9x16", "localagg32", "LocalAgg", (32,), {}, (2, 32, 9, 16), True),
    ("selfattn16_6x10", "selfattn16", "SelfAttn", (16, 1), _SA, (2, 16, 6, 10), True),
    ("selfattn16_5x7", "selfattn16", "SelfAttn", (16, 1), _SA, (1, 16, 5, 7), True),
    ("selfattn32_5x7", "selfattn32", "SelfAttn", (32, 1), _SA, (1, 32, 5, 7), True),
    ("selfattn32_2x3", "selfattn32", "SelfAttn", (32, 1), _SA, (2, 32, 2, 3), True),
    ("selfattn64_9x16", "selfattn64", "SelfAttn", (64, 1), _SA, (1, 64, 9, 16), True),
    ("selfattn64_1x1", "selfattn64", "SelfAttn", (64, 1), _SA, (1, 64, 1, 1), True),
    ("selfattn128_5x7", "selfattn128", "SelfAttn", (128, 2), _SA, (2, 128, 5, 7), True),
    ("selfattn128_6x10", "selfattn128", "SelfAttn", (128, 2), _SA, (1, 128, 6, 10), True),
    ("selfattn128sr1_5x7", "selfattn128sr1", "SelfAttn", (128, 2), dict(_SA, sr_ratio=1), (2, 128, 5, 7), True),
    ("selfattn128sr1_9x16", "selfattn128sr1", "SelfAttn", (128, 2), dict(_SA, sr_ratio=1), (1, 128, 9, 16), True),
    ("lglblock32_5x7", "lglblock32", "LGLBlock", (32, 1), _SA, (2, 32, 5, 7), True),
    ("lglblock32_6x10", "lglblock32", "LGLBlock", (32, 1), _SA, (1, 32, 6, 10), True),
    ("unit32_9x16", "unit32", "_DSUnitWithLGL", _UNIT, {}, (1, 32, 9, 16), None),
    ("unit32_2x3", "unit32", "_DSUnitWithLGL", _UNIT, {}, (2, 32, 2, 3), None),
    ("dsc3k2lgl_32_64_6x10", "dsc3k2lgl_32_64", "DSC3K2_LGL", (32, 64, 1, False, 0.25), {}, (2, 32, 6, 10), None),
    ("dsc3k2lgl_32_64_5x7", "dsc3k2lgl_32_64", "DSC3K2_LGL", (32, 64, 1, False, 0.25), {}, (1, 32, 5, 7), None),
    ("dsc3k2lgl_64_64_9x16", "dsc3k2lgl_64_64", "DSC3K2_LGL", (64, 64, 2, True), {}, (1, 64, 9, 16), None),
    ("dsc3k2lgl_64_64_5x7", "dsc3k2lgl_64_64", "DSC3K2_LGL", (64, 64, 2, True), {}, (2, 64, 5, 7), None),
]


def fill(mod, prefix, lgl):
    """Load the synthetic weights of a module-level case (BatchNorm eps 1e-3 as initialize_weights sets it)."""
    mod.eval()
    for mm in mod.modules():
        if isinstance(mm, torch.nn.BatchNorm2d):
            mm.eps = 1e-3
    mod.load_state_dict({k: tensor(prefix + "." + k, tuple(v.shape), lgl=lgl) for k, v in mod.state_dict().items()})
    return mod


def case_input(shape):
    b, c, h, w = shape
    return synth.synth_images(b, h, w, c=c) * 2 - 1
