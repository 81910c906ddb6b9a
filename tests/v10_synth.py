"""Synthetic weights, inputs and cases for the YOLOv10 tests, shared by tests/golden/make_golden_v10.py and the tests.  Everything is drawn
from seeded generators keyed by a case tag, so the generator (which runs the reference) and the tests (which do not) build bit-identical
inputs."""
import numpy as np

import synthdata as synth
from v9_synth import case_input, pack_keys, unpack_keys  # noqa: F401  (same input generator and key packing as the YOLOv9 goldens)

GAIN = 1.9
FILES = [f"yolov10{s}.yaml" for s in "nsmblx"]
PARAMS = {"yolov10n.yaml": 2775520, "yolov10x.yaml": 31808960}  # the reference's own files; the others: what the reference reports for its files


CLS_GAIN = 4.0


def state_dict(own, gain=GAIN, prefix="", cls_gain=CLS_GAIN):
    """Seeded tensors for every key of `own` (a state_dict, or {key: shape}).  The closing nn.Conv2d of every class tower (`cv3.i.2.weight`, both
    branches) gets cls_gain times the usual amplitude: with the usual one the class logits of a synthetic model sit within a few hundredths of
    their bias, and no confidence threshold separates the best rows by more than fp32 noise."""
    out = {}
    for k, v in own.items():
        t = synth.synth_tensor(prefix + k, tuple(v.shape) if hasattr(v, "shape") else tuple(v), gain=gain)
        parts = k.split(".")
        if len(parts) >= 4 and parts[-4].endswith("cv3") and parts[-2] == "2" and parts[-1] == "weight":
            t = t * cls_gain
        out[k] = t
    return out


# ---- modules on small maps: (tag, class name, constructor args, constructor kwargs, input shape)
MODULE_CASES = [
    ("scdown", "SCDown", (16, 32, 3, 2), {}, (2, 16, 9, 13)),          # odd map, all four borders
    ("scdown_k64", "SCDown", (16, 64, 3, 2), {}, (1, 16, 6, 8)),       # the narrowest width the fused f16 kernel takes (fp32 here: two launches)
    ("repvggdw", "RepVGGDW", (16,), {}, (2, 16, 7, 9)),
    ("cib", "CIB", (32, 32), {}, (2, 32, 6, 7)),                       # with the add
    ("cib_lk", "CIB", (32, 32), {"lk": True}, (2, 32, 6, 7)),
    ("cib_noadd", "CIB", (16, 32), {}, (2, 16, 6, 7)),                 # c1 != c2: no add
    ("cib_lk_noadd", "CIB", (32, 32, False), {"lk": True}, (1, 32, 5, 9)),
    ("c2fcib", "C2fCIB", (32, 32, 2, True, True), {}, (2, 32, 6, 7)),
    ("c2fcib_plain", "C2fCIB", (32, 48, 1, False), {}, (1, 32, 5, 6)),
    ("psa", "PSA", (128, 128), {}, (2, 128, 5, 6)),                    # c = 64: 1 head
    ("psa2", "PSA", (256, 256), {}, (1, 256, 4, 5)),                   # c = 128: 2 heads
]

# ---- the model cases: tag -> (file, (B, H, W), weight gain, image seed, class-tower gain); gains and seeds were tried until the reference's
# rows met the row-order condition below (yolov10x saturates every score to 1.0 at gain 1.9)
MODEL_CASES = {
    "yolov10n_64x96": ("yolov10n.yaml", (2, 64, 96), GAIN, 0, 4.0),   # SCDown x3, PSA (2 heads), C2fCIB with lk
    "yolov10x_64": ("yolov10x.yaml", (1, 64, 64), 1.7, 1, 8.0),       # C2fCIB without lk in the backbone, the 5-head PSA, the 320 / 640 widths
}


def model_weights(tag, own):
    _, _, gain, _, cls_gain = MODEL_CASES[tag]
    return state_dict(own, gain=gain, cls_gain=cls_gain)


def model_images(tag):
    _, shape, _, seed, _ = MODEL_CASES[tag]
    return synth.synth_images(*shape, seed=seed)

ROW_GAP = 1e-3  # the generator asserts: the reference's scores of the rows at or above `conf`, and the one after them, differ by more than this
MIN_ROWS = 5

# ---- ey_scdown shapes (tests/test_gpu_scdown.py): (B, H, W, C1, C2).  16 -> 32 is outside the gate (C2 % 64): the smallest widths it admits
SCDOWN_SHAPES = [(2, 9, 13, 16, 64), (1, 2, 2, 16, 64), (1, 1, 1, 16, 64), (2, 40, 24, 64, 128), (1, 6, 6, 320, 640), (1, 7, 5, 640, 640), (1, 33, 47, 128, 128)]


def separated_rows(scores, conf):
    """Number of leading rows (scores sorted descending) at or above conf; asserts nothing.  -> (n, smallest gap among rows 0..n)."""
    s = np.asarray(scores, dtype=np.float64)
    n = int((s >= conf).sum())
    head = s[:min(n + 1, len(s))]
    gap = float(np.min(-np.diff(head))) if len(head) > 1 else float("inf")
    return n, gap
