"""Synthetic weights, inputs and cases for the YOLOv3 / YOLOv5 / YOLOv6 tests, shared by tests/golden/make_golden_classic.py and the tests.
Everything is drawn from seeded generators keyed by a case tag, so the generator (which runs the reference) and the tests (which do not)
build bit-identical inputs."""
import numpy as np
import torch
import torch.nn as nn

import synthdata as synth
from v9_synth import case_input, exact_input, pack_keys, unpack_keys  # noqa: F401  (same input generator and key packing as the YOLOv9 goldens)
from v10_synth import separated_rows, state_dict  # noqa: F401  (the class-tower gain and the row rule of the YOLOv10 goldens)

GAIN = 1.9
# every file name the three families answer to: (requested name, file, scale)
V5_SCALES = "nsmlx"
V6_SCALES = "nsmlx"
NAMES = ([(f"yolov5{c}.yaml", "v5/yolov5.yaml", c) for c in V5_SCALES] + [(f"yolov5{c}-p6.yaml", "v5/yolov5-p6.yaml", c) for c in V5_SCALES]
         + [(f"yolov6{c}.yaml", "v6/yolov6.yaml", c) for c in V6_SCALES]
         + [("yolov3.yaml", "v3/yolov3.yaml", ""), ("yolov3-spp.yaml", "v3/yolov3-spp.yaml", ""), ("yolov3-tiny.yaml", "v3/yolov3-tiny.yaml", "")])
# the structure golden: parameter counts at nc = 80 as the reference reports them for its own files
PARAMS = {"yolov5n.yaml": 2654816, "yolov5x.yaml": 97276448, "yolov5n-p6.yaml": 4334896, "yolov3-tiny.yaml": 12173248, "yolov3.yaml": 103754144,
          "yolov3-spp.yaml": 104803744, "yolov6n.yaml": 4500080, "yolov6m.yaml": 52020496}
STRUCT_FILES = list(PARAMS)
STRIDES = {"yolov5n.yaml": [8.0, 16.0, 32.0], "yolov5x.yaml": [8.0, 16.0, 32.0], "yolov5n-p6.yaml": [8.0, 16.0, 32.0, 64.0], "yolov3-tiny.yaml": [16.0, 32.0],
           "yolov3.yaml": [8.0, 16.0, 32.0], "yolov3-spp.yaml": [8.0, 16.0, 32.0], "yolov6n.yaml": [8.0, 16.0, 32.0], "yolov6m.yaml": [8.0, 16.0, 32.0]}

# ---- modules on small odd maps: tag -> (input shape, all-negative input).  `make_module` builds each from a namespace of constructors, so that
# the generator passes the reference's (and torch's) classes and the tests pass this project's.
OPS_CASES = {
    "spp": ((2, 32, 7, 9), False),
    "bottleneck_row_n2": ((2, 32, 5, 7), False),   # the YAML row [-1, 2, Bottleneck, [32]] through parse_model: an nn.Sequential
    "zeropad_maxpool": ((2, 16, 6, 5), True),      # ZeroPad2d((0, 1, 0, 1)) + MaxPool2d(2, 1, 0) on an all-negative map: the border is 0
    "maxpool_s2": ((2, 16, 5, 7), False),          # MaxPool2d(2, 2, 0): the odd last row and column are dropped
    "deconv": ((2, 16, 5, 7), False),              # ConvTranspose2d(16, 24, 2, 2, 0) with bias
    "stem6": ((2, 3, 12, 20), False),              # Conv(3, 16, 6, 2, 2)
    "stem3s1": ((2, 3, 12, 20), False),            # Conv(3, 16, 3, 1)
}
ROW_DICT = {"nc": 80, "backbone": [[-1, 2, "Bottleneck", [32]]], "head": []}


def make_module(tag, ns):
    """ns: Conv, SPP, MaxPool2d, ZeroPad2d, ConvTranspose2d (classes) and parse (parse_model(dict, ch) -> (nn.Sequential, save))."""
    if tag == "spp":
        return ns["SPP"](32, 48)
    if tag == "bottleneck_row_n2":
        import copy
        return ns["parse"](copy.deepcopy(ROW_DICT), 32)[0]
    if tag == "zeropad_maxpool":
        return nn.Sequential(ns["ZeroPad2d"]([0, 1, 0, 1]), ns["MaxPool2d"](2, 1, 0))
    if tag == "maxpool_s2":
        return ns["MaxPool2d"](2, 2, 0)
    if tag == "deconv":
        return ns["ConvTranspose2d"](16, 24, 2, 2, 0)
    if tag == "stem6":
        return ns["Conv"](3, 16, 6, 2, 2)
    if tag == "stem3s1":
        return ns["Conv"](3, 16, 3, 1)
    raise KeyError(tag)


def ops_input(tag):
    shape, negative = OPS_CASES[tag]
    if negative:
        return torch.tensor(exact_input(tag, shape, half=False, negative=True))
    return case_input(tag, shape)


def prepare(m, tag):
    """eps as in a model (initialize_weights), seeded weights, eval mode."""
    for mod in m.modules():
        if isinstance(mod, nn.BatchNorm2d):
            mod.eps = 1e-3
    if len(m.state_dict()):
        m.load_state_dict(state_dict(m.state_dict(), prefix=tag + "."))
    return m.eval()


# ---- the model cases: tag -> (file or dict recipe, (B, H, W), weight gain, image seed, class-tower gain).  The full-width yolov3 files hold
# 415 MB of weights, too much for a test of a few seconds: they run at a quarter of the width, passed as a dict.
#  Gains and seeds were tried (gain 1.9 / 1.5 / 1.3 / 1.1, class gain 3 / 1.5 / 4, seeds 0-3, in that order) until the reference's kept rows
# met the row condition below; at gain 1.9 most of these models saturate their best scores to 1.0.
MODEL_CASES = {
    "yolov5n_64x96": ("yolov5n.yaml", (2, 64, 96), 1.3, 0, 3.0),
    "yolov5n-p6_64x128": ("yolov5n-p6.yaml", (1, 64, 128), 1.1, 0, 3.0),     # four levels, a 1x2 map at stride 64
    "yolov3-tiny_64x96": ("yolov3-tiny.yaml", (2, 64, 96), GAIN, 0, 3.0),    # two levels
    "yolov3_w025_64x96": ("yolov3.yaml", (1, 64, 96), 1.5, 2, 1.5),
    "yolov3-spp_w025_64x96": ("yolov3-spp.yaml", (1, 64, 96), 1.3, 3, 4.0),
    "yolov6n_64x96": ("yolov6n.yaml", (1, 64, 96), 1.5, 1, 1.5),             # ReLU
}
WIDTH = {"yolov3_w025_64x96": 0.25, "yolov3-spp_w025_64x96": 0.25}
NL = {"yolov5n_64x96": 3, "yolov5n-p6_64x128": 4, "yolov3-tiny_64x96": 2, "yolov3_w025_64x96": 3, "yolov3-spp_w025_64x96": 3, "yolov6n_64x96": 3}


def model_cfg(tag, load_yaml):
    """What to hand to DetectionModel / YOLO: the file name, or the file's dict with width_multiple overridden.  load_yaml(name) -> dict."""
    name = MODEL_CASES[tag][0]
    if tag not in WIDTH:
        return name
    d = load_yaml(name)
    d["width_multiple"] = WIDTH[tag]
    return d


def model_weights(tag, own):
    _, _, gain, _, cls_gain = MODEL_CASES[tag]
    return state_dict(own, gain=gain, cls_gain=cls_gain)


def model_images(tag):
    _, shape, _, seed, _ = MODEL_CASES[tag]
    return synth.synth_images(*shape, seed=seed)


ROW_GAP = 1e-3  # the generator asserts: the scores of the rows the reference's NMS keeps differ by more than this, and no candidate's best score is this close to conf
MIN_ROWS = 5


def kept_rows_separated(y_img, det, conf):
    """y_img (4 + nc, A): one image's decoded prediction; det (n, 6): the reference's NMS rows for it (score-descending).  -> (n, smallest gap
    between consecutive kept scores (v10_synth.separated_rows), distance of the nearest candidate score to conf)."""
    n, gap = separated_rows(np.asarray(det)[:, 4], conf)
    best = np.asarray(y_img, dtype=np.float64)[4:].max(0)
    return n, gap, float(np.abs(best - conf).min())
