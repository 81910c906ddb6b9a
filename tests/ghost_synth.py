"""Synthetic weights, inputs and cases for the YOLOv8 / YOLOv8-ghost tests, shared by tests/golden/make_golden_ghost.py and the tests.
Everything is drawn from seeded generators keyed by a case tag, so the generator (which runs the reference) and the tests (which do not)
build bit-identical inputs."""
import numpy as np

import synthdata as synth
from v9_synth import case_input, pack_keys, unpack_keys  # noqa: F401  (same input generator and key packing as the YOLOv9 goldens)
from v10_synth import separated_rows, state_dict  # noqa: F401  (the class-tower gain and the row rule of the YOLOv10 goldens)

GAIN = 1.9
STEMS = ["yolov8{}.yaml", "yolov8{}-p2.yaml", "yolov8{}-p6.yaml", "yolov8{}-ghost.yaml", "yolov8{}-ghost-p2.yaml", "yolov8{}-ghost-p6.yaml"]
SCALES = "nsmlx"
FILES = [s.format(c) for s in STEMS for c in SCALES]
GHOST_FILES = [f for f in FILES if "ghost" in f]
# what the reference's own files say about themselves (the comments of its scale tables); every other count: what the reference reports for
# its files when the generator builds them
PARAMS = {"yolov8n.yaml": 3157200, "yolov8n-ghost.yaml": 1865316, "yolov8s-ghost.yaml": 5960072, "yolov8m-ghost.yaml": 10336312, "yolov8l-ghost.yaml": 14277872,
          "yolov8x-ghost.yaml": 22229308, "yolov8n-ghost-p2.yaml": 2033944, "yolov8s-ghost-p2.yaml": 5562080, "yolov8m-ghost-p2.yaml": 9031728,
          "yolov8l-ghost-p2.yaml": 12214448, "yolov8x-ghost-p2.yaml": 18664776, "yolov8n-ghost-p6.yaml": 2901100, "yolov8s-ghost-p6.yaml": 9520008,
          "yolov8m-ghost-p6.yaml": 18002904, "yolov8l-ghost-p6.yaml": 21227584, "yolov8x-ghost-p6.yaml": 33057852}
NL = {"": 3, "-p2": 4, "-p6": 4, "-ghost": 3, "-ghost-p2": 4, "-ghost-p6": 4}  # pyramid levels by file suffix

# hidden widths (half the output) of the 1x1 GhostConvs of yolov8{n,m,x}-ghost.yaml, as the reference builds them: multiples of 4 that are no
# multiples of 8 at all three scales.  The -p2 files have the same sets; the -p6 files add the 768-wide stage (24 and 48 at n).
HIDDEN = {"n": [4, 8, 16, 32, 64], "m": [12, 24, 48, 72, 96, 144], "x": [20, 40, 80, 160]}
HIDDEN_P6_N = [4, 8, 16, 24, 32, 48, 64]

# ---- modules on small odd maps: (tag, class name, constructor args, constructor kwargs, input shape)
MODULE_CASES = [
    ("ghostconv_h4", "GhostConv", (16, 8), {}, (2, 16, 7, 9)),            # hidden 4
    ("ghostconv_h12", "GhostConv", (48, 24), {}, (1, 48, 5, 7)),          # hidden 12
    ("ghostconv_noact", "GhostConv", (8, 16), {"act": False}, (2, 8, 9, 5)),
    ("ghostconv_k3s2", "GhostConv", (16, 32, 3, 2), {}, (2, 16, 9, 13)),  # the downsampling form, odd map
    ("ghostbottleneck", "GhostBottleneck", (16, 16), {}, (2, 16, 7, 9)),
    ("ghostbottleneck_s2", "GhostBottleneck", (16, 32, 3, 2), {}, (1, 16, 9, 7)),
    ("c3ghost", "C3Ghost", (32, 32, 2), {}, (2, 32, 5, 7)),
    ("c3ghost_noshortcut", "C3Ghost", (48, 32, 1, False), {}, (1, 48, 6, 5)),
    ("c2", "C2", (32, 48, 2, False), {}, (1, 32, 5, 6)),                  # the head block of yolov8-p6.yaml
]

# ---- the model cases: tag -> (file, (B, H, W), weight gain, image seed, class-tower gain); gains and seeds were tried until the reference's
# kept rows met the row condition below
MODEL_CASES = {
    "yolov8n-ghost_64x96": ("yolov8n-ghost.yaml", (2, 64, 96), GAIN, 1, 1.5),    # hidden 4 ... 128
    "yolov8x-ghost-p6_64": ("yolov8x-ghost-p6.yaml", (1, 64, 64), 1.3, 2, 4.0),   # hidden 20 ... 320, four levels, a 1x1 map at stride 64 (at gain 1.9 every score is 1.0)
    "yolov8n-p2_64": ("yolov8n-p2.yaml", (1, 64, 64), GAIN, 4, 3.0),             # the plain family, four levels
}


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


# ---- ey_ghost_conv shapes (tests/test_gpu_ghost_conv.py): (B, H, W, C1, Ch).  The kernel's largest tile is 16 x 16 output pixels, balanced
# over the map: 17 x 17 is one tile plus one pixel in each direction (four 9 x 9 tiles)
GHOST_SHAPES = [(1, 1, 1, 8, 4), (1, 2, 3, 16, 4), (2, 9, 13, 16, 8), (1, 17, 17, 24, 12), (1, 17, 17, 32, 64), (1, 5, 7, 40, 20), (1, 6, 6, 320, 320),
                (2, 40, 24, 64, 32)]
