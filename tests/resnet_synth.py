"""Synthetic weights, inputs and cases for the ResNet classifiers and the YOLOv8 task models, shared by tests/golden/make_golden_resnet.py and
the tests.  Everything is drawn from seeded generators keyed by tensor name or case tag, so the generator (which runs the reference) and the
tests (which do not) build bit-identical inputs and no weights are stored."""
import zlib

import numpy as np
import torch

import synthdata as synth

SCALES = "nsmlx"
V8_TASK_YAMLS = ("yolov8-cls.yaml", "yolov8-seg.yaml", "yolov8-seg-p6.yaml", "yolov8-pose.yaml", "yolov8-pose-p6.yaml", "yolov8-obb.yaml",
                 "yolov8-cls-resnet50.yaml", "yolov8-cls-resnet101.yaml")
TASK = {"cls": "classify", "seg": "segment", "pose": "pose", "obb": "obb"}


def scaled(name, scale):
    """'yolov8-seg-p6.yaml', 's' -> 'yolov8s-seg-p6.yaml'."""
    return name.replace("yolov8", "yolov8" + scale, 1)


def task_of(name):
    return TASK[name.split("-")[1].split(".")[0]]


def _rng(tag, seed=0):
    return np.random.default_rng([zlib.crc32(tag.encode()), seed])


def _f16(a):
    return a.astype(np.float16).astype(np.float32)


# ---- model weights.  A bottleneck block adds cv3's output to its input 16 (33) times in a row; with the gain of the detection models on every
# conv the sum would grow block by block.  The two convs that feed the sum (cv3 and the shortcut) get a smaller gain, which keeps the maps
# of all stages within one order of magnitude (the generator prints them).  The head's linear weights are scaled down so that the softmax of the
# all-positive pooled features is not saturated and the first six probabilities of a row are apart.
GAIN, GAIN_SUM, GAIN_LINEAR = 1.9, 0.15, 0.25
RESNET_NC = 80  # as the cls golden (tests/golden/make_golden_cls.py)
RESNET_SEED = {"yolov8n-cls-resnet50.yaml": 0, "yolov8n-cls-resnet101.yaml": 0}  # moved by the generator until the f16 ranking is decidable


def state_dict(own, seed=0):
    out = {}
    for k, v in own.items():
        gain = GAIN_SUM if (".cv3.conv." in k or ".shortcut." in k) and ".layer." in k else GAIN
        out[k] = synth.synth_tensor(k, tuple(v.shape), seed=seed, gain=gain)
        if k.endswith("linear.weight") and any(".layer." in q for q in own):
            out[k] = out[k] * GAIN_LINEAR
    return out


def f16_state_dict(sd):
    """the weights a half() model holds, as fp32 (for the generator's decidability run)."""
    return {k: (v.half().float() if v.is_floating_point() else v) for k, v in sd.items()}


RESNET_LAYER_SHAPE, RESNET_SHAPE = (2, 32, 32), (2, 64, 64)
VAL_NC, VAL_SHAPE, VAL_BATCHES = 10, (4, 64, 64), 2


def val_images(i):
    B, H, W = VAL_SHAPE
    return synth.synth_images(B, H, W, seed=40 + i)


# ---- the YOLOv8 task models: yaml -> (golden tag, (B, H, W))
V8_MODELS = {
    "yolov8n-cls.yaml": ("yolov8n_cls_64", (2, 64, 64)),
    "yolov8n-seg.yaml": ("yolov8n_seg_64", (2, 64, 64)),
    "yolov8n-pose.yaml": ("yolov8n_pose_64", (2, 64, 64)),
    "yolov8n-obb.yaml": ("yolov8n_obb_64", (2, 64, 64)),
    "yolov8n-seg-p6.yaml": ("yolov8n_seg_p6_128", (2, 128, 128)),
    "yolov8n-pose-p6.yaml": ("yolov8n_pose_p6_128", (2, 128, 128)),
}
V8_CONF = 0.05  # the confidence threshold of the predict checks (lowered per model by the generator where fewer than five rows survive)


# ---- ey_maxpool3x3s2: (tag, B, C, H, W)
POOL_CASES = [("mp_1x1", 1, 8, 1, 1), ("mp_6x5", 2, 16, 6, 5), ("mp_17x24", 2, 64, 17, 24)]


def pool_input(tag, shape, negative=False):
    x = _rng(tag, 1).normal(0.0, 1.0, shape).astype(np.float32)
    return -np.abs(x) - np.float32(0.25) if negative else x


# ---- the (7, 2, 3) stem and the block tails (ey_resnet_tail and the composed form): images and sizes
STEM_IMAGES = [(1, 1), (16, 16), (33, 47), (64, 72)]

# (tag, B, C1, C2, stride, H, W of x): C1 = 0 is the identity block (the block input is 4 C2 wide and is the residual).  The widest pair reads a
# 3x3 x at stride 2: its OUTPUT is the 2x2 map.
TAIL_CASES = [
    ("tail_id_c64_5x4", 3, 0, 64, 1, 5, 4),
    ("tail_p1_c64_1x1", 2, 64, 64, 1, 1, 1),
    ("tail_p1_c64_5x4", 2, 64, 64, 1, 5, 4),
    ("tail_p2_c256_9x7", 2, 256, 128, 2, 9, 7),
    ("tail_p2_c1024_3x3", 1, 1024, 512, 2, 3, 3),
]


def tail_case(tag, B, C1, C2, s, H, W, exact=False):
    """-> t (B, C2, Ho, Wo), x (B, C1 or 4 C2, H, W), W3 (4 C2, C2), Ws (4 C2, C1) or None, bias (4 C2,): float32 numpy, f16-representable
    activations and weights.  exact: small integers and multiples of 1/4, every sum exact in fp32 in any order."""
    r = _rng(tag, 5 if exact else 4)
    Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
    cx = C1 if C1 else 4 * C2
    if exact:
        t = r.integers(-2, 3, (B, C2, Ho, Wo)).astype(np.float32)
        x = r.integers(-2, 3, (B, cx, H, W)).astype(np.float32)
        w3 = (r.integers(-2, 3, (4 * C2, C2)) / 4.0).astype(np.float32)
        ws = (r.integers(-2, 3, (4 * C2, C1)) / 4.0).astype(np.float32) if C1 else None
        b = (r.integers(-8, 9, 4 * C2) / 4.0).astype(np.float32)
        return t, x, w3, ws, b
    t = _f16(r.normal(0.0, 1.0, (B, C2, Ho, Wo)).astype(np.float32))
    x = _f16(r.normal(0.0, 1.0, (B, cx, H, W)).astype(np.float32))
    l3 = (3.0 * GAIN_SUM / C2) ** 0.5
    w3 = _f16(r.uniform(-l3, l3, (4 * C2, C2)).astype(np.float32))
    ws = None
    if C1:
        ls = (3.0 * GAIN_SUM / C1) ** 0.5
        ws = _f16(r.uniform(-ls, ls, (4 * C2, C1)).astype(np.float32))
    b = r.normal(0.0, 0.1, 4 * C2).astype(np.float32)
    return t, x, w3, ws, b


# ---- ey_classify_pool above the 64 KiB tile: (tag, B, C1, H, W, Cout)
WIDE_POOL_CASES = [(f"cpw_c{c1}_{h}x{w}", 2, c1, h, w, 1280) for c1 in (2048, 2024) for h, w in ((1, 1), (2, 2), (7, 7))]
