"""Synthetic weights, inputs and cases for the obb task, shared by tests/golden/make_golden_obb.py and the tests.  Everything is drawn
from seeded generators keyed by a case tag, so the generator (which runs the reference) and the tests (which do not) build bit-identical
inputs; the NMS cases whose seed the generator had to search for (exact cases: every column margin > 1e-3) read the seed it stored."""
import zlib

import numpy as np
import torch

import synthdata as synth

GAIN = 1.9
NAME = "yolo11{}-obb.yaml"
SCALES = "nsmlx"
OBB_ARGS = ["nc", 1]  # the OBB row of yolo11-obb.yaml: [nc, ne]
MAX_WH = 7680.0
PI = float(np.pi)


def state_dict(own, gain=GAIN, prefix=""):
    return {k: synth.synth_tensor(prefix + k, tuple(v.shape) if hasattr(v, "shape") else tuple(v), gain=gain) for k, v in own.items()}


def edgeline_obb_cfg(load):
    """yolo11-test.yaml (EdgeLine) as a dict with its last row swapped to OBB."""
    d = dict(load)
    d["head"] = [list(r) for r in d["head"]]
    d["head"][-1] = [d["head"][-1][0], 1, "OBB", list(OBB_ARGS)]
    return d


def _rng(tag, seed=0):
    return np.random.default_rng([zlib.crc32(tag.encode()), seed])


# ---- the OBB head on small maps: (tag, constructor args, input shapes)
HEAD_CASE = ("obb_n", dict(nc=80, ne=1, ch=(64, 128, 256)), [(1, 64, 8, 12), (1, 128, 4, 6), (1, 256, 2, 3)])


def case_input(tag, shape):
    return torch.tensor(_rng(tag, 7).normal(0.0, 1.0, shape), dtype=torch.float32)


# ---- ey_obb_decode_levels: (tag, level maps (H, W), strides, nc, B, half, sliced)
DECODE_CASES = [
    ("dec_1x1_nc1_f32", [(1, 1)], [8.0], 1, 1, False, False),
    ("dec_3x5_nc3_b3_f16", [(3, 5)], [16.0], 3, 3, True, False),
    ("dec_3lv_nc80_f32", [(8, 12), (3, 5), (1, 1)], [8.0, 16.0, 32.0], 80, 1, False, False),
    ("dec_3lv_nc3_b3_f16_sliced", [(8, 12), (3, 5), (1, 1)], [8.0, 16.0, 32.0], 3, 3, True, True),
    ("dec_8x12_nc80_f16", [(8, 12)], [8.0], 80, 1, True, False),
    ("dec_3lv_nc1_b3_f32_sliced", [(8, 12), (3, 5), (1, 1)], [8.0, 16.0, 32.0], 1, 3, False, True),
]


def decode_case(tag, maps, strides, nc, B, half, sliced):
    """-> per level (box (B,64,H,W), cls (B,nc,H,W), angle (B,1,H,W)) fp32 NCHW logits (f16-representable when half)."""
    r = _rng(tag, 1)
    out = []
    for H, W in maps:
        lv = []
        for c, sd in ((64, 2.0), (nc, 2.5), (1, 2.0)):
            a = r.normal(0.0, sd, (B, c, H, W)).astype(np.float32)
            lv.append(torch.tensor(a.astype(np.float16).astype(np.float32) if half else a))
        out.append(tuple(lv))
    return out


# ---- scenes of rotated boxes: clusters of near-duplicates, as a detector emits them in front of NMS
def scene(r, n, clusters, imgsz=640.0):
    """-> (n,5) float32 xywhr; angles in [-pi/4, 3pi/4)."""
    k = max(1, int(clusters))
    cx, cy = r.uniform(0.05 * imgsz, 0.95 * imgsz, k), r.uniform(0.05 * imgsz, 0.95 * imgsz, k)
    w, h = r.lognormal(np.log(48.0), 0.5, k), r.lognormal(np.log(20.0), 0.5, k)
    t = r.uniform(-PI / 4, 3 * PI / 4, k)
    j = r.integers(0, k, n)
    b = np.stack([cx[j] + r.normal(0, 3.0, n), cy[j] + r.normal(0, 3.0, n), w[j] * np.exp(r.normal(0, 0.08, n)), h[j] * np.exp(r.normal(0, 0.08, n)),
                  t[j] + r.normal(0, 0.05, n)], 1)
    b[:, 4] = (b[:, 4] + PI / 4) % PI - PI / 4
    return b.astype(np.float32)


def _probiou_special(tag):
    f = np.float32
    if tag == "pi_identical":  # every box against itself and the others
        b = scene(_rng(tag), 9, 3)
        return b, b.copy()
    if tag == "pi_rot_pi":  # w != h: rotated by pi (the same Gaussian), and by pi/2 with w and h swapped
        a = np.array([[100, 120, 60, 20, 0.3], [300.5, 40.25, 15, 90, -0.6], [50, 50, 33, 7, 1.1]], f)
        b = a.copy()
        b[:, 4] += f(np.pi)
        c = a.copy()
        c[:, [2, 3]] = a[:, [3, 2]]
        c[:, 4] += f(np.pi / 2)
        return a, np.concatenate([b, c]).astype(f)
    if tag == "pi_zero_wh":  # degenerate boxes among ordinary ones
        a = scene(_rng(tag), 6, 2)
        a[1, 2:4] = 0
        a[4, 2:4] = 0
        b = a.copy()
        b[0, 2:4] = 0
        return a, b
    if tag == "pi_angle_ends":  # the ends of the head's angle range
        a = scene(_rng(tag), 8, 2)
        a[::2, 4] = f(-np.pi / 4)
        a[1::2, 4] = f(3 * np.pi / 4)
        b = scene(_rng(tag, 1), 5, 2)
        b[:2] = a[:2]
        b[2, 4] = f(3 * np.pi / 4)
        return a, b
    if tag == "pi_class_offset":  # centres as the NMS forms them: + 79 * 7680 in fp32
        a = scene(_rng(tag), 40, 4)
        b = scene(_rng(tag), 40, 4)[::-1].copy()
        b[:, :2] += _rng(tag, 2).normal(0, 1.5, (40, 2)).astype(f)
        off = f(79.0) * f(MAX_WH)
        a[:, :2] = a[:, :2] + off
        b[:, :2] = b[:, :2] + off
        return a, b
    raise KeyError(tag)


PROBIOU_SIZES = [(1, 1), (1, 130), (130, 1), (63, 65), (64, 64), (65, 63), (130, 130)]
PROBIOU_CASES = [f"pi_{n}x{m}" for n, m in PROBIOU_SIZES] + ["pi_identical", "pi_rot_pi", "pi_zero_wh", "pi_angle_ends", "pi_class_offset"]


def probiou_case(tag):
    """-> obb1 (N,5), obb2 (M,5) float32."""
    for n, m in PROBIOU_SIZES:
        if tag == f"pi_{n}x{m}":
            r = _rng(tag)
            both = scene(r, n + m, max(1, (n + m) // 8))  # one scene: boxes of the two sets share clusters
            p = r.permutation(n + m)
            return both[p[:n]], both[p[n:]]
    return _probiou_special(tag)


# ---- ey_nms_rotated cases.  `counts`: candidates per image (anchors beyond them score below conf); A = anchors per image.
# exact = the generator searches the seed until every column's fp64 margin |colmax - thr| exceeds 1e-3 (compared bit for bit).
def _nc(tag, counts, A, nc=3, conf=0.25, iou=0.45, **kw):
    d = dict(tag=tag, counts=list(counts), A=A, nc=nc, conf=conf, iou=iou, classes=None, agnostic=False, max_det=300, max_nms=30000, exact=False, special=None)
    d.update(kw)
    return d


NMS_CASES = [
    _nc("nms_n0", [0], 40),
    _nc("nms_n1", [1], 40),
    _nc("nms_n2", [2], 40, special="pair"),
    _nc("nms_n63", [63], 100, exact=True),
    _nc("nms_n64", [64], 100, iou=0.7),
    _nc("nms_n65", [65], 100, exact=True, max_det=20),  # max_det below the kept count
    _nc("nms_n129", [129], 200),
    _nc("nms_n257", [257], 300, iou=0.7),  # one past the 256-row chunk / 256-column tile of the pair kernel
    _nc("nms_n1100", [1100], 1300),  # beyond one 1024-thread workgroup
    _nc("nms_b3", [150, 0, 37], 200, exact=True),
    _nc("nms_agnostic_off", [12], 30, nc=2, special="twins"),
    _nc("nms_agnostic_on", [12], 30, nc=2, special="twins", agnostic=True),
    _nc("nms_classes", [120], 200, nc=4, classes=[1, 3]),
    _nc("nms_max_nms", [200], 260, max_nms=150),
    _nc("nms_ties", [90], 120, special="ties"),
    _nc("nms_iou0", [40], 60, iou=0.0),
    _nc("nms_iou1", [40], 60, iou=1.0),
]
NMS_BY_TAG = {c["tag"]: c for c in NMS_CASES}


def nms_case(case, seed=0):
    """-> pred (B, 4+nc+1, A) float32 tensor: clustered boxes, a best class per anchor, candidates = the first counts[b] anchors of a random
    permutation (the others score below conf)."""
    tag, nc, A, conf = case["tag"], case["nc"], case["A"], case["conf"]
    B = len(case["counts"])
    r = _rng(tag, seed)
    p = np.zeros((B, 4 + nc + 1, A), np.float32)
    for b, n in enumerate(case["counts"]):
        box = scene(r, A, max(1, A // 10))
        best = np.where(np.arange(A) < n, r.uniform(conf + 0.02, 0.98, A), r.uniform(0.0, max(conf - 0.02, 0.0), A))
        cls = r.integers(0, nc, A)
        if case["special"] == "pair":  # two candidates on top of each other
            box[1] = box[0]
            box[1, 0] += 0.5
            cls[1] = cls[0]
        if case["special"] == "twins":  # every even anchor has a copy of another class at the same place
            box[1::2] = box[0::2]
            cls[0::2], cls[1::2] = 0, 1
        if case["special"] == "ties":  # groups of equal scores
            best[:n] = np.round(best[:n] * 8) / 8 + 0.01
        perm = r.permutation(A)
        box, best, cls = box[perm], best[perm], cls[perm]
        sc = r.uniform(0.0, 0.5, (nc, A)) * best[None, :]
        sc[cls, np.arange(A)] = best
        p[b, :4] = box[:, :4].T
        p[b, 4:4 + nc] = sc
        p[b, 4 + nc] = box[:, 4]
    return torch.tensor(p)


# ---- tensor utilities
def rbox_vectors():
    """(n,5) xywhr rows for regularize_rboxes / xywhr2xyxyxyxy: w > h, w < h, w == h, angles on both sides of the range."""
    b = scene(_rng("rboxes"), 12, 4)
    b[3, 3] = b[3, 2]
    b[5, 4] = np.float32(-np.pi / 4)
    b[6, 4] = np.float32(3 * np.pi / 4 - 1e-3)
    b[7, [2, 3]] = b[7, [3, 2]]
    return torch.tensor(b)
