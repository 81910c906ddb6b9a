"""Synthetic weights, inputs and cases for the pose task, shared by tests/golden/make_golden_pose.py and the tests.  Everything is drawn
from seeded generators keyed by a case tag, so the generator (which runs the reference) and the tests (which do not) build bit-identical
inputs; cases whose seed the generator had to search for (every OKS and box IoU further than 1e-4 from a threshold) read the seed it stored."""
import zlib

import numpy as np
import torch

import synthdata as synth

GAIN = 1.9
NAME = "yolo11{}-pose.yaml"
SCALES = "nsmlx"
KPT_SHAPE = [17, 3]
POSE_ARGS = ["nc", "kpt_shape"]  # the Pose row of yolo11-pose.yaml
OKS_SIGMA = np.array([0.26, 0.25, 0.25, 0.35, 0.35, 0.79, 0.79, 0.72, 0.72, 0.62, 0.62, 1.07, 1.07, 0.87, 0.87, 0.89, 0.89]) / 10.0
THRESHOLDS = np.linspace(0.5, 0.95, 10)
MARGIN = 1e-4


def state_dict(own, gain=GAIN, prefix=""):
    return {k: synth.synth_tensor(prefix + k, tuple(v.shape) if hasattr(v, "shape") else tuple(v), gain=gain) for k, v in own.items()}


def edgeline_pose_cfg(load, kpt_shape=(5, 2)):
    """yolo11-test.yaml (EdgeLine) as a dict with its last row swapped to Pose and the top-level kpt_shape key the row names."""
    d = dict(load)
    d["kpt_shape"] = list(kpt_shape)
    d["head"] = [list(r) for r in d["head"]]
    d["head"][-1] = [d["head"][-1][0], 1, "Pose", list(POSE_ARGS)]
    return d


def _rng(tag, seed=0):
    return np.random.default_rng([zlib.crc32(tag.encode()), seed])


# ---- the Pose head on small maps: (tag, constructor args, input shapes)
HEAD_CASE = ("pose_n", dict(nc=80, kpt_shape=(17, 3), ch=(64, 128, 256)), [(1, 64, 8, 12), (1, 128, 4, 6), (1, 256, 2, 3)])


def case_input(tag, shape):
    return torch.tensor(_rng(tag, 7).normal(0.0, 1.0, shape), dtype=torch.float32)


# ---- ey_kpts_decode_levels / ey_kpts_decode_rows: (tag, level maps (H, W), strides, kpt_shape, B, half, sliced)
# sliced: the maps are windows of wider NaN-filled buffers -- 16-byte aligned for f16 (vector loads), misaligned for f32 (scalar loads)
_L3, _S3 = [(4, 6), (2, 3), (1, 2)], [8.0, 16.0, 32.0]
DECODE_CASES = [
    ("kd_3lv_17x3_b1_f32_sliced", _L3, _S3, (17, 3), 1, False, True),
    ("kd_3lv_17x3_b2_f16_sliced", _L3, _S3, (17, 3), 2, True, True),
    ("kd_3lv_5x2_b2_f32_sliced", _L3, _S3, (5, 2), 2, False, True),
    ("kd_3lv_5x2_b1_f16_sliced", _L3, _S3, (5, 2), 1, True, True),
    ("kd_3lv_17x3_b2_f32", _L3, _S3, (17, 3), 2, False, False),
    ("kd_3lv_5x2_b2_f16", _L3, _S3, (5, 2), 2, True, False),
    ("kd_1x1_17x3_b1_f32", [(1, 1)], [32.0], (17, 3), 1, False, False),
    ("kd_1x1_5x2_b2_f16_sliced", [(1, 1)], [32.0], (5, 2), 2, True, True),
]
DECODE_BY_TAG = {c[0]: c for c in DECODE_CASES}


def decode_case(tag, maps, strides, kpt_shape, B, half, sliced):
    """-> per level keypoint logits (B, nk, H, W) fp32 NCHW (f16-representable when half)."""
    r = _rng(tag, 1)
    nk = kpt_shape[0] * kpt_shape[1]
    out = []
    for H, W in maps:
        a = r.normal(0.0, 2.0, (B, nk, H, W)).astype(np.float32)
        out.append(torch.tensor(a.astype(np.float16).astype(np.float32) if half else a))
    return out


def rows_index(maps, B, max_det):
    """-> (index (B, max_det) int32, count (B,) int32) for ey_kpts_decode_rows: the first and last anchor of every level, anchors of all
    levels mixed, -1 entries inside the count; image 0 is full or nearly so, the last image of a batch has count 0, others count < max_det."""
    sizes = [h * w for h, w in maps]
    offs = np.concatenate([[0], np.cumsum(sizes)])
    A = int(offs[-1])
    ends = [int(v) for l in range(len(maps)) for v in (offs[l], offs[l + 1] - 1)]
    r = _rng(f"rows{A}_{B}_{max_det}")
    count = np.array([(max_det if B > 1 else max(1, max_det - 1)) if b == 0 else (0 if b == B - 1 else max(1, max_det // 2)) for b in range(B)], np.int32)
    index = r.integers(0, A, (B, max_det)).astype(np.int32)  # (beyond the count: stale anchors, which the kernel must not decode)
    for b in range(B):
        n = int(count[b])
        live = ends + [-1] + [int(v) for v in r.integers(0, A, max(n - len(ends) - 1, 0))] if n > len(ends) else ends[:n]
        index[b, :n] = np.array(live, np.int32)[r.permutation(len(live))] if n > 1 else live
    return index, count


# ---- ey_kpt_iou cases
def people(r, m, K, imgsz=640.0):
    """-> gt (m, K, 3) keypoints with visibility 0 / 1 / 2, boxes (m, 4) xyxy around them."""
    cx, cy = r.uniform(0.2 * imgsz, 0.8 * imgsz, m), r.uniform(0.2 * imgsz, 0.8 * imgsz, m)
    w, h = r.uniform(30, 160, m), r.uniform(60, 300, m)
    g = np.zeros((m, K, 3), np.float32)
    g[..., 0] = cx[:, None] + r.uniform(-0.5, 0.5, (m, K)) * w[:, None]
    g[..., 1] = cy[:, None] + r.uniform(-0.5, 0.5, (m, K)) * h[:, None]
    g[..., 2] = r.choice([0.0, 1.0, 2.0], (m, K), p=[0.2, 0.3, 0.5])
    box = np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], 1).astype(np.float32)
    return g, box


def guesses(r, g, box, n, ndim):
    """n predictions spread around the ground truths: noise of 1 to 25 % of the box size."""
    m, K = g.shape[:2]
    j = r.integers(0, m, n)
    size = np.sqrt((box[j, 2] - box[j, 0]) * (box[j, 3] - box[j, 1]))
    p = np.zeros((n, K, ndim), np.float32)
    p[..., :2] = g[j, :, :2] + r.normal(0, 1, (n, K, 2)) * (size * r.uniform(0.01, 0.25, n))[:, None, None]
    if ndim == 3:
        p[..., 2] = r.uniform(0, 1, (n, K))
    return p


def _area(box):
    return ((box[:, 2] - box[:, 0]) * (box[:, 3] - box[:, 1]) * np.float32(0.53)).astype(np.float32)


OKS_SIZES = [(1, 1), (7, 40), (3, 65)]
OKS_CASES = [f"oks_{m}x{n}" for m, n in OKS_SIZES] + ["oks_k5_ndim2", "oks_novis", "oks_identical", "oks_area0"]


def oks_case(tag):
    """-> gt (M,K,3), pred (N,K,ndim), area (M,), sigma (K,) float32."""
    r = _rng(tag)
    sig17 = OKS_SIGMA.astype(np.float32)
    for m, n in OKS_SIZES:
        if tag == f"oks_{m}x{n}":
            g, box = people(r, m, 17)
            return g, guesses(r, g, box, n, 3), _area(box), sig17
    if tag == "oks_k5_ndim2":  # uniform sigma, predictions without the confidence entry
        g, box = people(r, 4, 5)
        return g, guesses(r, g, box, 9, 2), _area(box), (np.ones(5) / 5).astype(np.float32)
    if tag == "oks_novis":  # ground truths 0 and 2 have no visible keypoint: exactly 0
        g, box = people(r, 3, 17)
        g[0, :, 2] = 0
        g[2, :, 2] = 0
        return g, guesses(r, g, box, 6, 3), _area(box), sig17
    if tag == "oks_identical":  # every prediction equals a ground truth
        g, box = people(r, 5, 17)
        g[:, 0, 2] = 2
        return g, g.copy(), _area(box), sig17
    if tag == "oks_area0":  # area 0: d == 0 (prediction 0 = ground truth 0) and d > 0
        g, box = people(r, 2, 17)
        g[:, :, 2] = 1
        p = guesses(r, g, box, 4, 3)
        p[0, :, :2] = g[0, :, :2]
        a = _area(box)
        a[0] = 0
        return g, p, a, sig17
    raise KeyError(tag)


def oks_batch():
    """three images: (7 gt x 40 pred), no ground truth (0 x 5), no prediction (3 x 0) -> list of (gt, pred, area), sigma."""
    g0, p0, a0, sg = oks_case("oks_7x40")
    r = _rng("oks_batch")
    g1, b1 = people(r, 2, 17)
    p1 = guesses(r, g1, b1, 5, 3)
    g2, b2 = people(r, 3, 17)
    return [(g0, p0, a0), (g1[:0], p1, _area(b1)[:0]), (g2, p0[:0], _area(b2))], sg


# ---- tensor utilities
def coords_vectors():
    """(n, K, 3) keypoints in a 96 x 128 network frame: inside, outside on every side, confidences on both sides of 0.5."""
    r = _rng("coords")
    c = np.zeros((6, 5, 3), np.float32)
    c[..., 0] = r.uniform(-20, 150, (6, 5))
    c[..., 1] = r.uniform(-20, 120, (6, 5))
    c[..., 2] = r.uniform(0, 1, (6, 5))
    c[0, 0, 2], c[0, 1, 2] = 0.5, np.float32(0.49999997)
    return torch.tensor(c)


COORDS_IMG1 = (96, 128)
COORDS_CASES = [  # (tag, img0_shape, ratio_pad, normalize, padding)
    ("sc_same", (96, 128), None, False, True),
    ("sc_letterbox", (300, 480), None, False, True),
    ("sc_ratio_pad", (200, 240), ((0.5, 0.5), (4.0, 0.0)), False, True),
    ("sc_normalize", (300, 480), None, True, True),
    ("sc_nopad", (300, 480), None, False, False),
    ("sc_tall", (480, 300, 3), None, False, True),
]


# ---- the end-to-end validation case (tests/golden/poseval_case.npz): the batch dict the validators take
def poseval_batch(g, img=None, wrap=np.asarray):
    B, H, W = (int(v) for v in g["image_shape"])
    if img is None:
        img = torch.zeros((B, 3, H, W))
    return {"img": img, "cls": wrap(g["cls"]), "bboxes": wrap(g["bboxes"]), "batch_idx": wrap(g["batch_idx"]), "keypoints": wrap(g["keypoints"]),
            "ori_shape": [tuple(int(v) for v in s) for s in g["ori_shape"]],
            "ratio_pad": [((float(a), float(a)), (int(p[0]), int(p[1]))) for a, p in zip(g["ratio_gain"], g["ratio_padwh"])]}


def poseval_images(g):
    B, H, W = (int(v) for v in g["image_shape"])
    return synth.synth_images(B, H, W, seed=int(g["image_seed"]))
