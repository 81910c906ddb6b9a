"""Seeded cases for the validation matching (ey_match_batch, utils.metrics.ConfusionMatrix / match_batch), shared by the golden generator
(tests/golden/make_golden_confusion.py) and the tests.  A case is one image: detections that are jittered copies of labels plus strays, with
right and wrong classes and confidences on both sides of 0.25, in the network-input frame; labels in original-image pixels.  `case(spec,
seed)` is deterministic; the generator redraws with the next seed until `violations(case)` is empty and records the seed that it used."""
import numpy as np

IOUV = np.linspace(0.5, 0.95, 10)
CM_CONF, CM_IOU = 0.25, 0.45
IMGSZ = (160, 192)

# (name, detections, labels, nc, letterbox): every count of the issue appears on each side, with the three empty pairs
SPECS = [
    ("d0_g0", 0, 0, 3, False), ("d0_g3", 0, 3, 3, False), ("d5_g0", 5, 0, 3, True), ("d1_g1", 1, 1, 1, False), ("d5_g3", 5, 3, 3, True),
    ("d63_g63", 63, 63, 80, False), ("d64_g64", 64, 64, 80, True), ("d65_g65", 65, 65, 3, False), ("d255_g70", 255, 70, 80, True),
    ("d256_g257", 256, 257, 80, False), ("d257_g64", 257, 64, 1, True), ("d300_g257", 300, 257, 3, True), ("d300_g70", 300, 70, 80, False),
    ("d300_g1", 300, 1, 1, False), ("d1_g65", 1, 65, 3, True), ("d63_g3", 63, 3, 1, True), ("d300_g0", 300, 0, 80, False), ("d0_g257", 0, 257, 80, True),
]
OBB_SPECS = [("obb_d5_g3", 5, 3, 3), ("obb_d65_g64", 65, 64, 15), ("obb_d0_g3", 0, 3, 3), ("obb_d5_g0", 5, 0, 3), ("obb_d300_g70", 300, 70, 15)]
CLS_SPEC = ("cls", 257, 7)  # samples, classes


def box_iou(a, b):
    """(N,4) x (M,4) -> (N,M) fp32, the expression of the reference's box_iou."""
    a, b = np.asarray(a, np.float32)[:, None], np.asarray(b, np.float32)[None]
    wh = np.clip(np.minimum(a[..., 2:], b[..., 2:]) - np.maximum(a[..., :2], b[..., :2]), 0, None)
    inter = wh[..., 0] * wh[..., 1]
    return inter / ((a[..., 2] - a[..., 0]) * (a[..., 3] - a[..., 1]) + (b[..., 2] - b[..., 0]) * (b[..., 3] - b[..., 1]) - inter + np.float32(1e-7))


def geometry(letterbox):
    """-> (ori_shape, ratio_pad): with a letterbox the original is larger and of another aspect than the input, so gain and pads matter."""
    if not letterbox:
        return IMGSZ, None
    ori = (300, 500)
    gain = min(IMGSZ[0] / ori[0], IMGSZ[1] / ori[1])
    pad = ((IMGSZ[1] - ori[1] * gain) / 2, (IMGSZ[0] - ori[0] * gain) / 2)
    return ori, ((gain, gain), pad)


def xform_row(ori, ratio_pad):
    """padx, pady, gain, w0, h0 of ey_match_batch; without ratio_pad the same numbers ops.scale_boxes derives."""
    if ratio_pad is None:
        gain = min(IMGSZ[0] / ori[0], IMGSZ[1] / ori[1])
        pad = (round((IMGSZ[1] - ori[1] * gain) / 2 - 0.1), round((IMGSZ[0] - ori[0] * gain) / 2 - 0.1))
    else:
        gain, pad = ratio_pad[0][0], ratio_pad[1]
    return np.array([pad[0], pad[1], gain, ori[1], ori[0]], np.float32)


def scale_boxes(det, ori, ratio_pad):
    """ops.scale_boxes + clip_boxes in numpy fp32: (v - pad) / gain, clamp."""
    x = xform_row(ori, ratio_pad)
    out = np.array(det, np.float32, copy=True)
    out[:, [0, 2]] = np.clip((out[:, [0, 2]] - x[0]) / x[2], np.float32(0), x[3])
    out[:, [1, 3]] = np.clip((out[:, [1, 3]] - x[1]) / x[2], np.float32(0), x[4])
    return out


def _draw(rng, nd, ng, nc, ori, obb=False):
    h, w = ori
    cx, cy = rng.uniform(0.1 * w, 0.9 * w, ng), rng.uniform(0.1 * h, 0.9 * h, ng)
    bw, bh = rng.uniform(0.06 * w, 0.3 * w, ng), rng.uniform(0.06 * h, 0.3 * h, ng)
    gcls = rng.integers(0, nc, ng)
    g = np.stack([cx, cy, bw, bh], 1)
    d = np.zeros((nd, 4))
    dcls = rng.integers(0, nc, nd)
    src = np.full(nd, -1)
    for i in range(nd):
        if ng and rng.random() < 0.75:  # a jittered copy of a label: mostly the right class
            k = int(rng.integers(0, ng))
            src[i] = k
            s = rng.choice([0.03, 0.1, 0.25])
            d[i] = g[k] * (1 + rng.normal(0, s, 4) * [0.3, 0.3, 1, 1])
            d[i, 2:] = np.abs(d[i, 2:]) + 1
            if rng.random() < 0.8:
                dcls[i] = gcls[k]
        else:  # a stray
            d[i] = [rng.uniform(0, w), rng.uniform(0, h), rng.uniform(0.05 * w, 0.3 * w), rng.uniform(0.05 * h, 0.3 * h)]
    conf = np.where(rng.random(nd) < 0.6, rng.uniform(0.3, 0.99, nd), rng.uniform(0.002, 0.2, nd))
    if obb:
        ga, da = rng.uniform(-0.7, 0.7, ng), np.where(src >= 0, 0, rng.uniform(-0.7, 0.7, nd))
        da = da + np.where(src >= 0, ga[np.maximum(src, 0)] if ng else 0, 0) + rng.normal(0, 0.05, nd) * (src >= 0)
        return g, ga, gcls, d, da, dcls, conf
    xyxy = lambda b: np.stack([b[:, 0] - b[:, 2] / 2, b[:, 1] - b[:, 3] / 2, b[:, 0] + b[:, 2] / 2, b[:, 1] + b[:, 3] / 2], 1)  # noqa: E731
    return xyxy(g), gcls, xyxy(d), dcls, conf


def case(spec, seed):
    """-> dict(name, nc, det (n,6) fp32 in the input frame, gt (m,4) fp32 xyxy in original pixels, gt_cls (m,) fp32, ori_shape, ratio_pad)."""
    name, nd, ng, nc, letterbox = spec
    rng = np.random.default_rng(seed)
    ori, ratio_pad = geometry(letterbox)
    g, gcls, d, dcls, conf = _draw(rng, nd, ng, nc, ori)
    g = np.clip(g, 0, [ori[1], ori[0]] * 2).astype(np.float32)
    x = xform_row(ori, ratio_pad).astype(np.float64)
    d = d * x[2] + [x[0], x[1]] * 2  # original pixels -> the input frame
    det = np.concatenate([d, conf[:, None], dcls[:, None]], 1).astype(np.float32).reshape(nd, 6)
    return dict(name=name, nc=nc, det=det, gt=g.reshape(ng, 4), gt_cls=gcls.astype(np.float32), ori_shape=ori, ratio_pad=ratio_pad)


def obb_case(spec, seed):
    """-> dict(name, nc, det (n,7) fp32 x,y,w,h,conf,cls,angle, gt (m,5) fp32 xywhr, gt_cls (m,) fp32), all in one frame."""
    name, nd, ng, nc = spec
    rng = np.random.default_rng(seed)
    g, ga, gcls, d, da, dcls, conf = _draw(rng, nd, ng, nc, IMGSZ, obb=True)
    det = np.concatenate([d, conf[:, None], dcls[:, None], da[:, None]], 1).astype(np.float32).reshape(nd, 7)
    gt = np.concatenate([g, ga[:, None]], 1).astype(np.float32).reshape(ng, 5)
    return dict(name=name, nc=nc, det=det, gt=gt, gt_cls=gcls.astype(np.float32))


def cls_case(seed):
    """-> (top-5 classes (n, 5) int32, best first, targets (n,) int32, nc)."""
    _, n, nc = CLS_SPEC
    rng = np.random.default_rng(seed)
    top = np.stack([rng.permutation(nc)[:5] for _ in range(n)]).astype(np.int32)
    tgt = np.where(rng.random(n) < 0.6, top[:, 0], rng.integers(0, nc, n)).astype(np.int32)
    return top, tgt, nc


def violations(iou, det, gt_cls):
    """What would make a case's expected result depend on a tie-break or on the last bits of an IoU.  iou: (m, n) fp32 of the case in the
    labels' frame.  -> list of strings, empty when the case is clean:
      - a candidate IoU within 2^-18 relative of a threshold (the ten of IOUV, and the matrix's 0.45);
      - a confidence within 1e-6 of 0.25;
      - an exact tie among the candidates (IoU > 0.45, or IoU >= 0.5 with equal classes) of a detection or of a label."""
    bad = []
    iou = np.asarray(iou, np.float64)
    for thr in list(IOUV) + [CM_IOU]:
        if iou.size and (np.abs(iou - thr) <= thr * 2.0 ** -18).any():
            bad.append(f"an IoU within 2^-18 of {thr}")
    if len(det) and (np.abs(det[:, 4].astype(np.float64) - CM_CONF) <= 1e-6).any():
        bad.append("a confidence within 1e-6 of 0.25")
    if iou.size:
        same = np.asarray(gt_cls)[:, None] == det[None, :, 5]
        for cand in (np.where(iou > 0.45 - 1e-3, iou, -1.0), np.where((iou >= 0.5 - 1e-3) & same, iou, -1.0)):
            for axis in (0, 1):
                s = np.sort(cand, axis=axis)
                eq = np.diff(s, axis=axis) == 0
                live = (s[1:] if axis == 0 else s[:, 1:]) >= 0
                if (eq & live).any():
                    bad.append(f"an exact IoU tie along axis {axis}")
    return bad


_CACHE = {}


def golden_cases(golden_dir):
    """The committed cases with their recorded reference results, computed once and shared (callers must not modify them):
    -> (boxes, obbs, cls): boxes / obbs are lists of the case dicts plus `predn` (the rows in the labels' frame; for obb the rows themselves),
    `matrix` (int64) and `tp` (bool (n, 10)); cls = (top5, targets, nc, matrix)."""
    import os
    if golden_dir not in _CACHE:
        z = np.load(os.path.join(golden_dir, "confusion_cases.npz"))
        assert int(z["skipped"]) == 0
        boxes, obbs = [], []
        for spec in SPECS:
            c = case(spec, int(z[spec[0] + "_seed"]))
            c["predn"] = scale_boxes(c["det"], c["ori_shape"], c["ratio_pad"]) if len(c["det"]) else c["det"].copy()
            c["matrix"], c["tp"] = z[spec[0] + "_matrix"], z[spec[0] + "_tp"]
            boxes.append(c)
        for spec in OBB_SPECS:
            c = obb_case(spec, int(z[spec[0] + "_seed"]))
            c["predn"], c["matrix"], c["tp"] = c["det"], z[spec[0] + "_matrix"], z[spec[0] + "_tp"]
            obbs.append(c)
        _CACHE[golden_dir] = (boxes, obbs, cls_case(int(z["cls_seed"])) + (z["cls_matrix"],))
    return _CACHE[golden_dir]
