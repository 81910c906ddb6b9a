"""Synthetic masks and prompts for the FastSAM tests, shared by tests/golden/make_golden_fastsam.py and the tests: everything is
regenerated from seeds, so the fixtures hold results only.  A case is searched deterministically (seed 0, 1, ...) until the float64
restatement (tests/fp64_fastsam_ref.py) says its inputs are decidable: every box prompt's best and second-best IoU at least GAP apart
(the two tie cases duplicate a mask on purpose and are checked for an exact tie instead) and every point robust.  The generator asserts
the same conditions again on the reference's side."""
import zlib

import numpy as np

import fp64_fastsam_ref as f64

GAP = 2e-3  # searched with a margin over the 1e-3 the generator asserts

# tag: mask (mh, mw), originals per image, masks per image, P, Q, labels ("ones", "zeros", "mixed", "override"), duplicated mask pair or None
OP_CASES = {
    "same_64x96": ((64, 96), [(64, 96)], [12], 3, 5, "mixed", None),
    "batch3_64x96": ((64, 96), [(50, 75), (135, 240), (64, 96)], [12, 0, 1], 17, 5, "override", None),
    "crop_135x240": ((64, 96), [(135, 240)], [12], 3, 1, "ones", None),
    "odd_37x53": ((37, 53), [(50, 75), (37, 53)], [12, 12], 1, 5, "zeros", None),
    "sq32_97x13": ((32, 32), [(97, 13)], [12], 3, 0, "ones", None),
    "one_1x1": ((1, 1), [(1, 1)], [1], 1, 1, "ones", None),
    "points_50x75": ((64, 96), [(50, 75)], [12], 0, 5, "mixed", None),
    "tie_same_64x96": ((64, 96), [(64, 96)], [12], 1, 0, "ones", (3, 7)),
    "tie_odd_37x53": ((37, 53), [(50, 75)], [12], 1, 1, "ones", (2, 9)),
}
LABELS = {"ones": [1, 1, 1, 1, 1], "zeros": [0, 0, 0, 0, 0], "mixed": [1, 1, 0, 1, 0], "override": [1, 0, 1, 0, 1]}


def blobs(r, n, mask_hw, shape):
    """n uint8 masks [n, mh, mw]: one rectangle or ellipse each, inside the letterbox crop, of different sizes."""
    mh, mw = mask_hw
    top, bottom, left, right, _, _ = f64.geometry(mask_hw, shape)
    h, w = bottom - top, right - left
    m = np.zeros((n, mh, mw), np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    for k in range(n):
        ry, rx = max(0.5, h * (0.08 + 0.03 * k) * r.uniform(0.8, 1.2)), max(0.5, w * (0.06 + 0.035 * k) * r.uniform(0.8, 1.2))
        cy, cx = r.uniform(0, h), r.uniform(0, w)
        if k % 2:
            inside = ((yy + 0.5 - cy) / ry) ** 2 + ((xx + 0.5 - cx) / rx) ** 2 <= 1.0
        else:
            inside = (abs(yy + 0.5 - cy) <= ry) & (abs(xx + 0.5 - cx) <= rx)
        if not inside.any():
            inside[min(int(cy), h - 1), min(int(cx), w - 1)] = True
        m[k, top:bottom, left:right] = inside
    return m


def _box(r, kind, hmin, wmin):
    """kinds 0-3: full image, one pixel, touching two borders, reaching past the image; then anything."""
    if kind == 0:
        return [0, 0, wmin, hmin]
    if kind == 1:
        x, y = int(r.integers(0, wmin)), int(r.integers(0, hmin))
        return [x, y, x + 1, y + 1]
    x1, y1 = int(r.integers(0, max(1, wmin - 1))), int(r.integers(0, max(1, hmin - 1)))
    x2, y2 = int(r.integers(x1 + 1, wmin + 1)), int(r.integers(y1 + 1, hmin + 1))
    if kind == 2:
        return [0, y1, x2, hmin]
    if kind == 3:
        return [x1, y1, wmin + 7, hmin + 5]
    return [x1, y1, x2, y2]


def _try(tag, seed):
    mask_hw, shapes, counts, P, Q, lab, dup = OP_CASES[tag]
    r = np.random.default_rng([zlib.crc32(tag.encode()), seed])
    masks = [blobs(r, n, mask_hw, s) for n, s in zip(counts, shapes)]
    if dup:
        masks[0][dup[1]] = masks[0][dup[0]]
    hmin, wmin = min(s[0] for s in shapes), min(s[1] for s in shapes)
    boxes = []
    for p in range(P):
        for _ in range(60):
            b = _box(r, p % 5, hmin, wmin)
            if dup:  # the duplicated mask's own extent in the original image: the pair is the best, exactly tied
                ys, xs = np.nonzero(f64.scale_masks64(masks[0][dup[0]], shapes[0]) > 0.5)
                b = [int(xs.min()), int(ys.min()), int(xs.max()) + 1, int(ys.max()) + 1]
            ref = f64.prompt64(masks, shapes, [b])
            if dup:
                ok = ref[0]["best"][0] == dup[0] and ref[0]["iou"][0][dup[0]] == ref[0]["iou"][0][dup[1]] and np.sort(ref[0]["iou"][0])[-1] - np.sort(ref[0]["iou"][0])[-3] >= GAP
            else:
                ok = all(d is None or d["gap"][0] >= GAP for d in ref)
            if ok:
                boxes.append(b)
                break
            if p % 5 == 0 or dup:
                return None  # (the full-image box has no freedom: other masks)
        else:
            return None
    pts = []
    for q in range(Q):
        for _ in range(200):
            if q < 4 and len(masks[0]) > min(q // 2, len(masks[0]) - 1):  # inside a mask of the first image (points 0 and 1 share one), the last one anywhere
                ys, xs = np.nonzero(f64.scale_masks64(masks[0][min(q // 2, len(masks[0]) - 1)], shapes[0]) > 0.5)
                ok = (ys < hmin) & (xs < wmin)
                if not ok.any():
                    return None
                k = int(r.integers(0, int(ok.sum())))
                x, y = int(xs[ok][k]), int(ys[ok][k])
            else:
                x, y = int(r.integers(0, wmin)), int(r.integers(0, hmin))
            if all(f64.robust_point(m, s, x, y) for m, s in zip(masks, shapes)):
                pts.append([x, y])
                break
        else:
            return None
    return dict(tag=tag, seed=seed, mask_hw=mask_hw, shapes=shapes, counts=counts, masks=masks, boxes=np.array(boxes, np.int32).reshape(-1, 4),
                points=np.array(pts, np.int32).reshape(-1, 2), labels=np.array(LABELS[lab][:Q], np.int32), dup=dup)


_CACHE = {}


def op_case(tag):
    if tag not in _CACHE:
        for seed in range(200):
            c = _try(tag, seed)
            if c is not None:
                _CACHE[tag] = c
                break
        else:
            raise AssertionError(f"{tag}: no decidable case within 200 seeds")
    return _CACHE[tag]


# ---- scale_masks cases: (tag, input shape (N,C,H,W), target, padding)
SCALE_CASES = [("sm_96x160_270x480", (1, 3, 96, 160), (270, 480), True), ("sm_64x96_50x75", (2, 2, 64, 96), (50, 75), True),
               ("sm_32x32_97x13", (1, 4, 32, 32), (97, 13), True), ("sm_64x96_135x240", (1, 2, 64, 96), (135, 240), True),
               ("sm_37x53_same", (1, 2, 37, 53), (37, 53), True), ("sm_1x1", (1, 1, 1, 1), (1, 1), True), ("sm_37x53_nopad", (1, 2, 37, 53), (80, 60), False)]


def scale_input(tag, shape, kind):
    """kind "u8": 0/1 bytes; "f32" / "f16": gaussian values (f16: representable in half precision)."""
    r = np.random.default_rng([zlib.crc32(tag.encode()), 11])
    if kind == "u8":
        return (r.uniform(0, 1, shape) < 0.4).astype(np.uint8)
    a = r.normal(0, 1, shape).astype(np.float32)
    return a.astype(np.float16).astype(np.float32) if kind == "f16" else a


# ---- the model fixture: yolov8n-seg, nc = 1, B = 2 at 64 x 96.  With these synthetic weights NMS at the default 0.7 keeps several masks that cover
# the whole image (they tie under every box prompt); at 0.5 eight detections per image remain and box prompts with a clear winner exist
MODEL_YAML, MODEL_SHAPE, MODEL_CONF, MODEL_IOU = "yolov8n-seg.yaml", (2, 64, 96), 0.05, 0.5
