"""Synthetic cases for obb validation, shared by tests/golden/make_golden_obbval.py and the tests: predictions for the multi-label rotated NMS
(ey_nms_rotated_ml) and operands for ey_probiou_batch.  Everything is drawn from seeded generators keyed by a case tag, so the generator
(which runs the reference) and the tests (which do not) build bit-identical inputs; the tests read the seed the generator stored."""
import numpy as np
import torch

import obb_synth

MAX_WH = obb_synth.MAX_WH
MARGIN = 1e-3  # every column's float64 |colmax - thr| of a golden NMS case exceeds this (make_golden_obb.py's MARGIN)
THRESHOLDS = np.linspace(0.5, 0.95, 10)
IOU_MARGIN = 1e-4  # every [gt x pred] ProbIoU of the validation case is further than this from each threshold


def grid_scene(r, n, clusters, pitch=72.0):
    """-> (n,5) float32 xywhr: clusters on a grid of `pitch` pixels, members that differ by a fraction of a pixel.  ProbIoU is then either
    close to 1 (same cluster) or close to 0 (another cluster), which keeps thousands of columns away from the threshold."""
    k = max(1, int(clusters))
    side = int(np.ceil(np.sqrt(k)))
    cx, cy = (np.arange(k) % side + 0.5) * pitch, (np.arange(k) // side + 0.5) * pitch
    w, h = r.uniform(28.0, 36.0, k), r.uniform(9.0, 14.0, k)
    t = r.uniform(-obb_synth.PI / 4, 3 * obb_synth.PI / 4, k)
    j = r.integers(0, k, n)
    b = np.stack([cx[j] + r.normal(0, 0.25, n), cy[j] + r.normal(0, 0.25, n), w[j] * np.exp(r.normal(0, 0.01, n)), h[j] * np.exp(r.normal(0, 0.01, n)),
                  t[j] + r.normal(0, 0.01, n)], 1)
    b[:, 4] = (b[:, 4] + obb_synth.PI / 4) % obb_synth.PI - obb_synth.PI / 4
    return b.astype(np.float32)


# ---- ey_nms_rotated_ml cases.  mode "hot": counts[b] anchors have a best class above conf and their other classes at a random fraction of
# it (some of them candidates too); "all": every (anchor, class) score is above conf; "flat": exactly counts[b] (anchor, class) scores are.
def _c(tag, counts, A, nc=3, mode="hot", conf=0.25, iou=0.45, **kw):
    d = dict(tag=tag, counts=list(counts), A=A, nc=nc, mode=mode, conf=conf, iou=iou, classes=None, agnostic=False, max_det=300, max_nms=30000, scene="clusters",
             triple=False)
    d.update(kw)
    return d


NMS_CASES = [
    _c("ml_few", [14], 64),
    _c("ml_all270", [90], 90, mode="all", conf=0.001, iou=0.7),  # 270 candidates: one past the 256-wide tile
    _c("ml_cut", [64], 64, nc=5, mode="all", max_nms=100),  # the cut falls inside an anchor's classes
    _c("ml_triple", [10], 64, triple=True),  # one anchor with all three classes above conf
    _c("ml_triple_agnostic", [10], 64, triple=True, agnostic=True),
    _c("ml_classes", [30], 64, nc=4, classes=[1, 3]),
    _c("ml_max_det5", [40], 64, max_det=5),
    _c("ml_nc1", [40], 64, nc=1),
    _c("ml_b3_empty", [25, 0, 9], 64),
    _c("ml_exact_max_nms", [150], 64, mode="flat", max_nms=150),
    _c("ml_max_nms_plus1", [151], 64, mode="flat", max_nms=150),
    _c("ml_large", [1200, 1200], 1200, nc=5, mode="all", conf=0.001, max_nms=4096, scene="grid"),  # the select over 6000 keys
]
NMS_BY_TAG = {c["tag"]: c for c in NMS_CASES}
TRIPLE_ANCHOR = 7


def nms_case(case, seed=0):
    """-> pred (B, 4+nc+1, A) float32 tensor."""
    tag, nc, A, conf = case["tag"], case["nc"], case["A"], case["conf"]
    B = len(case["counts"])
    r = obb_synth._rng(tag, seed)
    p = np.zeros((B, 4 + nc + 1, A), np.float32)
    for b, n in enumerate(case["counts"]):
        box = grid_scene(r, A, max(1, A // 12)) if case["scene"] == "grid" else obb_synth.scene(r, A, max(1, A // 10))
        box = box[r.permutation(A)]
        if case["mode"] == "all":
            sc = r.uniform(conf + 0.02, 0.98, (nc, A))
        elif case["mode"] == "flat":
            hot = np.zeros(nc * A, bool)
            hot[r.permutation(nc * A)[:n]] = True
            sc = np.where(hot.reshape(nc, A), r.uniform(conf + 0.02, 0.98, (nc, A)), r.uniform(0.0, conf - 0.02, (nc, A)))
        else:
            hot = np.zeros(A, bool)
            hot[r.permutation(A)[:n]] = True
            best = np.where(hot, r.uniform(conf + 0.02, 0.98, A), r.uniform(0.0, conf - 0.02, A))
            sc = r.uniform(0.0, 1.0, (nc, A)) * best[None, :]
            sc[r.integers(0, nc, A), np.arange(A)] = best
            if case["triple"] and n:
                sc[:, TRIPLE_ANCHOR] = r.uniform(conf + 0.05, 0.98, nc)
        p[b, :4] = box[:, :4].T
        p[b, 4:4 + nc] = sc
        p[b, 4 + nc] = box[:, 4]
    return torch.tensor(p)


# ---- ey_probiou_batch: (predictions, labels) per image
PAIR_SIZES = [(0, 3), (5, 0), (1, 1), (130, 65)]


def pair_case():
    """-> (pred (N_total,5), gt (M_total,5)) float32 arrays grouped by image in PAIR_SIZES order, and the two B+1 offset lists."""
    r = obb_synth._rng("probiou_batch")
    preds, gts = [], []
    for n, m in PAIR_SIZES:
        both = obb_synth.scene(r, n + m, max(1, (n + m) // 8))
        q = r.permutation(n + m)
        preds.append(both[q[:n]])
        gts.append(both[q[n:]])
    off = lambda parts: [0] + list(np.cumsum([len(t) for t in parts]))  # noqa: E731
    return np.concatenate(preds).astype(np.float32), np.concatenate(gts).astype(np.float32), off(preds), off(gts)
