"""float64 restatement of FastSAM's prompt selection (reference ultralytics/models/fastsam/predict.py:61-103) and of scale_masks
(utils/ops.py:716-737), numpy only, shared by tests/golden/make_golden_fastsam.py, the CPU tests and the GPU tests.

The per-axis source indices and weights are fp32 VALUES, torch's CPU operator's (compute_source_index_and_lambda with float opmath, the
source coordinate as ONE fused multiply-add); everything after them -- the resize, the sums over boxes, the IoU -- is float64.  So the
restatement differs from the reference's resize-and-sum only by the reference's own fp32 rounding, and from ey_mask_prompt only by the
kernel's fp32 summation, for which `area_bound` states the bound from the kernel's summation order (csrc/fastsam.hip)."""
import numpy as np

U = 2.0 ** -24  # unit roundoff of fp32


def geometry(mask_hw, shape, padding=True):
    """(top, bottom, left, right, H0, W0): the crop of scale_masks (ops.py:726-733) and the target.  padding=False keeps the top-left
    corner and cuts the WHOLE padding off the bottom and the right, as the reference does."""
    mh, mw = int(mask_hw[0]), int(mask_hw[1])
    h0, w0 = int(shape[0]), int(shape[1])
    gain = min(mh / h0, mw / w0)
    pad = [mw - w0 * gain, mh - h0 * gain]
    if padding:
        pad[0] /= 2
        pad[1] /= 2
    top, left = (int(pad[1]), int(pad[0])) if padding else (0, 0)
    return top, int(mh - pad[1]), left, int(mw - pad[0]), h0, w0


def axis_map(n_in, n_out):
    """-> i0, i1 (int64 [n_out]), l0, l1 (float32 [n_out]) of F.interpolate(mode="bilinear", align_corners=False) along one axis."""
    y = np.arange(n_out)
    if n_in == n_out:
        return y.copy(), y.copy(), np.ones(n_out, np.float32), np.zeros(n_out, np.float32)
    f = np.float32
    scale = f(n_in) / f(n_out)
    # fmaf(scale, y + 0.5, -0.5): the product of two fp32 values is exact in float64, and so is the difference wherever it is not negative
    r = (np.float64(scale) * (y.astype(f) + f(0.5)).astype(np.float64) - 0.5).astype(f)
    r = np.where(r < 0, f(0), r).astype(f)
    i0 = np.minimum(np.floor(r).astype(np.int64), n_in - 1)
    l1 = np.clip(r - i0.astype(f), f(0), f(1)).astype(f)
    i1 = i0 + (i0 < n_in - 1)
    return i0, i1, (f(1) - l1).astype(f), l1


def axis_matrix(n_in, n_out):
    """float64 [n_out][n_in]: row y holds l0 at i0 and l1 at i1 (added where they coincide)."""
    i0, i1, l0, l1 = axis_map(n_in, n_out)
    a = np.zeros((n_out, n_in))
    np.add.at(a, (np.arange(n_out), i0), l0.astype(np.float64))
    np.add.at(a, (np.arange(n_out), i1), l1.astype(np.float64))
    return a


def axis_terms(n_in, n_out):
    """The most weights any one source index collects from the whole target axis: the longest chain of a box weight's sum."""
    i0, i1, l0, l1 = axis_map(n_in, n_out)
    return int((np.bincount(i0, minlength=n_in) + np.bincount(i1, minlength=n_in)).max())


def scale_masks64(masks, shape, padding=True):
    """masks [..., H, W] -> float64 [..., H0, W0]."""
    m = np.asarray(masks, np.float64)
    h, w = m.shape[-2:]
    top, bottom, left, right, h0, w0 = geometry((h, w), shape, padding)
    ay, ax = axis_matrix(bottom - top, h0), axis_matrix(right - left, w0)
    return ay @ m[..., top:bottom, left:right] @ ax.T


def area_bound(mask_hw, shape):
    """Relative bound of an fp32 area of ey_mask_prompt against this restatement.  Every term is >= 0, so each rounding adds at most u
    relative to the final sum.  The kernel's longest chain for one area:
      ty - 1 and tx - 1 additions inside a row weight and a column weight (ty, tx = axis_terms);
      min(15, mw - 1) additions of column weights into a word's row sum, 1 product with the row weight;
      rows_per_word * ceil(nwords / 256) additions into a thread's accumulator (nwords = ceil(mh mw / 16) words of 16 bytes, a word
      touches at most rows_per_word = ceil(15 / mw) + 1 rows);
      6 levels of the lane tree and 3 additions over the waves."""
    mh, mw = mask_hw
    top, bottom, left, right, h0, w0 = geometry(mask_hw, shape)
    ty, tx = axis_terms(bottom - top, h0), axis_terms(right - left, w0)
    nwords = -(-mh * mw // 16)
    rows_per_word = -(-15 // mw) + 1
    k = (ty - 1) + (tx - 1) + min(15, mw - 1) + 1 + rows_per_word * -(-nwords // 256) + 6 + 3
    return k * U / (1.0 - k * U)


def iou_bound(inter, full, area, e):
    """Absolute bound of fl(inter' / fl(fl(area + full') - inter')) against inter / (area + full - inter) when inter', full' carry the
    relative error e: the denominator moves by e (full + inter) plus its two roundings, the quotient by one more rounding; second-order
    terms are covered by the factor 1.001 (e and u are below 1e-4)."""
    den = area + full - inter
    rel = e + (e * (full + inter) + 2 * U * (area + full)) / den + U
    return 1.001 * (inter / den) * rel


def prompt64(masks, shapes, bboxes=None, points=None, labels=None):
    """masks: list (per image) of uint8 [N_b, mh, mw]; shapes: list of (H0, W0); prompts as int arrays.  -> list (per image) of dicts:
    full [N], inter / iou [P, N], best [P] (ties to the lower index), gap [P] (best minus second best; inf for N == 1), hit bool [Q, N],
    keep bool [N].  An image without masks gives None."""
    boxes = np.zeros((0, 4), np.int64) if bboxes is None else np.asarray(bboxes, np.int64).reshape(-1, 4)
    pts = np.zeros((0, 2), np.int64) if points is None else np.asarray(points, np.int64).reshape(-1, 2)
    labs = np.ones(len(pts), np.int64) if labels is None else np.asarray(labels, np.int64).reshape(-1)
    out = []
    for m, shape in zip(masks, shapes):
        if len(m) == 0:
            out.append(None)
            continue
        r = scale_masks64(m != 0, shape)
        h0, w0 = r.shape[1:]
        d = {"full": r.sum((1, 2))}
        d["inter"] = np.stack([r[:, b[1]:min(b[3], h0), b[0]:min(b[2], w0)].sum((1, 2)) for b in boxes]) if len(boxes) else np.zeros((0, len(m)))
        area = ((boxes[:, 3] - boxes[:, 1]) * (boxes[:, 2] - boxes[:, 0])).astype(np.float64)
        d["area"] = area
        d["iou"] = d["inter"] / (area[:, None] + d["full"][None] - d["inter"])
        d["best"] = d["iou"].argmax(1) if len(boxes) else np.zeros(0, np.int64)
        srt = np.sort(d["iou"], 1)
        d["gap"] = srt[:, -1] - srt[:, -2] if len(m) > 1 else np.full(len(boxes), np.inf)
        d["hit"] = np.stack([r[:, p[1], p[0]] != 0 for p in pts]) if len(pts) else np.zeros((0, len(m)), bool)
        keep = np.zeros(len(m), bool)
        keep[d["best"]] = True
        if len(pts):
            pk = np.ones(len(m), bool) if labs.sum() == 0 else np.zeros(len(m), bool)
            for hrow, lab in zip(d["hit"], labs):
                pk[hrow] = bool(lab)
            keep |= pk
        d["keep"] = keep
        out.append(d)
    return out


def robust_point(masks, shape, x, y, wmin=1e-3):
    """A point every implementation must agree on: for every mask, the (up to) 2 x 2 source pixels of (y, x) are all clear, or one that is
    set has both of its weights >= wmin.  masks uint8 [N, mh, mw]."""
    m = np.asarray(masks) != 0
    if len(m) == 0:
        return True
    top, bottom, left, right, h0, w0 = geometry(m.shape[1:], shape)
    i0, i1, l0, l1 = (a[y] for a in axis_map(bottom - top, h0))
    j0, j1, k0, k1 = (a[x] for a in axis_map(right - left, w0))
    rows, cols = [int(i0), int(i1)], [int(j0), int(j1)]
    wgt = np.outer(np.array([l0, l1], np.float64), np.array([k0, k1], np.float64))
    for mk in m[:, top:bottom, left:right]:
        nb = mk[np.ix_(rows, cols)]
        if nb.any() and not (nb & (wgt >= wmin)).any():
            return False
    return True
