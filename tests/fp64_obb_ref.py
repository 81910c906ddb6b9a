"""float64 restatements for the obb task, written from the formulas (DFL expectation + rotated anchor decode, the Bhattacharyya /
Hellinger form of ProbIoU, fast-NMS): the yardstick the HIP kernels and the reference's fp32 results are both measured against.  numpy."""
import numpy as np

EPS = 1e-7


def _sigmoid(v):
    return 1.0 / (1.0 + np.exp(-v))


def decode64(levels, strides):
    """levels: per level (box (B,64,H,W), cls (B,nc,H,W), angle logits (B,1,H,W)) -> (B, 4+nc+1, A) float64: rows 0-3 the rotated box
    (cx, cy, w, h) in input pixels, then the class probabilities, last the angle (sigmoid(a) - 1/4) pi."""
    out = []
    for (box, cls, ang), s in zip(levels, strides):
        box, cls, ang = (np.asarray(t, np.float64) for t in (box, cls, ang))
        B, _, H, W = box.shape
        l = box.reshape(B, 4, 16, H * W)
        e = np.exp(l - l.max(2, keepdims=True))
        dist = ((e / e.sum(2, keepdims=True)) * np.arange(16.0)[None, None, :, None]).sum(2)  # (B,4,HW): left, top, right, bottom
        th = (_sigmoid(ang.reshape(B, H * W)) - 0.25) * np.pi
        gx, gy = np.tile(np.arange(W) + 0.5, H), np.repeat(np.arange(H) + 0.5, W)
        xf, yf = (dist[:, 2] - dist[:, 0]) / 2, (dist[:, 3] - dist[:, 1]) / 2
        x = xf * np.cos(th) - yf * np.sin(th) + gx
        y = xf * np.sin(th) + yf * np.cos(th) + gy
        rows = [x * s, y * s, (dist[:, 0] + dist[:, 2]) * s, (dist[:, 1] + dist[:, 3]) * s]
        out.append(np.concatenate([np.stack(rows, 1), _sigmoid(cls.reshape(B, -1, H * W)), th[:, None]], 1))
    return np.concatenate(out, 2)


def _cov(b):
    a, c = b[:, 2] ** 2 / 12.0, b[:, 3] ** 2 / 12.0
    cs, sn = np.cos(b[:, 4]), np.sin(b[:, 4])
    return a * cs ** 2 + c * sn ** 2, a * sn ** 2 + c * cs ** 2, (a - c) * cs * sn


def probiou64(o1, o2):
    """(N,5), (M,5) xywhr -> (N,M) float64: 1 - sqrt(1 - exp(-bd) + eps), bd the clamped Bhattacharyya distance of the boxes' Gaussians."""
    o1, o2 = np.asarray(o1, np.float64), np.asarray(o2, np.float64)
    a1, b1, c1 = (t[:, None] for t in _cov(o1))
    a2, b2, c2 = (t[None, :] for t in _cov(o2))
    dx, dy = o1[:, 0, None] - o2[None, :, 0], o1[:, 1, None] - o2[None, :, 1]
    sa, sb, sc = a1 + a2, b1 + b2, c1 + c2
    det = sa * sb - sc ** 2
    t1 = (sa * dy ** 2 + sb * dx ** 2) / (det + EPS) * 0.25
    t2 = (sc * -dx * dy) / (det + EPS) * 0.5
    d1, d2 = np.maximum(a1 * b1 - c1 ** 2, 0.0), np.maximum(a2 * b2 - c2 ** 2, 0.0)
    t3 = np.log(det / (4.0 * np.sqrt(d1 * d2) + EPS) + EPS) * 0.5
    bd = np.clip(t1 + t2 + t3, EPS, 100.0)
    return 1.0 - np.sqrt(1.0 - np.exp(-bd) + EPS)


def candidates(p, nc, conf, classes, max_nms):
    """One image p (4+nc+1, A) float32 -> (anchors in NMS order, best score, class): best class score > conf (strict, fp32), class filter,
    descending score with ties by ascending anchor, the max_nms best."""
    sc = p[4:4 + nc]
    cls = sc.argmax(0)
    best = sc[cls, np.arange(sc.shape[1])]
    ok = best > np.float32(conf)
    if classes is not None:
        ok &= np.isin(cls, np.asarray(list(classes)))
    idx = np.nonzero(ok)[0]
    idx = idx[np.lexsort((idx, -best[idx].astype(np.float64)))][:max_nms]
    return idx, best[idx], cls[idx]


def nms_boxes(p, nc, idx, cls, agnostic, max_wh):
    """The (n,5) float32 pair input: (x + c max_wh, y + c max_wh, w, h, r), the sum formed in float32."""
    c = cls.astype(np.float32) * np.float32(0.0 if agnostic else max_wh)
    return np.stack([p[0, idx] + c, p[1, idx] + c, p[2, idx], p[3, idx], p[4 + nc, idx]], 1).astype(np.float32)


def nms_rotated64(pred, conf, iou, classes=None, agnostic=False, max_det=300, max_nms=30000, max_wh=7680.0):
    """pred (B, 4+nc+1, A) float32 -> per image dict(order, colmax, margin, keep, index, rows): column j of the score-ordered candidates is
    kept iff max(0, max_{i<j} probiou(i, j)) < iou."""
    pred = np.asarray(pred, np.float32)
    nc = pred.shape[1] - 5
    thr = float(np.float32(iou))
    out = []
    for p in pred:
        idx, best, cls = candidates(p, nc, conf, classes, max_nms)
        n = len(idx)
        boxes = nms_boxes(p, nc, idx, cls, agnostic, max_wh)
        colmax = np.triu(probiou64(boxes, boxes), 1).max(0) if n else np.zeros(0)  # (the zeros of the lower triangle are part of the maximum)
        keep = colmax < thr
        index = idx[keep][:max_det]
        kc = np.nonzero(keep)[0][:max_det]
        rows = np.stack([p[0, index], p[1, index], p[2, index], p[3, index], best[kc], cls[kc].astype(np.float32), p[4 + nc, index]], 1) if len(index) else np.zeros((0, 7), np.float32)
        out.append(dict(order=idx, boxes=boxes, colmax=colmax, margin=np.abs(colmax - thr), keep=keep, index=index, rows=rows.astype(np.float32)))
    return out


def ulp32(v):
    return np.spacing(np.abs(np.asarray(v, np.float64)).astype(np.float32)).astype(np.float64)


def bound(err_ref, value):
    """The tolerance rule for every float output of the obb kernels: 4 E + 2 ulp(fp32) of the value, E = the reference's own fp32 error."""
    return 4.0 * err_ref + 2.0 * ulp32(value)
