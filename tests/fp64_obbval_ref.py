"""float64 restatement of rotated NMS in the validation regime (multi_label: every (anchor, class) score above conf is a candidate, the
max_nms best by score, fast-NMS on ProbIoU), written from the rule; the pair arithmetic and the helpers are tests/fp64_obb_ref.py's.  numpy."""
import numpy as np

from fp64_obb_ref import nms_boxes, probiou64


def candidates_ml(p, nc, conf, classes, max_nms):
    """One image p (4+nc+1, A) float32 -> (anchor, class, score) of the candidates in NMS order: score > conf (strict, fp32), class filter,
    descending score with ties by ascending anchor * nc + class, the max_nms best."""
    sc = p[4:4 + nc]
    ok = sc > np.float32(conf)
    if classes is not None:
        ok &= np.isin(np.arange(nc), np.asarray(list(classes)))[:, None]
    a, c = np.nonzero(ok.T)  # anchor-major: ascending anchor * nc + class
    s = sc[c, a]
    order = np.lexsort((a * nc + c, -s.astype(np.float64)))[:max_nms]
    return a[order], c[order], s[order]


def nms_rotated_ml64(pred, conf, iou, classes=None, agnostic=False, max_det=300, max_nms=30000, max_wh=7680.0):
    """pred (B, 4+nc+1, A) float32 -> per image dict(anchor, cls, score, total, boxes, colmax, margin, keep, index, kcls, rows): column j of
    the score-ordered candidates is kept iff max(0, max_{i<j} probiou(i, j)) < iou.  margin = |colmax - thr| of every column; total = the
    number of candidates before the max_nms cut; index / kcls = anchor and class of the first max_det kept columns."""
    pred = np.asarray(pred, np.float32)
    nc = pred.shape[1] - 5
    thr = float(np.float32(iou))
    out = []
    for p in pred:
        total = int(candidates_ml(p, nc, conf, classes, p.shape[1] * nc)[0].size)
        a, c, s = candidates_ml(p, nc, conf, classes, max_nms)
        n = len(a)
        boxes = nms_boxes(p, nc, a, c, agnostic, max_wh)
        colmax = np.triu(probiou64(boxes, boxes), 1).max(0) if n else np.zeros(0)  # (the zeros of the lower triangle are part of the maximum)
        keep = colmax < thr
        kc = np.nonzero(keep)[0][:max_det]
        index, kcls = a[kc], c[kc]
        rows = np.stack([p[0, index], p[1, index], p[2, index], p[3, index], s[kc], kcls.astype(np.float32), p[4 + nc, index]], 1) if len(kc) else np.zeros((0, 7), np.float32)
        out.append(dict(anchor=a, cls=c, score=s, total=total, boxes=boxes, colmax=colmax, margin=np.abs(colmax - thr), keep=keep, index=index, kcls=kcls,
                        rows=rows.astype(np.float32)))
    return out


def distinct_scores(pred, conf):
    """True when no two candidate scores of an image are equal (the order of the candidates is then the same under every sort)."""
    pred = np.asarray(pred, np.float32)
    for p in pred:
        s = p[4:-1][p[4:-1] > np.float32(conf)]
        if len(np.unique(s)) != len(s):
            return False
    return True
