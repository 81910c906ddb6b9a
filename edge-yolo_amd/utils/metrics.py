"""Detection validation metrics on the host (numpy), mirroring the reference's definitions so that the same predictions
give the same mAP: `box_iou` (utils/metrics.py:52-72), `match_predictions` (engine/validator.py:222-262, the default
non-scipy branch), `compute_ap` / `ap_per_class` (utils/metrics.py:505-623), `smooth` (:494-502), and the fitness-style
summary of `DetMetrics` (:808).  The reference runs these on the CPU as well; only NMS (validation mode: conf 0.001,
multi_label, models/yolo/detect/val.py:92-102) is device work and goes through `ey_nms`.

Segment validation adds `mask_iou` (utils/metrics.py:137-153; device tensors run on `ey_mask_iou`, host arrays on a numpy restatement with
the same bits), the host form of the overlap_mask expansion (models/yolo/segment/val.py:206-209) and `SegmentMetrics` (:909-1029).

`batch_probiou` (utils/metrics.py:244-275) is the pairwise ProbIoU of oriented boxes on `ey_probiou` (device tensors only); `probiou_host` is its
numpy restatement for host operands and `OBBMetrics` (:1240-1308) the obb task's metrics.

Pose validation adds `OKS_SIGMA` (:17-20), `kpt_iou` (:156-175; device tensors on `ey_kpt_iou`, host operands on a numpy restatement) and
`PoseMetrics` (:1051-1176)."""
import numpy as np


def box_iou(box1, box2, eps=1e-7):
    """(N,4) x (M,4) xyxy -> (N,M) IoU, float32 arithmetic like the reference."""
    b1 = np.asarray(box1, np.float32)[:, None, :]
    b2 = np.asarray(box2, np.float32)[None, :, :]
    wh = np.clip(np.minimum(b1[..., 2:], b2[..., 2:]) - np.maximum(b1[..., :2], b2[..., :2]), 0, None)
    inter = wh[..., 0] * wh[..., 1]
    a1 = (b1[..., 2] - b1[..., 0]) * (b1[..., 3] - b1[..., 1])
    a2 = (b2[..., 2] - b2[..., 0]) * (b2[..., 3] - b2[..., 1])
    return inter / (a1 + a2 - inter + np.float32(eps))


IOUV = np.linspace(0.5, 0.95, 10)  # mAP@0.5:0.95 thresholds (models/yolo/detect/val.py:38)


def match_predictions(pred_classes, true_classes, iou, iouv=IOUV):
    """iou: (L labels, D detections).  Returns the (D, len(iouv)) boolean "correct" matrix: per threshold, candidate
    (label, detection) pairs of matching class with IoU >= thr are taken in descending IoU order, keeping each detection
    and then each label once."""
    pred_classes, true_classes = np.asarray(pred_classes), np.asarray(true_classes)
    correct = np.zeros((pred_classes.shape[0], len(iouv)), bool)
    iou = np.asarray(iou) * (true_classes[:, None] == pred_classes)
    for i, thr in enumerate(np.asarray(iouv).tolist()):
        m = np.array(np.nonzero(iou >= thr)).T
        if m.shape[0]:
            if m.shape[0] > 1:
                m = m[iou[m[:, 0], m[:, 1]].argsort()[::-1]]
                m = m[np.unique(m[:, 1], return_index=True)[1]]
                m = m[np.unique(m[:, 0], return_index=True)[1]]
            correct[m[:, 1].astype(int), i] = True
    return correct


def _closed_tp(iou, gt_cls, det_cls, iouv):
    """match_predictions as the closed form the kernel runs (csrc/match_core.inc.h): iou (G, D) fp32 -> (D, T) bool.  Best label per detection
    (of equal ones the higher index), then every label goes to the lowest detection that wants it at the threshold."""
    iou = np.asarray(iou, np.float32)
    G, D = iou.shape
    thr = np.asarray(iouv, np.float32)
    tp = np.zeros((D, len(thr)), bool)
    if G == 0 or D == 0:
        return tp
    q = iou * (np.asarray(gt_cls, np.float32)[:, None] == np.asarray(det_cls, np.float32)[None, :])
    gs = G - 1 - np.argmax(q[::-1], axis=0)
    b = q[gs, np.arange(D)]
    for t in range(len(thr)):
        d = np.nonzero(b >= thr[t])[0]
        taker = np.full(G, D, np.int64)
        np.minimum.at(taker, gs[d], d)
        tp[d, t] = taker[gs[d]] == d
    return tp


def _closed_cm(matrix, iou, gt_cls, det_cls, conf, nc, cm_conf, cm_iou):
    """ConfusionMatrix.process_batch as the closed form the kernel runs: adds one image to `matrix` ((nc+1, nc+1), row = predicted).  Among the
    detections above cm_conf: best label per detection (valid above cm_iou), then every label takes its highest-IoU detection (of equal ones the
    lower index); what is left on either side goes to the background row / column."""
    iou = np.asarray(iou, np.float32)
    gt_cls, det_cls = np.asarray(gt_cls).astype(np.int64), np.asarray(det_cls).astype(np.int64)
    part = np.nonzero(np.asarray(conf, np.float32) > np.float32(cm_conf))[0]
    G = len(gt_cls)
    taken = np.full(G, -1, np.int64)
    if G and len(part):
        sub = iou[:, part]
        gs = G - 1 - np.argmax(sub[::-1], axis=0)
        b = sub[gs, np.arange(len(part))]
        ok = b > np.float32(cm_iou)
        for g in np.unique(gs[ok]):
            k = np.nonzero(ok & (gs == g))[0]
            taken[g] = part[k[np.argmax(b[k])]]  # argmax: the first of equal values
    for g in range(G):
        matrix[det_cls[taken[g]] if taken[g] >= 0 else nc, gt_cls[g]] += 1
    for d in np.setdiff1d(part, taken[taken >= 0]):
        matrix[det_cls[d], nc] += 1


def _is_dev(t):
    return hasattr(t, "is_cuda") and t.is_cuda


def _check_classes(cls, nc, what):
    c = np.asarray(_host(cls)).reshape(-1)
    if len(c) and not ((c >= 0) & (c < nc) & (c == np.floor(c))).all():
        raise ValueError(f"{what}: class ids must be integers in [0, {nc}), got {c[~((c >= 0) & (c < nc) & (c == np.floor(c)))][:4].tolist()}")
    return c.astype(np.int32)


def _labels_to(dev, gt, gt_cls, nc, what, width=4):
    """labels for the kernel: boxes fp32 (M, width) and classes int32 (M,) on `dev`; host class ids are checked before the upload."""
    import torch
    if not _is_dev(gt_cls):
        gt_cls = torch.from_numpy(_check_classes(gt_cls, nc, what)).to(dev)
    if gt is not None and not _is_dev(gt):
        gt = torch.from_numpy(np.ascontiguousarray(np.asarray(_host(gt), np.float32).reshape(-1, width))).to(dev)
    return None if gt is None else gt.float().contiguous(), gt_cls.to(torch.int32).contiguous()


def match_batch(rows, gt_bboxes, gt_cls, iouv=IOUV, iou=None, count=None, gt_off=None, nc=None, xform=None, iou_off=None, iou_n=None):
    """The true positives of match_predictions, as the closed form of csrc/match_core.inc.h.
    Host form (count is None): rows (n, 6+) x1,y1,x2,y2,conf,cls of ONE image and its labels gt_bboxes (m, 4) xyxy, gt_cls (m,), all in one
      frame -> (n, len(iouv)) bool in numpy; iou: the image's (m, n) matrix in the place of the box IoU.
    Device form: rows (B, max_det, >= 6) fp32 and count (B,) int32 on the device, as ops.nms_device returns them, the labels of the batch
      (gt_bboxes (M, 4), gt_cls (M,), host or device) grouped by the host list gt_off, nc, and optionally xform (B, 5) padx, pady, gain, w0, h0
      (host or device) or the flat matrices iou / iou_off / iou_n -> uint8 (B, max_det, T) on the device from one ey_match_batch launch, zero at
      and beyond each image's count."""
    if count is None:
        if _is_dev(rows):
            raise ValueError("match_batch: device rows need count= and gt_off= (the batch form)")
        r = np.asarray(_host(rows), np.float32)
        r = r.reshape(-1, r.shape[-1] if r.ndim == 2 else 6)
        g = np.asarray(_host(gt_cls)).reshape(-1)
        m = box_iou(np.asarray(_host(gt_bboxes), np.float32).reshape(-1, 4), r[:, :4]) if iou is None else np.asarray(_host(iou), np.float32).reshape(len(g), len(r))
        return _closed_tp(m, g, r[:, 5], iouv)
    import torch
    from ..nn import _ops
    if not _is_dev(rows):
        raise ValueError("match_batch: the batch form runs on the device: rows on the host go through the per-image form (count=None)")
    if nc is None or gt_off is None:
        raise ValueError("match_batch: the batch form needs nc= and gt_off=")
    dev = rows.device
    gt, cls = _labels_to(dev, None if iou is not None else gt_bboxes, gt_cls, nc, "match_batch")
    if xform is not None and not _is_dev(xform):
        xform = torch.from_numpy(np.ascontiguousarray(np.asarray(_host(xform), np.float32).reshape(-1, 5))).to(dev)
    with torch.cuda.device(dev):
        tp = torch.zeros((rows.shape[0], rows.shape[1], len(iouv)), dtype=torch.uint8, device=dev)
        _ops.match_batch(rows, count, cls, gt_off, iouv, nc, gt=gt, xform=xform, iou=iou, iou_off=iou_off, iou_n=iou_n, tp=tp)
    return tp


class ConfusionMatrix:
    """The reference's ConfusionMatrix (utils/metrics.py:294-393): `matrix` (float64, (nc+1, nc+1) for task "detect" with the background last,
    (nc, nc) for "classify"; row = predicted, column = true), `process_batch`, `process_cls_preds`, `tp_fp`, `print`.  Host operands take the
    numpy closed form, device tensors ey_match_batch (integer atomics into an int32 matrix on the device, which `matrix` adds in); both give
    the reference's counts on tie-free data, and on exact IoU ties the rule of csrc/match_core.inc.h (the reference's is numpy's unstable
    sort).  plot() is not built."""

    def __init__(self, nc, conf=0.25, iou_thres=0.45, task="detect"):
        self.task = task
        self.nc = int(nc)
        self._host_matrix = np.zeros((self.nc + 1, self.nc + 1)) if task == "detect" else np.zeros((self.nc, self.nc))
        self._dev_matrix = None
        self.conf = 0.25 if conf in {None, 0.001} else conf  # the reference's rule: the validation default means 0.25 here
        self.iou_thres = iou_thres

    @property
    def matrix(self):
        if self._dev_matrix is None:
            return self._host_matrix
        return self._host_matrix + self._dev_matrix.cpu().numpy().reshape(self.nc + 1, self.nc + 1)

    def _device_counts(self, dev):
        import torch
        if self.task != "detect":
            raise ValueError("ConfusionMatrix: process_batch is the detect task's; task='classify' takes process_cls_preds")
        if self._dev_matrix is None or self._dev_matrix.device != dev:
            if self._dev_matrix is not None:
                self._host_matrix += self._dev_matrix.cpu().numpy().reshape(self.nc + 1, self.nc + 1)
            self._dev_matrix = torch.zeros((self.nc + 1) ** 2, dtype=torch.int32, device=dev)
        return self._dev_matrix

    def process_cls_preds(self, preds, targets):
        """preds: list of (n_i, k) top-k class arrays, best first; targets: list of (n_i,) classes.  On the host."""
        p = np.concatenate([np.asarray(_host(x)).reshape(len(x), -1) for x in preds])[:, 0].astype(np.int64)
        t = np.concatenate([np.asarray(_host(x)).reshape(-1) for x in targets]).astype(np.int64)
        if len(p) != len(t) or (len(p) and not ((p >= 0) & (p < self.nc) & (t >= 0) & (t < self.nc)).all()):
            raise ValueError(f"ConfusionMatrix.process_cls_preds: {len(p)} predictions, {len(t)} targets, classes must lie in [0, {self.nc})")
        np.add.at(self._host_matrix, (p, t), 1)

    def process_batch(self, detections, gt_bboxes, gt_cls):
        """One image.  detections (n, 6) x1,y1,x2,y2,conf,cls or (n, 7) x,y,w,h,conf,cls,angle with (m, 5) xywhr labels, or None; gt_bboxes
        (m, 4 | 5); gt_cls (m,).  Device detections run ey_match_batch (obb: on the ProbIoU matrix of ey_probiou), host ones numpy.  Class ids
        outside [0, nc) raise ValueError on both routes (the device route reads the rows' class column for that; process_device_batch does not)."""
        if self.task != "detect":
            raise ValueError("ConfusionMatrix: process_batch is the detect task's; task='classify' takes process_cls_preds")
        if _is_dev(detections):
            import torch
            from ..nn import _ops
            dev = detections.device
            det = detections.float()
            if not _is_dev(gt_cls):
                gt_cls = np.asarray(_host(gt_cls)).reshape(-1)
            if not _is_dev(gt_bboxes):
                gt_bboxes = np.asarray(_host(gt_bboxes), np.float32)
            n, m = int(det.shape[0]), int(gt_cls.shape[0])
            obb = det.dim() == 2 and det.shape[1] == 7 and gt_bboxes.shape[-1] == 5
            _check_classes(det[:, 5], self.nc, "ConfusionMatrix.process_batch: detections")  # (as the host route; one read of the column)
            gt, cls = _labels_to(dev, gt_bboxes, gt_cls, self.nc, "ConfusionMatrix.process_batch", 5 if obb else 4)
            with torch.cuda.device(dev):
                iou = off = ld = None
                if obb and n and m:
                    iou, off, ld = _ops.probiou(gt, det[:, [0, 1, 2, 3, 6]].contiguous()).reshape(-1), [0], [n]
                elif obb:
                    iou, off, ld = torch.zeros(1, dtype=torch.float32, device=dev), [0], [n]
                rows = det[None, :, :6].contiguous() if n else torch.zeros((1, 1, 6), dtype=torch.float32, device=dev)
                count = torch.full((1,), n, dtype=torch.int32, device=dev)
                _ops.match_batch(rows, count, cls, [0, m], IOUV[:1], self.nc, gt=None if obb else gt, iou=iou, iou_off=off, iou_n=ld, cm_conf=self.conf,
                                 cm_iou=self.iou_thres, matrix=self._device_counts(dev))
            return
        g = _check_classes(gt_cls, self.nc, "ConfusionMatrix.process_batch")
        if detections is None:
            det = np.zeros((0, 6), np.float32)
        else:
            det = np.asarray(_host(detections), np.float32)
            det = det.reshape(-1, det.shape[-1] if det.ndim == 2 else 6)
        _check_classes(det[:, 5], self.nc, "ConfusionMatrix.process_batch: detections")
        gb = np.asarray(_host(gt_bboxes), np.float32)
        if not len(g) or not len(det):
            iou = np.zeros((len(g), len(det)), np.float32)
        elif det.shape[1] == 7 and gb.shape[-1] == 5:
            iou = probiou_host(gb.reshape(-1, 5), np.concatenate([det[:, :4], det[:, -1:]], 1))
        else:
            iou = box_iou(gb.reshape(-1, 4), det[:, :4])
        _closed_cm(self._host_matrix, iou, g, det[:, 5], det[:, 4], self.nc, self.conf, self.iou_thres)

    def process_device_batch(self, rows, count, gt_bboxes, gt_cls, gt_off, xform=None, iou=None, iou_off=None, iou_n=None, iouv=None):
        """A whole batch in ONE ey_match_batch launch: rows (B, max_det, >= 6) / count (B,) as ops.nms_device returns them, the batch's labels
        (host or device) grouped by the host list gt_off, xform or the flat matrices as for match_batch.  iouv given: the launch also returns
        the true positives, uint8 (B, max_det, T), zero at and beyond each count; else None."""
        import torch
        from ..nn import _ops
        if not _is_dev(rows):
            raise ValueError("ConfusionMatrix.process_device_batch: rows on the host go image by image through process_batch")
        dev = rows.device
        gt, cls = _labels_to(dev, None if iou is not None else gt_bboxes, gt_cls, self.nc, "ConfusionMatrix.process_device_batch")
        if xform is not None and not _is_dev(xform):
            xform = torch.from_numpy(np.ascontiguousarray(np.asarray(_host(xform), np.float32).reshape(-1, 5))).to(dev)
        with torch.cuda.device(dev):
            tp = None if iouv is None else torch.zeros((rows.shape[0], rows.shape[1], len(iouv)), dtype=torch.uint8, device=dev)
            _ops.match_batch(rows, count, cls, gt_off, IOUV[:1] if iouv is None else iouv, self.nc, gt=gt, xform=xform, iou=iou, iou_off=iou_off, iou_n=iou_n,
                             cm_conf=self.conf, cm_iou=self.iou_thres, tp=tp, matrix=self._device_counts(dev))
        return tp

    def tp_fp(self):
        m = self.matrix
        tp = m.diagonal()
        fp = m.sum(1) - tp
        return (tp[:-1], fp[:-1]) if self.task == "detect" else (tp, fp)

    def print(self):
        for row in self.matrix:
            print(" ".join(map(str, row)))


def smooth(y, f=0.05):
    nf = round(len(y) * f * 2) // 2 + 1
    p = np.ones(nf // 2)
    yp = np.concatenate((p * y[0], y, p * y[-1]), 0)
    return np.convolve(yp, np.ones(nf) / nf, mode="valid")


def compute_ap(recall, precision):
    mrec = np.concatenate(([0.0], recall, [1.0]))
    mpre = np.concatenate(([1.0], precision, [0.0]))
    mpre = np.flip(np.maximum.accumulate(np.flip(mpre)))
    x = np.linspace(0, 1, 101)  # 101-point COCO interpolation
    trapz = getattr(np, "trapezoid", None) or np.trapz
    return trapz(np.interp(x, mrec, mpre), x), mpre, mrec


def ap_per_class(tp, conf, pred_cls, target_cls, eps=1e-16):
    """-> dict(tp, fp, p, r, f1, ap (nc,10), classes)."""
    i = np.argsort(-conf)
    tp, conf, pred_cls = tp[i], conf[i], pred_cls[i]
    classes, nt = np.unique(target_cls, return_counts=True)
    nc = classes.shape[0]
    x = np.linspace(0, 1, 1000)
    ap, p_curve, r_curve = np.zeros((nc, tp.shape[1])), np.zeros((nc, 1000)), np.zeros((nc, 1000))
    for ci, c in enumerate(classes):
        sel = pred_cls == c
        n_l, n_p = nt[ci], sel.sum()
        if n_p == 0 or n_l == 0:
            continue
        fpc = (1 - tp[sel]).cumsum(0)
        tpc = tp[sel].cumsum(0)
        recall = tpc / (n_l + eps)
        r_curve[ci] = np.interp(-x, -conf[sel], recall[:, 0], left=0)
        precision = tpc / (tpc + fpc)
        p_curve[ci] = np.interp(-x, -conf[sel], precision[:, 0], left=1)
        for j in range(tp.shape[1]):
            ap[ci, j] = compute_ap(recall[:, j], precision[:, j])[0]
    f1_curve = 2 * p_curve * r_curve / (p_curve + r_curve + eps)
    k = smooth(f1_curve.mean(0), 0.1).argmax()
    p, r, f1 = p_curve[:, k], r_curve[:, k], f1_curve[:, k]
    tpn = (r * nt).round()
    fpn = (tpn / (p + eps) - tpn).round()
    return dict(tp=tpn, fp=fpn, p=p, r=r, f1=f1, ap=ap, classes=classes.astype(int))


class DetMetrics:
    """Accumulates per-image matches and reports mp, mr, mAP50, mAP50-95 (reference DetMetrics / Metric, metrics.py:627-808)."""

    def __init__(self, iouv=IOUV):
        self.iouv = iouv
        self.tp, self.conf, self.pred_cls, self.target_cls = [], [], [], []

    def update(self, det, labels):
        """det: (n,6) x1,y1,x2,y2,conf,cls (same pixel frame as labels); labels: (m,5) cls,x1,y1,x2,y2."""
        det, labels = np.asarray(det, np.float32).reshape(-1, 6), np.asarray(labels, np.float32).reshape(-1, 5)
        self.target_cls.append(labels[:, 0])
        if det.shape[0] == 0:
            return
        if labels.shape[0]:
            correct = match_predictions(det[:, 5], labels[:, 0], box_iou(labels[:, 1:], det[:, :4]), self.iouv)
        else:
            correct = np.zeros((det.shape[0], len(self.iouv)), bool)
        self.tp.append(correct)
        self.conf.append(det[:, 4])
        self.pred_cls.append(det[:, 5])

    def results(self):
        if not self.tp:
            return dict(mp=0.0, mr=0.0, map50=0.0, map=0.0)
        r = ap_per_class(np.concatenate(self.tp), np.concatenate(self.conf), np.concatenate(self.pred_cls), np.concatenate(self.target_cls))
        ap = r["ap"]
        return dict(mp=float(r["p"].mean()) if len(r["p"]) else 0.0, mr=float(r["r"].mean()) if len(r["r"]) else 0.0,
                    map50=float(ap[:, 0].mean()) if len(ap) else 0.0, map=float(ap.mean()) if len(ap) else 0.0, per_class=r)


def mask_iou_counts(inter, area1, area2, eps=1e-7):
    """Integer counts -> the reference's fp32 expression, one rounding per operation (utils/metrics.py:151-153):
    iou = fl(inter / fl(fl(fl(area1 + area2) - inter) + fl(eps))).  Counts up to 2^24 are exact in fp32."""
    inter = np.asarray(inter).astype(np.float32)
    union = (np.asarray(area1).astype(np.float32)[:, None] + np.asarray(area2).astype(np.float32)[None, :]) - inter
    return inter / (union + np.float32(eps))


def mask_iou(mask1, mask2, eps=1e-7):
    """Reference signature (utils/metrics.py:137-153): mask1 (M, n) ground truth x mask2 (N, n) predictions, 0/1 -> (M, N) fp32 IoU.
    Device tensors run on ey_mask_iou (bit-packed population counts) and return a device tensor; host arrays / CPU tensors take the
    numpy restatement below -- integer counts, then the same fp32 expression -- and return an ndarray.  Both give the reference's bits."""
    import torch
    if torch.is_tensor(mask1) and mask1.is_cuda:
        from ..nn import _ops
        if abs(float(eps) - 1e-7) > 1e-20:
            raise NotImplementedError("mask_iou: the kernel is built for the reference's eps=1e-7")
        if not (torch.is_tensor(mask2) and mask2.device == mask1.device) or mask1.dim() != 2 or mask2.dim() != 2 or mask1.shape[1] != mask2.shape[1]:
            raise ValueError("mask_iou: expected (M, n) and (N, n) tensors on one device")
        M, n = mask1.shape
        N = mask2.shape[0]
        if M == 0 or N == 0 or n == 0:
            return torch.zeros((M, N), dtype=torch.float32, device=mask1.device)
        u8 = [m.contiguous() if m.dtype == torch.uint8 else (m != 0).to(torch.uint8) for m in (mask1, mask2)]  # (layout only)
        with torch.cuda.device(mask1.device):
            iou, _, _ = _ops.mask_iou(u8[1].view(N, 1, n), [0, N], u8[0].view(M, 1, n), [0, M])
        return iou.view(M, N)
    g = (np.asarray(mask1.detach().cpu().numpy() if torch.is_tensor(mask1) else mask1) != 0).astype(np.float32)
    p = (np.asarray(mask2.detach().cpu().numpy() if torch.is_tensor(mask2) else mask2) != 0).astype(np.float32)
    if g.ndim != 2 or p.ndim != 2 or g.shape[1] != p.shape[1]:
        raise ValueError("mask_iou: expected (M, n) and (N, n) masks")
    if g.shape[1] > 1 << 24:
        raise NotImplementedError("mask_iou: more than 2^24 pixels (the counts would not be exact in fp32)")
    inter = g @ p.T  # 0/1 operands, sums below 2^24: the fp32 product is the exact count in any summation order
    return mask_iou_counts(inter, g.sum(1), p.sum(1), eps)


def batch_probiou(obb1, obb2, eps=1e-7):
    """(N,5) x (M,5) xywhr -> (N,M) fp32 ProbIoU (https://arxiv.org/pdf/2106.06072v1.pdf) on ey_probiou.  Device tensors; numpy arrays and
    host tensors are moved to the current device and the result comes back where the first operand was.  eps is the kernel's 1e-7."""
    import torch
    from ..nn import _ops
    if eps != 1e-7:
        raise NotImplementedError(f"batch_probiou: eps={eps} (the kernel is built for the reference's 1e-7)")
    o1 = torch.from_numpy(obb1) if isinstance(obb1, np.ndarray) else obb1
    o2 = torch.from_numpy(obb2) if isinstance(obb2, np.ndarray) else obb2
    dev = o1.device if o1.is_cuda else (o2.device if o2.is_cuda else torch.device("cuda", torch.cuda.current_device()))
    with torch.cuda.device(dev):
        out = _ops.probiou(o1.to(dev), o2.to(dev))
    return out if o1.is_cuda else out.to(o1.device)


def probiou_host(obb1, obb2, eps=1e-7):
    """batch_probiou for host operands: (N,5) x (M,5) xywhr arrays / CPU tensors -> (N,M) fp32 ndarray, the numpy restatement of the
    reference's fp32 expression (metrics.py:178-195,244-275), operation by operation.  The route of a validator without a device."""
    f = np.float32
    o1, o2 = np.asarray(_host(obb1), f).reshape(-1, 5), np.asarray(_host(obb2), f).reshape(-1, 5)

    def cov(b):
        a, c = b[:, 2] ** 2 / f(12), b[:, 3] ** 2 / f(12)
        cs, sn = np.cos(b[:, 4]), np.sin(b[:, 4])
        return a * cs ** 2 + c * sn ** 2, a * sn ** 2 + c * cs ** 2, (a - c) * cs * sn

    x1, y1, x2, y2 = o1[:, 0, None], o1[:, 1, None], o2[None, :, 0], o2[None, :, 1]
    a1, b1, c1 = (t[:, None] for t in cov(o1))
    a2, b2, c2 = (t[None, :] for t in cov(o2))
    e = f(eps)
    det = (a1 + a2) * (b1 + b2) - (c1 + c2) ** 2
    t1 = (((a1 + a2) * (y1 - y2) ** 2 + (b1 + b2) * (x1 - x2) ** 2) / (det + e)) * f(0.25)
    t2 = (((c1 + c2) * (x2 - x1) * (y1 - y2)) / (det + e)) * f(0.5)
    t3 = np.log(det / (f(4) * np.sqrt(np.maximum(a1 * b1 - c1 ** 2, f(0)) * np.maximum(a2 * b2 - c2 ** 2, f(0))) + e) + e) * f(0.5)
    bd = np.clip(t1 + t2 + t3, e, f(100))
    return (f(1) - np.sqrt(f(1) - np.exp(-bd) + e)).astype(f)


# per-keypoint falloff constants of the COCO keypoint evaluation (reference utils/metrics.py:17-20)
OKS_SIGMA = np.array([0.26, 0.25, 0.25, 0.35, 0.35, 0.79, 0.79, 0.72, 0.72, 0.62, 0.62, 1.07, 1.07, 0.87, 0.87, 0.89, 0.89]) / 10.0


def kpt_iou(kpt1, kpt2, area, sigma, eps=1e-7):
    """Object keypoint similarity, reference signature (utils/metrics.py:156-175): kpt1 (N,K,3) ground truth, kpt2 (M,K,2 or 3) predictions,
    area (N,) of the ground-truth boxes, sigma (K,) -> (N,M) fp32.  Device tensors run one ey_kpt_iou call and return a device tensor; host
    arrays / CPU tensors take the numpy restatement below (the reference's fp32 expression, operation by operation) and return an ndarray."""
    import torch
    if torch.is_tensor(kpt1) and kpt1.is_cuda:
        from ..nn import _ops
        if abs(float(eps) - 1e-7) > 1e-20:
            raise NotImplementedError("kpt_iou: the kernel is built for the reference's eps=1e-7")
        dev = kpt1.device
        N, M = kpt1.shape[0], kpt2.shape[0]
        if N == 0 or M == 0:
            return torch.zeros((N, M), dtype=torch.float32, device=dev)
        sg = torch.as_tensor(np.asarray(_host(sigma), np.float32)).to(dev) if not (torch.is_tensor(sigma) and sigma.is_cuda) else sigma.float().contiguous()
        with torch.cuda.device(dev):
            out, _ = _ops.kpt_iou(kpt2.to(dev).float().contiguous(), [0, M], kpt1.float().contiguous(), [0, N], torch.as_tensor(area).to(dev).float().contiguous(), sg)
        return out.view(N, M)
    g, p, a = (np.asarray(_host(t), np.float32) for t in (kpt1, kpt2, area))
    sg = np.asarray(_host(sigma), np.float32)
    if g.ndim != 3 or p.ndim != 3 or g.shape[2] != 3 or p.shape[2] < 2 or g.shape[1] != p.shape[1] or sg.shape != (g.shape[1],) or a.shape != (g.shape[0],):
        raise ValueError(f"kpt_iou: expected (N,K,3), (M,K,2|3), (N,), (K,), got {g.shape}, {p.shape}, {a.shape}, {sg.shape}")
    d = (g[:, None, :, 0] - p[None, :, :, 0]) ** 2 + (g[:, None, :, 1] - p[None, :, :, 1]) ** 2  # (N, M, K)
    vis = g[..., 2] != 0
    e = d / ((np.float32(2) * sg) ** 2 * (a[:, None, None] + np.float32(eps)) * np.float32(2))
    return ((np.exp(-e) * vis[:, None].astype(np.float32)).sum(-1, dtype=np.float32) / (vis.sum(-1)[:, None].astype(np.float32) + np.float32(eps))).astype(np.float32)


def _host(t):
    return t.detach().cpu().numpy() if hasattr(t, "detach") else t


def expand_index_masks(index_map, nl):
    """Host form of the reference's overlap_mask expansion (models/yolo/segment/val.py:206-209): one (h, w) index map ->
    (nl, h, w) uint8, instance m = the pixels equal to m + 1.  (ey_mask_iou reads the map directly; this is for host masks.)"""
    m = np.asarray(index_map)
    m = m.reshape(m.shape[-2:])
    return (m[None] == (np.arange(nl).reshape(nl, 1, 1) + 1)).astype(np.uint8)


SEG_KEYS = ["metrics/precision(B)", "metrics/recall(B)", "metrics/mAP50(B)", "metrics/mAP75(B)", "metrics/mAP50-95(B)",
            "metrics/precision(M)", "metrics/recall(M)", "metrics/mAP50(M)", "metrics/mAP75(M)", "metrics/mAP50-95(M)"]  # reference metrics.py:988-1001


class Metric:
    """Per-class results of one ap_per_class run and their means (reference Metric, metrics.py:626-761, with the fork's mAP75 column)."""

    def __init__(self):
        self.p, self.r, self.f1, self.all_ap, self.ap_class_index = [], [], [], [], []

    def update(self, r):
        self.p, self.r, self.f1, self.all_ap, self.ap_class_index = r["p"], r["r"], r["f1"], r["ap"], r["classes"]

    def mean_results(self):
        ap = self.all_ap
        return [float(self.p.mean()) if len(self.p) else 0.0, float(self.r.mean()) if len(self.r) else 0.0,
                float(ap[:, 0].mean()) if len(ap) else 0.0, float(ap[:, 5].mean()) if len(ap) else 0.0, float(ap.mean()) if len(ap) else 0.0]

    def fitness(self):
        return float((np.array(self.mean_results()) * [0.0, 0.0, 0.0, 0.0, 1.0]).sum())  # the fork weights only mAP50-95 (metrics.py:758-761)


class SegmentMetrics:
    """Box and mask metrics side by side (reference SegmentMetrics, metrics.py:909-1029): `box`, `seg`, `keys`, `fitness`, `results_dict`."""

    def __init__(self):
        self.box, self.seg = Metric(), Metric()

    def process(self, tp, tp_m, conf, pred_cls, target_cls):
        self.seg.update(ap_per_class(tp_m, conf, pred_cls, target_cls))
        self.box.update(ap_per_class(tp, conf, pred_cls, target_cls))

    @property
    def keys(self):
        return list(SEG_KEYS)

    def mean_results(self):
        return self.box.mean_results() + self.seg.mean_results()

    @property
    def fitness(self):
        return self.seg.fitness() + self.box.fitness()

    @property
    def results_dict(self):
        return dict(zip(self.keys + ["fitness"], self.mean_results() + [self.fitness]))


POSE_KEYS = SEG_KEYS[:5] + [k.replace("(M)", "(P)") for k in SEG_KEYS[5:]]  # reference metrics.py:1130-1144


class PoseMetrics(SegmentMetrics):
    """Box and pose metrics side by side (reference PoseMetrics, metrics.py:1051-1176): SegmentMetrics with `pose` in the place of `seg`."""

    def __init__(self):
        self.box, self.pose = Metric(), Metric()

    @property
    def seg(self):
        return self.pose

    def process(self, tp, tp_p, conf, pred_cls, target_cls):
        self.pose.update(ap_per_class(tp_p, conf, pred_cls, target_cls))
        self.box.update(ap_per_class(tp, conf, pred_cls, target_cls))

    @property
    def keys(self):
        return list(POSE_KEYS)


OBB_KEYS = ["metrics/precision(B)", "metrics/recall(B)", "metrics/mAP50(B)", "metrics/mAP50-95(B)"]  # reference metrics.py:1268-1270


class OBBMetrics:
    """Rotated-box metrics (reference OBBMetrics, metrics.py:1240-1308): one Metric, `box`, fed with true positives matched on ProbIoU.
    The reference zips its four keys (+ fitness) with the fork's five means (+ fitness), which files mAP75 under "metrics/mAP50-95(B)" and
    mAP50-95 under "fitness"; here every key holds what it names: mAP50-95 is column 4 of `mean_results()`, and fitness (the fork weights
    only mAP50-95) is the same number as the reference's."""

    def __init__(self):
        self.box = Metric()

    def process(self, tp, conf, pred_cls, target_cls):
        self.box.update(ap_per_class(tp, conf, pred_cls, target_cls))

    @property
    def keys(self):
        return list(OBB_KEYS)

    def mean_results(self):
        """[precision, recall, mAP50, mAP75, mAP50-95], as Metric.mean_results."""
        return self.box.mean_results()

    @property
    def fitness(self):
        return self.box.fitness()

    @property
    def results_dict(self):
        m = self.mean_results()
        return dict(zip(self.keys + ["fitness"], [m[0], m[1], m[2], m[4], self.fitness]))


class ClassifyMetrics:
    """top-1 / top-5 accuracy of the classify task (reference utils/metrics.py:1184-1237)."""

    def __init__(self):
        self.top1 = 0
        self.top5 = 0
        self.speed = {"preprocess": 0.0, "inference": 0.0, "loss": 0.0, "postprocess": 0.0}
        self.task = "classify"

    def process(self, targets, pred):
        """targets: list of (n_i,) int32 class tensors; pred: list of (n_i, k) int32 top-k class tensors, best first."""
        pred, targets = np.concatenate([np.asarray(_host(p)) for p in pred]), np.concatenate([np.asarray(_host(t)).reshape(-1) for t in targets])
        correct = (targets[:, None] == pred).astype(np.float32)
        acc = np.stack((correct[:, 0], correct.max(1)), axis=1)  # (top1, top5) accuracy
        n = np.float32(len(acc))
        self.top1, self.top5 = (float(np.float32(v) / n) for v in acc.sum(0, dtype=np.float64))  # fp32 mean of 0 / 1 values: exact sum, one division

    @property
    def fitness(self):
        return (self.top1 + self.top5) / 2

    @property
    def results_dict(self):
        return dict(zip(self.keys + ["fitness"], [self.top1, self.top5, self.fitness]))

    @property
    def keys(self):
        return ["metrics/accuracy_top1", "metrics/accuracy_top5"]

    @property
    def curves(self):
        return []

    @property
    def curves_results(self):
        return []
