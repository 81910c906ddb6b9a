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
