"""Validation loop for the detect task, mirroring the reference's models/yolo/detect/val.py (`DetectionValidator.preprocess` :52-66,
`postprocess` :92-102, `_prepare_batch` :104-115, `_prepare_pred` :117-123, `update_metrics` :125-172, `get_stats` :179-188,
`_process_batch` :209-228) and engine/validator.py (`__call__` loop :107-218, `match_predictions` :222-262).

Device work = the forward on the HIP path + validation-mode NMS (conf 0.001, multi_label, iou 0.7, max_det 300: `ey_nms`); label
scaling, TP matching at the 10 IoU thresholds and AP run on the host in numpy (the reference runs them on the CPU too), through
`utils/metrics.py`.  Same predictions -> same statistics -> same mAP as the reference (pinned by tests/golden/validator_case.npz,
produced by the reference's own update_metrics / get_stats / DetMetrics).

`SegmentationValidator` below does the same for the segment task (models/yolo/segment/val.py): there the predicted masks and their IoU
with the ground truth stay on the device (`ey_process_mask`, `ey_mask_iou`); pinned by tests/golden/segval_case.npz."""
import numpy as np
import torch

from ..utils import metrics, ops

KEYS = ["metrics/precision(B)", "metrics/recall(B)", "metrics/mAP50(B)", "metrics/mAP75(B)", "metrics/mAP50-95(B)"]  # reference DetMetrics.keys (metrics.py:866-868)


def _np(x):
    return x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


def refuse_options(owner, what, **options):
    """The options of a validator that are accepted by name and not built: any that is set raises."""
    for name, on in options.items():
        if on:
            raise NotImplementedError(f"{owner}: {name}=True is not built ({what})")


def batch_offsets(n):
    """per-image counts -> the B+1 offsets of the images' rows in a batch's flat row tensor."""
    return np.concatenate([[0], np.cumsum(n)])


def pair_matrices(launch, n, nl):
    """The [gt x pred] matrices of a batch from ONE launch: `launch(pred_off, gt_off) -> (flat, out_off)` gets the offset tables of the
    images' n[i] predictions and nl[i] labels and returns the flat buffer that holds image i's row-major (nl[i], n[i]) matrix at out_off[i].
    One copy to the host -> list of (nl[i], n[i]) arrays, None where either side is empty."""
    flat, off = launch(batch_offsets(n), batch_offsets(nl))
    host = flat.cpu().numpy()  # the one D2H copy of the batch's matrices
    return [host[off[i]: off[i] + nl[i] * n[i]].reshape(nl[i], n[i]) if n[i] and nl[i] else None for i in range(len(n))]


class BaseValidator:
    """What every task's validator shares: the model behind a facade, the device, the image part of `preprocess`, and the loop."""

    val_options = {}  # val() keywords of the task beyond the common ones, with their defaults (the facade reads this off the class)

    def __init__(self, model, half=False, device=None):
        """model: a task model on its device (fused / dtype set by the caller), or a YOLO facade."""
        self.model = getattr(model, "model", model) if not hasattr(model, "forward_layers") else model
        self.half = half
        self.device = torch.device(device) if device is not None else next(self.model.parameters()).device

    # ---- reference detect/val.py:52-66, classify/val.py:49-54
    def preprocess(self, batch):
        """batch["img"]: (B,3,H,W) uint8 (0..255) or float in [0,1] tensor; the uint8 form is divided by 255 like the reference does."""
        img = batch["img"].to(self.device, non_blocking=True)
        scale = 255.0 if img.dtype == torch.uint8 else 1.0
        img = img.half() if self.half else img.float()
        batch = dict(batch)
        batch["img"] = (img / scale if scale != 1.0 else img).contiguous()
        return batch

    def _forward(self, img):
        return self.model(img)

    @torch.no_grad()
    def __call__(self, dataloader):
        """dataloader: iterable of batch dicts in the task's format (see the class).  Returns the task's results dict."""
        self.init_metrics()
        for batch in dataloader:
            batch = self.preprocess(batch)
            with torch.cuda.device(self.device):  # kernels go to the CURRENT device's stream
                preds = self.postprocess(self._forward(batch["img"]))
                self.update_metrics(preds, batch)
        return self.get_stats()


class DetectionValidator(BaseValidator):
    """Batches: {"img", "cls" (N,1), "bboxes" (N,4 normalised xywh in the network input frame), "batch_idx" (N,), "ori_shape" [B x (h,w)],
    "ratio_pad" [B x ((gain,gain),(padw,padh))] or absent} (the reference's dataset collate format, data/dataset.py); the results dict is the
    reference's DetMetrics.results_dict.

    Two keywords, both off by default, shared by every task with boxes (with both off nothing differs: same launches, copies, results):
    confusion_matrix=True: `self.confusion_matrix` (metrics.ConfusionMatrix, conf 0.25, IoU 0.45 like the reference's) is made by
      init_metrics and fed once per batch: device rows in one ey_match_batch launch, host-array rows image by image in numpy.
    device_match=True: the batch's true positives come from that kernel too (with both keywords it is ONE launch) and the host gets the kept
      rows and their TP bytes in one copy; host-array rows raise ValueError.  `stats` hold the same arrays in the same order either way."""

    val_options = {"confusion_matrix": False, "device_match": False}

    def __init__(self, model, conf=0.001, iou=0.7, max_det=300, half=False, single_cls=False, agnostic_nms=False, device=None, confusion_matrix=False,
                 device_match=False):
        """model: a DetectionModel on its device (fused / dtype set by the caller or by __call__), or a YOLO facade.
        conf None -> 0.001 like the reference (engine/validator.py:100-101)."""
        super().__init__(model, half, device)
        self._cm_on, self.device_match, self._stash = bool(confusion_matrix), bool(device_match), None
        self.conf = 0.001 if conf is None else conf
        self.iou, self.max_det, self.single_cls, self.agnostic_nms = iou, max_det, single_cls, agnostic_nms
        self.iouv = metrics.IOUV
        self.niou = len(self.iouv)
        self.nc = len(self.model.names)
        self.init_metrics()

    # ---- reference val.py:68-87
    def init_metrics(self):
        self.seen = 0
        self.stats = dict(tp=[], conf=[], pred_cls=[], target_cls=[], target_img=[])
        self.results_dict = dict(zip(KEYS + ["fitness"], [0.0] * 6))
        self.box = None
        self.confusion_matrix = metrics.ConfusionMatrix(self.nc, conf=self.conf) if self._cm_on else None  # (reference val.py:77)

    # ---- reference val.py:92-102
    def postprocess(self, preds):
        if not (self._cm_on or self.device_match):
            return ops.non_max_suppression(preds, self.conf, self.iou, multi_label=True, agnostic=self.single_cls or self.agnostic_nms, max_det=self.max_det)
        boxes, count, _ = ops.nms_device(preds, self.conf, self.iou, None, self.single_cls or self.agnostic_nms, self.max_det, multi_label=True)
        return self._kept(boxes, count)  # (what non_max_suppression returns, with the fixed-size pair kept for the matching kernel)

    def _kept(self, boxes, count):
        """NMS's fixed-size (boxes, count) -> the per-image kept rows (one D2H sync for the counts); with a keyword on, the pair is stashed
        for update_metrics."""
        n = count.tolist()
        rows = [boxes[i, :n[i]] for i in range(len(n))]
        if self._cm_on or self.device_match:
            self._stash = (boxes, count, n, rows)
        return rows

    def _device_batch(self, rows):
        """(rows (B, max_det, W) fp32, count (B,) int32, n) on the device for the per-image device rows `rows` -- the pair postprocess stashed
        when they are its rows, else the rows padded -- or None when they are host arrays."""
        if not (len(rows) and all(torch.is_tensor(r) and r.is_cuda for r in rows)):
            return None
        st, self._stash = self._stash, None
        if st is not None and st[3] is rows:
            return st[:3]
        n = [int(r.shape[0]) for r in rows]
        pad = torch.zeros((len(rows), max(max(n), 1), int(rows[0].shape[1])), dtype=torch.float32, device=rows[0].device)
        for i, r in enumerate(rows):
            pad[i, :n[i]] = r
        return pad, torch.tensor(n, dtype=torch.int32, device=pad.device), n

    @staticmethod
    def _xform(pb):
        """padx, pady, gain, w0, h0 of ops.scale_boxes for the image of `_prepare_batch`'s dict pb (ey_match_batch's xform row)."""
        (h1, w1), (h0, w0) = pb["imgsz"], pb["ori_shape"]
        if pb["ratio_pad"] is None:
            gain = min(h1 / h0, w1 / w0)
            pad = (round((w1 - w0 * gain) / 2 - 0.1), round((h1 - h0 * gain) / 2 - 0.1))
        else:
            gain, pad = pb["ratio_pad"][0][0], pb["ratio_pad"][1]
        return [pad[0], pad[1], gain, w0, h0]

    def _match_device(self, dev_batch, pbatches, iou=None, iou_off=None, want_cm=False, want_tp=True):
        """ONE ey_match_batch launch over the batch: the true positives (uint8 (B, max_det, niou) on the device) when want_tp, the confusion
        matrix's increments when want_cm.  iou / iou_off: the flat [gt x pred] matrices of a pair-matrix launch in the place of the boxes."""
        boxes, count, n = dev_batch
        if self.single_cls:
            boxes = boxes.clone()
            boxes[..., 5] = 0
        gt_off = batch_offsets([len(pb["cls"]) for pb in pbatches])
        cls = np.concatenate([pb["cls"] for pb in pbatches]) if pbatches else np.zeros(0, np.float32)
        gt = xform = None
        if iou is None:
            gt = np.concatenate([pb["bbox"].reshape(-1, 4) for pb in pbatches]).astype(np.float32)
            xform = np.asarray([self._xform(pb) for pb in pbatches], np.float32)
        if want_cm:
            return self.confusion_matrix.process_device_batch(boxes, count, gt, cls, gt_off, xform=xform, iou=iou, iou_off=iou_off, iou_n=n,
                                                              iouv=self.iouv if want_tp else None)
        return metrics.match_batch(boxes, gt, cls, self.iouv, iou=iou, count=count, gt_off=gt_off, nc=self.nc, xform=xform, iou_off=iou_off, iou_n=n)

    def _fetch_matched(self, dev_batch, tps, width=6):
        """The kept rows (first `width` columns) and their TP bytes in ONE copy to the host -> (rows per image, per tps entry the per-image
        (n_i, niou) bool arrays)."""
        boxes, count, n = dev_batch
        keep = ops.kept_rows(count, boxes.shape[1])
        host = torch.cat([boxes[keep][:, :width].float()] + [t[keep].float() for t in tps], 1).cpu().numpy()
        off, T = batch_offsets(n), self.niou
        rows = [host[off[i]:off[i + 1], :width] for i in range(len(n))]
        return rows, [[host[off[i]:off[i + 1], width + k * T: width + (k + 1) * T] != 0 for i in range(len(n))] for k in range(len(tps))]

    def _host_rows_only(self, rows):
        """device_match with rows that are host arrays: refused."""
        if self.device_match:
            raise ValueError(f"{type(self).__name__}: device_match=True matches on the device; these rows are host arrays (use the default host route)")

    # ---- reference val.py:104-115: labels of image si -> native (original-image) pixel space
    def _prepare_batch(self, si, batch):
        idx = _np(batch["batch_idx"]).reshape(-1) == si
        cls = _np(batch["cls"]).reshape(-1)[idx].astype(np.float32)
        bbox = _np(batch["bboxes"]).reshape(-1, 4)[idx].astype(np.float32)
        ori_shape = tuple(int(v) for v in batch["ori_shape"][si])
        imgsz = tuple(int(v) for v in batch["img"].shape[2:])
        ratio_pad = batch["ratio_pad"][si] if batch.get("ratio_pad") is not None else None
        if len(cls):
            b = torch.from_numpy(bbox)
            b = ops.xywh2xyxy(b) * torch.tensor(imgsz, dtype=torch.float32)[[1, 0, 1, 0]]  # normalised xywh -> input pixels xyxy
            bbox = ops.scale_boxes(imgsz, b, ori_shape, ratio_pad=ratio_pad).numpy()
        return {"cls": cls, "bbox": bbox.reshape(-1, 4), "ori_shape": ori_shape, "imgsz": imgsz, "ratio_pad": ratio_pad}

    # ---- reference val.py:117-123
    def _prepare_pred(self, pred, pbatch):
        predn = torch.as_tensor(_np(pred), dtype=torch.float32).clone()
        ops.scale_boxes(pbatch["imgsz"], predn[:, :4], pbatch["ori_shape"], ratio_pad=pbatch["ratio_pad"])
        return predn.numpy()

    # ---- reference val.py:209-228
    def _process_batch(self, detections, gt_bboxes, gt_cls):
        return metrics.match_predictions(detections[:, 5], gt_cls, metrics.box_iou(gt_bboxes, detections[:, :4]), self.iouv)

    # ---- reference val.py:125-172 (plots / json / txt saving are out of scope)
    def update_metrics(self, preds, batch):
        if not (self._cm_on or self.device_match):
            return self._image_stats(preds, batch)
        dev_batch = self._device_batch(preds)
        if dev_batch is None:
            self._host_rows_only(preds)
            return self._image_stats(preds, batch, host_cm=True)
        pbatches = [self._prepare_batch(si, batch) for si in range(len(preds))]
        tp = self._match_device(dev_batch, pbatches, want_cm=self._cm_on, want_tp=self.device_match)
        if not self.device_match:
            return self._image_stats(preds, batch, pbatches)
        rows, (tps,) = self._fetch_matched(dev_batch, [tp])
        self._image_stats(rows, batch, pbatches, tps={"tp": tps})

    def _image_stats(self, rows, batch, pbatches=None, tps=None, host_cm=False, **more_tp):
        """The per-image statistics loop of every task with boxes.  rows: per image the kept (n_i, 6+) rows [xyxy, conf, cls, ...] in
        network-input pixels.  pbatches: the images' `_prepare_batch` dicts where the task's batch-wide work made them already.
        more_tp: the task's further true-positive arrays by their `stats` key, each a `f(si, predn, pbatch) -> (n_i, niou) bool` that is
        called for the images that have both predictions and labels.  tps: the true-positive arrays by their `stats` key where the device
        matched the batch already: per key the per-image (n_i, niou) bool arrays (the rows' boxes are then not scaled on the host: `stats`
        take only their conf and cls).  host_cm: feed the confusion matrix image by image, in numpy (reference val.py:146-147,165-166)."""
        keys = ("tp", *more_tp) if tps is None else tuple(tps)
        for si, pred in enumerate(rows):
            self.seen += 1
            pred = _np(pred).astype(np.float32)
            pred = pred.reshape(-1, pred.shape[-1] if pred.ndim == 2 else 6)
            npr = pred.shape[0]
            stat = dict(conf=np.zeros(0, np.float32), pred_cls=np.zeros(0, np.float32), **{k: np.zeros((npr, self.niou), bool) for k in keys})
            pbatch = self._prepare_batch(si, batch) if pbatches is None else pbatches[si]
            cls, bbox = pbatch["cls"], pbatch["bbox"]
            stat["target_cls"] = cls
            stat["target_img"] = np.unique(cls)
            if npr == 0:  # an image with no predictions contributes only when it has labels
                if len(cls):
                    for k in self.stats:
                        self.stats[k].append(stat[k])
                    if host_cm:
                        self.confusion_matrix.process_batch(None, bbox, cls)
                continue
            if self.single_cls:
                pred = pred.copy()
                pred[:, 5] = 0
            predn = self._box_rows(pred, pbatch) if tps is None else pred
            stat["conf"], stat["pred_cls"] = predn[:, 4], predn[:, 5]
            if tps is not None:
                for k in keys:
                    stat[k] = np.asarray(tps[k][si], bool).reshape(npr, self.niou)
            elif len(cls):
                stat["tp"] = self._box_tp(si, predn, pbatch)
                for k, f in more_tp.items():
                    stat[k] = f(si, predn, pbatch)
            if host_cm:
                self.confusion_matrix.process_batch(predn, bbox, cls)
            for k in self.stats:
                self.stats[k].append(stat[k])

    def _box_rows(self, pred, pbatch):
        """The box part of an image's kept rows in original-image pixels: xyxy boxes take the first six columns (what rides behind column 6
        is the task's); a task whose boxes have another format (obb) overrides this."""
        return DetectionValidator._prepare_pred(self, pred[:, :6], pbatch)

    def _box_tp(self, si, predn, pbatch):
        """The box true positives of image si, which has predictions and labels."""
        return self._process_batch(predn, pbatch["bbox"], pbatch["cls"])

    def _gather_stats(self):
        """The accumulated statistics as one array per key, with the label counts per class / per image set aside; None while no prediction
        has matched a label at any threshold (the reference tests the box matches only, detect/val.py:186)."""
        stats = {k: (np.concatenate(v, 0) if v else np.zeros((0, self.niou) if k.startswith("tp") else 0)) for k, v in self.stats.items()}
        self.nt_per_class = np.bincount(stats["target_cls"].astype(int), minlength=self.nc)
        self.nt_per_image = np.bincount(stats["target_img"].astype(int), minlength=self.nc)
        stats.pop("target_img", None)
        return stats if len(stats["tp"]) and stats["tp"].any() else None

    # ---- reference val.py:179-188 + DetMetrics.process / results_dict (metrics.py:850-896)
    def get_stats(self):
        stats = self._gather_stats()
        if stats is not None:
            r = metrics.ap_per_class(stats["tp"], stats["conf"], stats["pred_cls"], stats["target_cls"])
            ap = r["ap"]
            mean = [float(r["p"].mean()) if len(r["p"]) else 0.0, float(r["r"].mean()) if len(r["r"]) else 0.0,
                    float(ap[:, 0].mean()) if len(ap) else 0.0, float(ap[:, 5].mean()) if len(ap) else 0.0, float(ap.mean()) if len(ap) else 0.0]
            self.box = r
            # fitness: the fork weights only mAP50-95 (Metric.fitness, metrics.py:758-761: w = [0, 0, 0, 0, 1])
            self.results_dict = dict(zip(KEYS + ["fitness"], mean + [mean[4]]))
        return self.results_dict

    # ---- convenience kept from round 1: labels as (m,5) [cls, x1,y1,x2,y2] in network-input pixels, no letterbox
    @torch.no_grad()
    def update(self, images, labels):
        B, _, H, W = images.shape
        cls, box, bi = [], [], []
        for i, lab in enumerate(labels):
            lab = np.asarray(lab, np.float32).reshape(-1, 5)
            xy = lab[:, 1:]
            cls.append(lab[:, :1])
            box.append(np.stack([(xy[:, 0] + xy[:, 2]) / 2 / W, (xy[:, 1] + xy[:, 3]) / 2 / H, (xy[:, 2] - xy[:, 0]) / W, (xy[:, 3] - xy[:, 1]) / H], 1))
            bi.append(np.full(len(lab), i, np.float32))
        batch = self.preprocess({"img": images, "cls": np.concatenate(cls), "bboxes": np.concatenate(box), "batch_idx": np.concatenate(bi),
                                 "ori_shape": [(H, W)] * B, "ratio_pad": None})
        with torch.cuda.device(self.device):
            preds = self.postprocess(self.model(batch["img"]))
        self.update_metrics(preds, batch)

    def results(self):
        r = self.get_stats()
        return dict(mp=r[KEYS[0]], mr=r[KEYS[1]], map50=r[KEYS[2]], map75=r[KEYS[3]], map=r[KEYS[4]])


class TwoMetricValidator(DetectionValidator):
    """The tasks that score the boxes and a second quantity of every instance side by side (segment: masks, pose: keypoints): the
    bookkeeping around a metrics object with `box` and that second Metric.  A task names the three class attributes."""

    metrics_cls = None  # metrics.SegmentMetrics or a subclass
    second = None  # the second Metric's name on the metrics object; get_stats mirrors it on the validator next to `box`
    tp_second = None  # its true-positive array's key in `stats` (the keyword of metrics_cls.process)

    def init_metrics(self):
        super().init_metrics()
        self.metrics = self.metrics_cls()
        self.stats = {self.tp_second: [], **self.stats}
        self.results_dict = dict.fromkeys(self.metrics.keys + ["fitness"], 0.0)
        setattr(self, self.second, None)
        self.kept = []

    # ---- reference detect/val.py:179-188 + SegmentMetrics / PoseMetrics .process / results_dict (metrics.py:949-1029)
    def get_stats(self):
        stats = self._gather_stats()
        if stats is not None:
            self.metrics.process(**stats)
            self.box = self.metrics.box
            setattr(self, self.second, getattr(self.metrics, self.second))
        self.results_dict = self.metrics.results_dict
        return self.results_dict


class SegmentationValidator(TwoMetricValidator):
    """Validation loop for the segment task, mirroring the reference's models/yolo/segment/val.py (`preprocess` :39-43, `postprocess` :71-84,
    `_prepare_batch` :86-91, `_prepare_pred` :93-97, `update_metrics` :99-166, `_process_batch` :173-217) with SegmentMetrics.

    Device work per batch: the forward, validation-mode NMS with the mask coefficients riding along (`nms_device`), the masks of ALL images
    at proto resolution in one `ey_process_mask` launch (the reference's default `ops.process_mask(..., upsample=False)`: boxes scaled by
    mw/iw, mh/ih in fp32, s = 1) and the mask IoU of ALL images in one `ey_mask_iou` call.  The masks never leave the device: the host gets the
    kept rows (n, 6), and the [gt x pred] IoU matrices in one copy per batch; matching and AP run in numpy like the detect task.

    batch["masks"]: overlap_mask=True (the reference's default) -> one index map per image, (B, h, w), instance m of an image = the pixels
    equal to m + 1 (m = the label's position within its image), read by the kernel as it is; overlap_mask=False -> (M_total, h, w) 0/1, one
    per label.  Ground truth of another resolution than the predicted masks is resized like the reference does (bilinear F.interpolate of the
    expanded float masks, then > 0.5) with torch on the device before the kernel: a cold path -- the dataset produces masks at proto
    resolution (mask_ratio 4) -- that does materialise the (nl, h, w) stack.

    Host masks (numpy / CPU tensors, `update_metrics(..., pred_masks=[...])` with a validator on the CPU) go through the numpy restatement of
    mask_iou: the route the CPU tests take.

    process_mask_native=True (the reference's `self.process = ops.process_mask_native` branch, segment/val.py:52, which it takes for
    save_json / save_txt): the masks of all images at the network-input resolution in one `ey_process_mask_native` launch (shape = imgsz:
    resized first, cropped by the boxes in input pixels after); the ground truth is resized to them on the cold path above.  It needs
    a validator on the device: on the CPU, where only ready masks are scored, it raises.  save_json, save_txt and plots are not built."""

    metrics_cls, second, tp_second = metrics.SegmentMetrics, "seg", "tp_m"  # (reference segment/val.py:45-53)
    val_options = {"overlap_mask": True, "save_json": False, "save_txt": False, "plots": False, "process_mask_native": False, **DetectionValidator.val_options}

    def __init__(self, model, conf=0.001, iou=0.7, max_det=300, half=False, single_cls=False, agnostic_nms=False, device=None, overlap_mask=True,
                 save_json=False, save_txt=False, plots=False, process_mask_native=False, confusion_matrix=False, device_match=False):
        refuse_options("SegmentationValidator", "COCO json / txt export and plots", save_json=save_json, save_txt=save_txt, plots=plots)
        self.process_mask_native = bool(process_mask_native)
        self.overlap_mask = bool(overlap_mask)
        self.keep_outputs = False  # True: update_metrics appends (rows (n,6+nm), mask bits (n,mh,mw)) per image to self.kept, on the host
        super().__init__(model, conf, iou, max_det, half, single_cls, agnostic_nms, device, confusion_matrix, device_match)
        if self.process_mask_native and self.device.type != "cuda":  # (the host route takes ready masks; the native assembly is the kernel alone)
            raise NotImplementedError(f"SegmentationValidator: process_mask_native=True is built on ey_process_mask_native and this validator is on '{self.device}': "
                                      "there is no CPU path; put the model on the device first (YOLO.val does) or pass device=")

    # ---- reference segment/val.py:39-43 (the masks stay integers: uint8 0/1 stacks, int32 index maps)
    def preprocess(self, batch):
        batch = super().preprocess(batch)
        m = torch.as_tensor(batch["masks"]) if not torch.is_tensor(batch["masks"]) else batch["masks"]
        m = m.to(self.device, non_blocking=True)
        batch["masks"] = (m.to(torch.int32) if self.overlap_mask else (m != 0).to(torch.uint8)).contiguous()
        return batch

    # ---- reference segment/val.py:71-84: (rows (n_i, 6 + nm) per image, proto)
    def postprocess(self, preds):
        boxes, count, _ = ops.nms_device(preds[0], self.conf, self.iou, None, self.single_cls or self.agnostic_nms, self.max_det, nc=self.nc, multi_label=True)
        proto = preds[1][-1] if len(preds[1]) == 3 else preds[1]
        return self._kept(boxes, count), proto  # (the one D2H sync of the NMS)

    # ---- reference segment/val.py:86-91
    def _prepare_batch(self, si, batch):
        pbatch = super()._prepare_batch(si, batch)
        masks = batch["masks"]
        if self.overlap_mask:
            pbatch["masks"] = masks[[si]]
        else:
            idx = _np(batch["batch_idx"]).reshape(-1) == si
            pbatch["masks"] = masks[torch.as_tensor(idx, device=masks.device)] if torch.is_tensor(masks) else np.asarray(masks)[idx]
        return pbatch

    def _batch_pred_masks(self, rows, proto, imgsz):
        """Masks of every image's kept rows at proto resolution, ONE ey_process_mask launch: (N_total, mh, mw) uint8 on the device.  The
        padded row tensor serves as the coefficient "map" (one level, H = rows per image, W = 1, anchor = row number); boxes are in
        network-input pixels (before scale_boxes), scaled to the proto grid like ops.process_mask does (reference ops.py:681-688)."""
        from ..nn import _ops
        from .. import _lib as L
        B, nm, mh, mw = proto.shape
        n = [int(r.shape[0]) for r in rows]
        if sum(n) == 0:
            return torch.empty((0, mh, mw), dtype=torch.uint8, device=proto.device)
        pad = torch.nn.utils.rnn.pad_sequence([r.float() for r in rows], batch_first=True).contiguous()  # (B, max n, 6 + nm)
        C = pad.shape[2]
        coef = torch.as_strided(pad, (B, nm, pad.shape[1], 1), (pad.shape[1] * C, 1, C, C), pad.storage_offset() + 6)
        dev = proto.device
        idx = torch.tensor([[i, j] for i in range(B) for j in range(n[i])], dtype=torch.int32).to(dev)
        ih, iw = imgsz
        if self.process_mask_native:  # (N_total, ih, iw): every image has the network input's shape, so the flat buffer is one stack
            boxes = torch.cat([r[:, :4].float() for r in rows], 0).contiguous()
            flat, _ = _ops.process_mask_native(L.as_nhwc(proto), [coef], idx, boxes, batch_offsets(n), [(ih, iw)] * B)
            return flat.view(sum(n), ih, iw)
        scale = torch.tensor([mw / iw, mh / ih, mw / iw, mh / ih], dtype=torch.float32, device=dev)
        boxes = (torch.cat([r[:, :4].float() for r in rows], 0) * scale).contiguous()
        return _ops.process_mask(L.as_nhwc(proto), [coef], idx, boxes, 1)

    # ---- reference segment/val.py:93-97 (one image; update_metrics assembles the masks of the whole batch at once instead)
    def _prepare_pred(self, pred, pbatch, proto):
        predn = super()._prepare_pred(pred[:, :6], pbatch)
        process = ops.process_mask_native if self.process_mask_native else ops.process_mask
        pred_masks = process(proto, pred[:, 6:], pred[:, :4], shape=pbatch["imgsz"])
        return predn, pred_masks

    @staticmethod
    def _resize_gt(gt, shape):
        """The reference's resize of float 0/1 ground truth to the predicted masks' shape (segment/val.py:210-212): torch plumbing, cold path."""
        g = torch.as_tensor(gt).float()
        g = torch.nn.functional.interpolate(g[None], tuple(shape), mode="bilinear", align_corners=False)[0]
        return (g > 0.5).to(torch.uint8)

    # ---- reference segment/val.py:173-217
    def _process_batch(self, detections, gt_bboxes, gt_cls, pred_masks=None, gt_masks=None, overlap=False, masks=False, iou=None):
        """masks=True: IoU of masks through metrics.mask_iou (device tensors: ey_mask_iou; host arrays: numpy), or `iou` when the caller
        computed the batch's matrices in one launch already."""
        if not masks:
            return super()._process_batch(detections, gt_bboxes, gt_cls)
        if iou is None:
            nl = len(gt_cls)
            if torch.is_tensor(gt_masks) and gt_masks.is_cuda:
                if overlap:
                    gt_masks = (gt_masks.view(1, *gt_masks.shape[-2:]) == torch.arange(1, nl + 1, device=gt_masks.device).view(nl, 1, 1)).to(torch.uint8)
                if tuple(gt_masks.shape[1:]) != tuple(pred_masks.shape[1:]):
                    gt_masks = self._resize_gt(gt_masks, pred_masks.shape[1:])
                iou = _np(metrics.mask_iou(gt_masks.reshape(nl, -1), pred_masks.reshape(pred_masks.shape[0], -1)))
            else:
                g, p = _np(gt_masks), _np(pred_masks)
                if overlap:
                    g = metrics.expand_index_masks(g, nl)
                if tuple(g.shape[1:]) != tuple(p.shape[1:]):
                    g = self._resize_gt(g, p.shape[1:]).numpy()
                iou = metrics.mask_iou(g.reshape(nl, -1), p.reshape(p.shape[0], -1))
        return metrics.match_predictions(detections[:, 5], gt_cls, iou, self.iouv)

    def _batch_mask_ious(self, pred_masks, n, batch, nl):
        """[gt x pred] mask IoU of every image in ONE ey_mask_iou call and one copy to the host: list of (nl_i, n_i) arrays (None where
        either side is empty).  pred_masks: (sum n, mh, mw) uint8 on the device."""
        from ..nn import _ops
        B = len(n)
        launch = self._mask_iou_launch(pred_masks, n, batch, nl)
        return [None] * B if launch is None else pair_matrices(launch, n, nl)

    def _mask_iou_launch(self, pred_masks, n, batch, nl):
        """The `launch(pred_off, gt_off) -> (flat, out_off)` of the batch's ey_mask_iou call, None when no image has both sides."""
        from ..nn import _ops
        B = len(n)
        gt = batch["masks"]
        if not any(a and b for a, b in zip(n, nl)):
            return None
        index = self.overlap_mask
        if not index:  # one mask per label, image after image (the collate order); anything else is gathered into that order
            bi = _np(batch["batch_idx"]).reshape(-1)
            order = np.argsort(bi, kind="stable")
            if not np.array_equal(order, np.arange(len(bi))):
                gt = gt[torch.as_tensor(order, device=gt.device)]
        if tuple(gt.shape[1:]) != tuple(pred_masks.shape[1:]):  # cold path, see the class docstring
            if index:
                gt = torch.cat([(gt[i:i + 1] == torch.arange(1, nl[i] + 1, device=gt.device).view(-1, 1, 1)) for i in range(B)], 0)
                index = False
            gt = self._resize_gt(gt, pred_masks.shape[1:])
        return lambda pred_off, gt_off: _ops.mask_iou(pred_masks, pred_off, gt.contiguous(), gt_off, index=index)[:2]

    # ---- reference segment/val.py:99-166
    def update_metrics(self, preds, batch, pred_masks=None):
        """preds: postprocess's (rows per image, proto).  pred_masks: optional list of per-image (n_i, h, w) 0/1 masks that replaces the
        mask assembly (proto may then be None): host arrays take the numpy route."""
        rows, proto = preds
        B = len(rows)
        ious = [None] * B
        on_device = pred_masks is None
        if on_device:
            n = [int(r.shape[0]) for r in rows]
            bi = _np(batch["batch_idx"]).reshape(-1)
            nl = [int((bi == si).sum()) for si in range(B)]
            imgsz = tuple(int(v) for v in batch["img"].shape[2:])
            all_masks = self._batch_pred_masks(rows, proto, imgsz)
            if self.keep_outputs:
                host, off = all_masks.cpu().numpy(), batch_offsets(n)
                self.kept += [(_np(rows[i]).copy(), host[off[i]:off[i + 1]]) for i in range(B)]
            dev_batch = self._device_batch(rows) if self._cm_on or self.device_match else None
            if dev_batch is not None:  # boxes: one launch for the true positives and the confusion matrix; masks: matrix mode on ey_mask_iou's buffer
                pbatches = [self._prepare_batch(si, batch) for si in range(B)]
                tp = self._match_device(dev_batch, pbatches, want_cm=self._cm_on, want_tp=self.device_match)
                if self.device_match:
                    launch = self._mask_iou_launch(all_masks, n, batch, nl)
                    tp_m = torch.zeros_like(tp)
                    if launch is not None:
                        flat, off = launch(batch_offsets(n), batch_offsets(nl))
                        tp_m = self._match_device(dev_batch, pbatches, iou=flat, iou_off=off)
                    host_rows, (tps, tps_m) = self._fetch_matched(dev_batch, [tp, tp_m])
                    return self._image_stats(host_rows, batch, pbatches, tps={"tp": tps, "tp_m": tps_m})
            ious = self._batch_mask_ious(all_masks, n, batch, nl)
        elif self._cm_on or self.device_match:
            self._host_rows_only(rows)

        def tp_m(si, predn, pbatch):
            return self._process_batch(predn, pbatch["bbox"], pbatch["cls"], None if on_device else pred_masks[si], pbatch["masks"], self.overlap_mask,
                                       masks=True, iou=ious[si])

        self._image_stats(rows, batch, host_cm=self._cm_on and not on_device, tp_m=tp_m)

    def update(self, images, labels):
        raise NotImplementedError("SegmentationValidator: the (images, labels) convenience of the detect task carries no masks; call it with batches")


class PoseValidator(TwoMetricValidator):
    """Validation loop for the pose task, mirroring the reference's models/yolo/pose/val.py (`init_metrics` :77-84, `_prepare_batch` :86-96,
    `_prepare_pred` :98-104, `update_metrics` :106-157, `_process_batch` :159-197) with PoseMetrics.

    Device work per batch: the forward WITHOUT the (B, nk, A) keypoint decode (Pose.forward(decode_kpts=False)), validation-mode multi-label
    NMS on the boxes and classes, the keypoints of the kept rows by anchor index (`ey_kpts_decode_rows`), their scaling to the original
    images as one expression over the batch, and the OKS of ALL images in one `ey_kpt_iou` call.  The host gets the kept rows and the
    [gt x pred] matrices in one copy each; matching and AP run in numpy like the detect task.

    batch["keypoints"]: (M_total, K, ndim) normalised to the network input, gathered per image through batch_idx.  sigma = OKS_SIGMA for
    kpt_shape [17, 3], else 1/K; kpt_shape comes from the model's head (datasets are not part of this build).  Host predictions
    (`update_metrics((rows, kpts), batch)` with numpy arrays / CPU tensors) go through the numpy restatement of kpt_iou: the route the CPU
    tests take.  save_json, save_txt and plots are not built."""

    metrics_cls, second, tp_second = metrics.PoseMetrics, "pose", "tp_p"
    val_options = {"save_json": False, "save_txt": False, "plots": False, **DetectionValidator.val_options}

    def __init__(self, model, conf=0.001, iou=0.7, max_det=300, half=False, single_cls=False, agnostic_nms=False, device=None, save_json=False, save_txt=False,
                 plots=False, confusion_matrix=False, device_match=False):
        refuse_options("PoseValidator", "COCO json / txt export and plots", save_json=save_json, save_txt=save_txt, plots=plots)
        self.keep_outputs = False  # True: update_metrics appends (rows (n,6), keypoints (n,K,ndim) in input pixels) per image to self.kept, on the host
        super().__init__(model, conf, iou, max_det, half, single_cls, agnostic_nms, device, confusion_matrix, device_match)

    # ---- reference pose/val.py:77-84
    def init_metrics(self):
        super().init_metrics()
        self.kpt_shape = [int(v) for v in self.model.model[-1].kpt_shape]
        nkpt = self.kpt_shape[0]
        self.sigma = metrics.OKS_SIGMA if self.kpt_shape == [17, 3] else np.ones(nkpt) / nkpt

    # ---- reference pose/val.py:64-75 + the keypoints of the kept rows: (rows (n_i, 6) per image, keypoints (B, max_det, K, ndim) in input pixels)
    def postprocess(self, preds):
        from ..nn import _ops
        y, (_, maps) = preds
        head = self.model.model[-1]
        boxes, count, index = ops.nms_device(y, self.conf, self.iou, None, self.single_cls or self.agnostic_nms, self.max_det, nc=self.nc, multi_label=True)
        kpts = _ops.kpts_decode_rows(head.kpt_levels(maps), head.kpt_shape, index, count)
        return self._kept(boxes, count), kpts  # (the one D2H sync of the NMS)

    def _forward(self, img):
        head = self.model.model[-1]
        was = head.decode_kpts
        head.decode_kpts = False
        try:
            return self.model(img)
        finally:
            head.decode_kpts = was

    # ---- reference pose/val.py:86-96
    def _prepare_batch(self, si, batch):
        pbatch = super()._prepare_batch(si, batch)
        idx = _np(batch["batch_idx"]).reshape(-1) == si
        kpts = torch.as_tensor(_np(batch["keypoints"]), dtype=torch.float32)[torch.as_tensor(idx)].clone()
        h, w = pbatch["imgsz"]
        kpts[..., 0] *= w
        kpts[..., 1] *= h
        pbatch["kpts"] = ops.scale_coords(pbatch["imgsz"], kpts, pbatch["ori_shape"], ratio_pad=pbatch["ratio_pad"]).numpy()
        return pbatch

    # ---- reference pose/val.py:159-197
    def _process_batch(self, detections, gt_bboxes, gt_cls, pred_kpts=None, gt_kpts=None, iou=None):
        """pred_kpts / gt_kpts given: OKS through metrics.kpt_iou (host arrays: numpy), or `iou` when the caller computed the batch's matrices
        in one launch already; otherwise box IoU."""
        if pred_kpts is None and gt_kpts is None and iou is None:
            return super()._process_batch(detections, gt_bboxes, gt_cls)
        if iou is None:
            iou = _np(metrics.kpt_iou(gt_kpts, pred_kpts, self._gt_area(gt_bboxes), self.sigma))
        return metrics.match_predictions(detections[:, 5], gt_cls, iou, self.iouv)

    @staticmethod
    def _gt_area(gt_bboxes):
        """(m, 4) xyxy ground-truth boxes -> the (m,) object areas OKS normalises by (reference pose/val.py:187)."""
        return (ops.xyxy2xywh(torch.as_tensor(gt_bboxes))[:, 2:].prod(1) * 0.53).numpy()  # 0.53: the COCO keypoint evaluation's box-to-area factor

    def _scale_pred_kpts(self, kpts, pbatches):
        """pose/val.py:98-104 for every image at once, on the tensor's device: (B, max_det, K, ndim) input pixels -> original-image pixels
        (scale_coords per image: - pad, / gain, clip), one expression over the batch."""
        B = kpts.shape[0]
        geo = np.zeros((B, 5), np.float32)
        for i, pb in enumerate(pbatches):
            if pb["ratio_pad"] is None:
                gain = min(pb["imgsz"][0] / pb["ori_shape"][0], pb["imgsz"][1] / pb["ori_shape"][1])
                pad = (pb["imgsz"][1] - pb["ori_shape"][1] * gain) / 2, (pb["imgsz"][0] - pb["ori_shape"][0] * gain) / 2
            else:
                gain, pad = pb["ratio_pad"][0][0], pb["ratio_pad"][1]
            geo[i] = [pad[0], pad[1], gain, pb["ori_shape"][1], pb["ori_shape"][0]]
        g = torch.from_numpy(geo).to(kpts.device).view(B, 5, 1, 1)
        out = kpts.clone()
        zero = torch.zeros((), dtype=torch.float32, device=kpts.device)
        out[..., 0] = torch.minimum(torch.maximum((kpts[..., 0] - g[:, 0]) / g[:, 2], zero), g[:, 3])
        out[..., 1] = torch.minimum(torch.maximum((kpts[..., 1] - g[:, 1]) / g[:, 2], zero), g[:, 4])
        return out

    # ---- reference pose/val.py:106-157
    def update_metrics(self, preds, batch):
        """preds: postprocess's (rows per image, keypoints).  keypoints: a (B, max_det, K, ndim) tensor (device: the one-launch route) or a
        list of per-image (n_i, K, ndim) host arrays, in network-input pixels."""
        from ..nn import _ops
        rows, kpts = preds
        B = len(rows)
        pbatches = [self._prepare_batch(si, batch) for si in range(B)]
        K = self.kpt_shape[0]
        on_device = torch.is_tensor(kpts) and kpts.is_cuda
        ious = [None] * B
        flags = self._cm_on or self.device_match
        if flags and not on_device:
            self._host_rows_only(rows)
        if on_device:
            launch = None
            n, nl = [int(r.shape[0]) for r in rows], [len(pb["cls"]) for pb in pbatches]
            scaled = self._scale_pred_kpts(kpts, pbatches)
            if self.keep_outputs:
                host = kpts.cpu().numpy()
                self.kept += [(_np(rows[i]).copy(), host[i, :n[i]]) for i in range(B)]
            if any(a and b for a, b in zip(n, nl)):
                dev = kpts.device
                pk = scaled[ops.kept_rows(torch.tensor(n, device=dev), kpts.shape[1])].contiguous()  # (sum n, K, ndim), image after image
                gk = torch.from_numpy(np.concatenate([pb["kpts"].reshape(-1, K, 3) for pb in pbatches], 0)).to(dev)
                ar = torch.from_numpy(np.concatenate([self._gt_area(pb["bbox"]) for pb in pbatches]).astype(np.float32)).to(dev)
                sg = torch.from_numpy(np.asarray(self.sigma, np.float32)).to(dev)
                launch = lambda pred_off, gt_off: _ops.kpt_iou(pk, pred_off, gk, gt_off, ar, sg)  # noqa: E731
            dev_batch = self._device_batch(rows) if flags else None
            if dev_batch is not None:  # boxes: one launch for the true positives and the confusion matrix; keypoints: matrix mode on ey_kpt_iou's buffer
                tp = self._match_device(dev_batch, pbatches, want_cm=self._cm_on, want_tp=self.device_match)
                if self.device_match:
                    tp_p = torch.zeros_like(tp)
                    if launch is not None:
                        flat, off = launch(batch_offsets(n), batch_offsets(nl))
                        tp_p = self._match_device(dev_batch, pbatches, iou=flat, iou_off=off)
                    host_rows, (tps, tps_p) = self._fetch_matched(dev_batch, [tp, tp_p])
                    return self._image_stats(host_rows, batch, pbatches, tps={"tp": tps, "tp_p": tps_p})
            if launch is not None:
                ious = pair_matrices(launch, n, nl)

        def tp_p(si, predn, pbatch):
            if on_device:
                return self._process_batch(predn, pbatch["bbox"], pbatch["cls"], iou=ious[si])
            pk = torch.as_tensor(_np(kpts[si]), dtype=torch.float32)[:len(predn)].reshape(len(predn), K, -1).clone()
            ops.scale_coords(pbatch["imgsz"], pk, pbatch["ori_shape"], ratio_pad=pbatch["ratio_pad"])
            return self._process_batch(predn, pbatch["bbox"], pbatch["cls"], pk.numpy(), pbatch["kpts"])

        self._image_stats(rows, batch, pbatches, host_cm=self._cm_on and not on_device, tp_p=tp_p)

    def update(self, images, labels):
        raise NotImplementedError("PoseValidator: the (images, labels) convenience of the detect task carries no keypoints; call it with batches")


class OBBValidator(DetectionValidator):
    """Validation loop for the obb task, mirroring the reference's models/yolo/obb/val.py (`postprocess` :39-51, `_process_batch` :53-80,
    `_prepare_batch` :82-93, `_prepare_pred` :95-101) with OBBMetrics.  The facade has no default validator for the task (the plain
    `val(loader)` refusal is pinned): it is handed in by name, `model.val(loader, validator=OBBValidator)`.

    Device work per batch: the forward, validation-mode rotated NMS (`ey_nms_rotated_ml`: every (anchor, class) score above conf is a
    candidate, fast-NMS on ProbIoU) and the ProbIoU of ALL images' labels against their kept rows in one `ey_probiou_batch` call.  The host
    gets the kept rows (n, 7) = x, y, w, h, conf, cls, angle and the [gt x pred] matrices in one copy per batch; scaling to the original
    images, matching and AP run on the host like the detect task.

    batch["bboxes"]: (N, 5) = xywh normalised to the network input plus the angle in radians.  Host predictions (`update_metrics(rows,
    batch)` with a validator on the CPU) go through the numpy restatement metrics.probiou_host: the route the CPU tests take.  save_json
    (the DOTA export), save_txt and plots are not built."""

    val_options = {"save_json": False, "save_txt": False, "plots": False, **DetectionValidator.val_options}

    def __init__(self, model, conf=0.001, iou=0.7, max_det=300, half=False, single_cls=False, agnostic_nms=False, device=None, save_json=False, save_txt=False,
                 plots=False, confusion_matrix=False, device_match=False):
        refuse_options("OBBValidator", "DOTA json / txt export and plots", save_json=save_json, save_txt=save_txt, plots=plots)
        super().__init__(model, conf, iou, max_det, half, single_cls, agnostic_nms, device, confusion_matrix, device_match)

    def init_metrics(self):
        super().init_metrics()
        self.metrics = metrics.OBBMetrics()
        self.results_dict = dict.fromkeys(self.metrics.keys + ["fitness"], 0.0)
        self._ious = None

    # ---- reference obb/val.py:39-51: rows (n_i, 7) per image
    def postprocess(self, preds):
        rows, count, _ = ops.nms_rotated_multi_label(preds, self.conf, self.iou, None, self.single_cls or self.agnostic_nms, self.max_det, nc=self.nc)
        return self._kept(rows, count)  # (the one D2H sync of the NMS)

    # ---- reference obb/val.py:82-93: labels of image si -> native (original-image) pixel space, xywh + angle
    def _prepare_batch(self, si, batch):
        idx = _np(batch["batch_idx"]).reshape(-1) == si
        cls = _np(batch["cls"]).reshape(-1)[idx].astype(np.float32)
        bbox = _np(batch["bboxes"]).reshape(-1, 5)[idx].astype(np.float32)
        ori_shape = tuple(int(v) for v in batch["ori_shape"][si])
        imgsz = tuple(int(v) for v in batch["img"].shape[2:])
        ratio_pad = batch["ratio_pad"][si] if batch.get("ratio_pad") is not None else None
        if len(cls):
            b = torch.from_numpy(bbox.copy())
            b[..., :4] *= torch.tensor(imgsz, dtype=torch.float32)[[1, 0, 1, 0]]
            bbox = ops.scale_boxes(imgsz, b, ori_shape, ratio_pad=ratio_pad, xywh=True).numpy()
        return {"cls": cls, "bbox": bbox.reshape(-1, 5), "ori_shape": ori_shape, "imgsz": imgsz, "ratio_pad": ratio_pad}

    # ---- reference obb/val.py:95-101
    def _prepare_pred(self, pred, pbatch):
        predn = torch.as_tensor(_np(pred), dtype=torch.float32).clone()
        ops.scale_boxes(pbatch["imgsz"], predn[:, :4], pbatch["ori_shape"], ratio_pad=pbatch["ratio_pad"], xywh=True)
        return predn.numpy()

    def _box_rows(self, pred, pbatch):
        return self._prepare_pred(pred[:, :7], pbatch)

    # ---- reference obb/val.py:53-80
    def _process_batch(self, detections, gt_bboxes, gt_cls, iou=None):
        """iou: the image's [gt x pred] ProbIoU matrix where the caller computed the batch's in one launch already."""
        if iou is None:
            iou = metrics.probiou_host(gt_bboxes, np.concatenate([detections[:, :4], detections[:, -1:]], 1))
        return metrics.match_predictions(detections[:, 5], gt_cls, iou, self.iouv)

    def _box_tp(self, si, predn, pbatch):
        return self._process_batch(predn, pbatch["bbox"], pbatch["cls"], iou=None if self._ious is None else self._ious[si])

    # ---- reference detect/val.py:125-172 with the ProbIoU of the whole batch in one launch
    def update_metrics(self, preds, batch):
        """preds: postprocess's rows per image; device tensors take the one-launch route, host arrays the numpy one."""
        from ..nn import _ops
        B = len(preds)
        pbatches = [self._prepare_batch(si, batch) for si in range(B)]
        self._ious = None
        flags = self._cm_on or self.device_match
        dev_batch = self._device_batch(preds) if flags else None
        if flags and dev_batch is None:
            self._host_rows_only(preds)
        host_cm, tps = self._cm_on and dev_batch is None, None
        if B and all(torch.is_tensor(r) and r.is_cuda for r in preds):
            n, nl = [int(r.shape[0]) for r in preds], [len(pb["cls"]) for pb in pbatches]
            launch, dev = None, preds[0].device
            if any(a and b for a, b in zip(n, nl)):
                host = torch.cat([r.float() for r in preds], 0).cpu().numpy()  # the one D2H copy of the batch's rows
                off = batch_offsets(n)
                preds = [host[off[i]:off[i + 1]] for i in range(B)]
                scaled = [self._prepare_pred(preds[i], pbatches[i])[:, [0, 1, 2, 3, 6]] for i in range(B)]
                pk = torch.from_numpy(np.ascontiguousarray(np.concatenate(scaled, 0), np.float32)).to(dev)
                gk = torch.from_numpy(np.ascontiguousarray(np.concatenate([pb["bbox"] for pb in pbatches], 0), np.float32)).to(dev)
                launch = lambda pred_off, gt_off: _ops.probiou_batch(pk, pred_off, gk, gt_off)  # noqa: E731
            with torch.cuda.device(dev):
                if dev_batch is not None:  # true positives and confusion matrix from ONE launch in matrix mode, on the ProbIoU buffer
                    flat, off = launch(batch_offsets(n), batch_offsets(nl)) if launch is not None else (torch.zeros(1, dtype=torch.float32, device=dev), [0] * B)
                    tp = self._match_device(dev_batch, pbatches, iou=flat, iou_off=off, want_cm=self._cm_on, want_tp=self.device_match)
                    if self.device_match:
                        host = torch.cat([tp[i, :n[i]] for i in range(B)], 0).cpu().numpy()  # (the rows came to the host above, for their scaling)
                        o = batch_offsets(n)
                        tps = {"tp": [host[o[i]:o[i + 1]] != 0 for i in range(B)]}
                        if launch is None:  # (the rows did not come to the host above: one copy of them here)
                            hr = torch.cat([r.float() for r in preds], 0).cpu().numpy()
                            preds = [hr[o[i]:o[i + 1]] for i in range(B)]
                elif launch is not None:
                    self._ious = pair_matrices(launch, n, nl)
        try:
            self._image_stats(preds, batch, pbatches, tps=tps, host_cm=host_cm)
        finally:
            self._ious = None

    # ---- reference detect/val.py:179-188 + OBBMetrics.process / results_dict (metrics.py:1252-1298)
    def get_stats(self):
        stats = self._gather_stats()
        if stats is not None:
            self.metrics.process(**stats)
            self.box = self.metrics.box
        self.results_dict = self.metrics.results_dict
        return self.results_dict

    def update(self, images, labels):
        raise NotImplementedError("OBBValidator: the (images, labels) convenience of the detect task carries no angles; call it with batches")

    def results(self):
        raise NotImplementedError("OBBValidator: results() is the detect task's summary; read get_stats() / results_dict")


class ClassificationValidator(BaseValidator):
    """Validation loop for the classify task, mirroring the reference's models/yolo/classify/val.py (`init_metrics` :41-47, `preprocess`
    :49-54, `update_metrics` :56-60, `postprocess` :74-76, `get_stats` :78-81) with ClassifyMetrics.

    Batches are {"img": (B,3,H,W) float in [0,1] or uint8 0..255, "cls": (B,) class indices}.  Device work per batch: the forward; the top
    min(nc, 5) classes come from the head's kernel (ey_classify_linear_softmax; equal probabilities rank the lower class first, where the
    reference's argsort is unspecified) and reach the host as ONE copy of a (B, 5) int32 tensor.  Host predictions (`update_metrics(probs,
    batch)` with a numpy array / CPU tensor of probabilities) are ranked by the same rule on the host: the route the CPU tests take.
    plots=True raises.  confusion_matrix=True: `self.confusion_matrix` (metrics.ConfusionMatrix, task "classify": (nc, nc), row = predicted,
    column = true) is fed with the top-1 class of every sample from the copy the batch makes anyway (reference classify/val.py:44,83)."""

    val_options = {"plots": False, "confusion_matrix": False}

    def __init__(self, model, conf=0.001, iou=0.7, max_det=300, half=False, single_cls=False, agnostic_nms=False, device=None, plots=False,
                 confusion_matrix=False):
        refuse_options("ClassificationValidator", "sample plots", plots=plots)
        self._cm_on = bool(confusion_matrix)
        super().__init__(model, half, device)
        self.metrics = metrics.ClassifyMetrics()
        self.init_metrics()

    def init_metrics(self):
        self.names = self.model.names
        self.nc = len(self.names)
        self.pred, self.targets = [], []
        self.confusion_matrix = metrics.ConfusionMatrix(self.nc, task="classify") if self._cm_on else None
        self.results_dict = dict(zip(self.metrics.keys + ["fitness"], [0.0] * 3))

    def postprocess(self, preds):
        """-> the (B, min(nc, 5)) int32 top classes of the forward that just ran (device tensor); what the forward returned is not used."""
        return self.model.model[-1].top5[0]

    @staticmethod
    def rank(probs, n5):
        """host form of the kernel's ranking: descending probability, equal probabilities by ascending class index -> (B, n5) int32."""
        p = _np(probs).astype(np.float32)
        return np.argsort(-p, axis=1, kind="stable")[:, :n5].astype(np.int32)

    def update_metrics(self, preds, batch):
        n5 = min(self.nc, 5)
        if torch.is_tensor(preds) and preds.dtype == torch.int32:
            top = preds[:, :n5].cpu().numpy()  # the one D2H copy of the batch
        else:
            top = self.rank(preds[0] if isinstance(preds, (list, tuple)) else preds, n5)
        self.pred.append(top)
        self.targets.append(_np(batch["cls"]).reshape(-1).astype(np.int32))
        if self.confusion_matrix is not None:
            self.confusion_matrix.process_cls_preds(self.pred[-1:], self.targets[-1:])

    def get_stats(self):
        self.metrics.process(self.targets, self.pred)
        self.results_dict = self.metrics.results_dict
        return self.results_dict


class FastSAMValidator(SegmentationValidator):
    """SegmentationValidator under its FastSAM name (reference models/fastsam/val.py:7-40: the same validator with the task fixed to
    "segment" and the plots, which are not built here at all, switched off)."""
