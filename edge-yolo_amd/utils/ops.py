"""Post-processing of the detection path, mirroring the reference's ultralytics/utils/ops.py:
`make_divisible` (:130-143), `non_max_suppression` (:167-316), `xywh2xyxy` (:416-433), `scale_boxes` (:92-127),
`clip_boxes` (:319-338), `crop_mask` (:644-660), `process_mask` (:663-693), `process_mask_native` (:696-713), `nms_rotated` (:146-164), `xywhr2xyxyxyxy` (:556-584),
`regularize_rboxes` (:775-790), `masks2segments` (:793-821).  NMS and mask assembly run in the HIP library (ey_nms, ey_nms_rotated, ey_process_mask, ey_process_mask_native, ey_mask_contours); there is no
torch/torchvision fallback."""
import math

import torch


def make_divisible(x, divisor):
    if isinstance(divisor, torch.Tensor):
        divisor = int(divisor.max())
    return math.ceil(x / divisor) * divisor


def xywh2xyxy(x):
    assert x.shape[-1] == 4, f"input shape last dimension expected 4 but input shape is {x.shape}"
    y = torch.empty_like(x)
    xy, wh = x[..., :2], x[..., 2:] / 2
    y[..., :2] = xy - wh
    y[..., 2:] = xy + wh
    return y


def clip_boxes(boxes, shape):
    boxes[..., 0] = boxes[..., 0].clamp(0, shape[1])
    boxes[..., 1] = boxes[..., 1].clamp(0, shape[0])
    boxes[..., 2] = boxes[..., 2].clamp(0, shape[1])
    boxes[..., 3] = boxes[..., 3].clamp(0, shape[0])
    return boxes


def kept_rows(count, max_det):
    """(B, max_det) bool, on count's device: which rows of a fixed-size (B, max_det, ...) NMS output exist, given the (B,) kept counts."""
    return torch.arange(max_det, device=count.device)[None, :] < count[:, None]


def scale_boxes(img1_shape, boxes, img0_shape, ratio_pad=None, padding=True, xywh=False):
    """Rescale xyxy boxes from the network input shape to the original image shape (reference :92-127)."""
    if ratio_pad is None:
        gain = min(img1_shape[0] / img0_shape[0], img1_shape[1] / img0_shape[1])
        pad = (round((img1_shape[1] - img0_shape[1] * gain) / 2 - 0.1), round((img1_shape[0] - img0_shape[0] * gain) / 2 - 0.1))
    else:
        gain, pad = ratio_pad[0][0], ratio_pad[1]
    if padding:
        boxes[..., 0] -= pad[0]
        boxes[..., 1] -= pad[1]
        if not xywh:
            boxes[..., 2] -= pad[0]
            boxes[..., 3] -= pad[1]
    boxes[..., :4] /= gain
    return clip_boxes(boxes, img0_shape)


def xyxy2xywh(x):
    """(..., 4) x1,y1,x2,y2 -> centre x, centre y, width, height (reference utils/ops.py:384-402)."""
    y = torch.empty_like(x) if isinstance(x, torch.Tensor) else x.copy()
    y[..., 0] = (x[..., 0] + x[..., 2]) / 2
    y[..., 1] = (x[..., 1] + x[..., 3]) / 2
    y[..., 2] = x[..., 2] - x[..., 0]
    y[..., 3] = x[..., 3] - x[..., 1]
    return y


def clip_coords(coords, shape):
    """Clip point coordinates (..., >= 2) to the image (h, w), in place (reference utils/ops.py:341-358)."""
    if isinstance(coords, torch.Tensor):
        coords[..., 0] = coords[..., 0].clamp(0, shape[1])
        coords[..., 1] = coords[..., 1].clamp(0, shape[0])
    else:  # numpy
        coords[..., 0] = coords[..., 0].clip(0, shape[1])
        coords[..., 1] = coords[..., 1].clip(0, shape[0])
    return coords


def scale_coords(img1_shape, coords, img0_shape, ratio_pad=None, normalize=False, padding=True):
    """Rescale point coordinates (x, y in the first two entries of the last axis) from img1_shape to img0_shape, in place (reference
    utils/ops.py:740-772; unlike scale_boxes the padding is not rounded)."""
    if ratio_pad is None:
        gain = min(img1_shape[0] / img0_shape[0], img1_shape[1] / img0_shape[1])
        pad = (img1_shape[1] - img0_shape[1] * gain) / 2, (img1_shape[0] - img0_shape[0] * gain) / 2
    else:
        gain, pad = ratio_pad[0][0], ratio_pad[1]
    if padding:
        coords[..., 0] -= pad[0]
        coords[..., 1] -= pad[1]
    coords[..., 0] /= gain
    coords[..., 1] /= gain
    coords = clip_coords(coords, img0_shape)
    if normalize:
        coords[..., 0] /= img0_shape[1]
        coords[..., 1] /= img0_shape[0]
    return coords


_CLASS_TENSORS = {}


def _end2end_filter(prediction, conf_thres, classes, max_det):
    """Output of an end2end head, (B, k, 6) rows [x1,y1,x2,y2,score,class] (reference ops.py:224-228): no suppression, only
    `pred[pred[:, 4] > conf][:max_det]` and then the class filter, here on fixed-size tensors (graph-capturable): kept rows are moved
    to the front in their order, the rest zeroed.  Returns (boxes (B,max_det,6), count (B,) int32, index (B,max_det) int32 = source row)."""
    p = prediction.float()
    B, K, _ = p.shape
    keep = p[..., 4] > conf_thres
    keep &= (keep.cumsum(1) - 1) < max_det
    if classes is not None:
        key = (tuple(classes), p.device)
        if key not in _CLASS_TENSORS:  # uploaded once per filter (never inside a captured graph after the first, eager, call)
            _CLASS_TENSORS[key] = torch.as_tensor(list(classes), dtype=torch.float32, device=p.device)
        keep &= (p[..., 5:6] == _CLASS_TENSORS[key]).any(-1)
    order = torch.sort((~keep).to(torch.uint8), dim=1, stable=True).indices  # kept rows first, original (descending score) order
    n = min(K, max_det)
    boxes = torch.zeros((B, max_det, 6), dtype=torch.float32, device=p.device)
    index = torch.full((B, max_det), -1, dtype=torch.int32, device=p.device)
    sel = order[:, :n]
    ok = torch.gather(keep, 1, sel)
    boxes[:, :n] = torch.gather(p, 1, sel[..., None].expand(-1, -1, 6)) * ok[..., None]
    index[:, :n] = torch.where(ok, sel.to(torch.int32), index[:, :n])
    return boxes, keep.sum(1).to(torch.int32), index


_CLASS_MASKS = {}


def _class_mask(classes, nc, device):
    """uint8 [nc] class-filter mask on `device`, uploaded once per (classes, nc, device): the first, eager, call of a predictor builds it, so
    nothing is copied from the host inside a captured graph (as `_CLASS_TENSORS` above).  The heads' fused decode takes its mask from here
    too (Detect._class_mask); a WorldDetect vocabulary change moves `nc` and with it the key."""
    if classes is None:
        return None
    key = (tuple(classes), int(nc), device)
    if key not in _CLASS_MASKS:
        mask = torch.zeros(nc, dtype=torch.uint8)
        mask[torch.as_tensor(list(classes), dtype=torch.long)] = 1
        _CLASS_MASKS[key] = mask.to(device)
    return _CLASS_MASKS[key]


def _nms_device_rotated(prediction, conf_thres, iou_thres, classes, agnostic, max_det, nc, max_nms, max_wh, multi_label):
    """nms_device(rotated=True): (B,4+nc+1,A) predictions of an OBB head (xywh, class scores, angle) -> (rows (B,max_det,7) = x,y,w,h,conf,
    cls,angle, count (B,), index (B,max_det)) on ey_nms_rotated (fast-NMS on ProbIoU, reference ops.py:146-164,289-293)."""
    from ..nn import _ops
    assert 0 <= conf_thres <= 1, f"Invalid Confidence threshold {conf_thres}, valid values are between 0.0 and 1.0"
    assert 0 <= iou_thres <= 1, f"Invalid IoU {iou_thres}, valid values are between 0.0 and 1.0"
    if isinstance(prediction, _ops.Candidates):
        raise ValueError("nms_device(rotated=True) takes the prediction tensor; fused candidates are axis-aligned")
    if not nc:
        # the reference's default, nc = channels - 4 (ops.py:231), scores the angle row as one more class; its OBB predictor and validator
        # always pass nc (obb/predict.py:38).  That nc-less form is not built
        raise NotImplementedError("rotated NMS needs nc= (the number of classes: the prediction is 4 + nc + 1 angle channels)")
    if prediction.shape[1] - nc - 4 != 1:
        raise ValueError(f"nms_device(rotated=True): nc={nc} but the prediction has {prediction.shape[1]} channels (4 + nc + 1 angle expected)")
    if multi_label and nc > 1:
        raise NotImplementedError("rotated NMS with multi_label=True (the validation regime, one candidate per (anchor, class)) is not served by this "
                                  "entry point, whose single-label (predict) form is pinned; call ops.nms_rotated_multi_label (ey_nms_rotated_ml)")
    with torch.cuda.device(prediction.device):  # launches go to the current device's stream (_lib.stream)
        p = prediction.float().contiguous()
        return _ops.nms_rotated(p, conf_thres, iou_thres, max_det, max_nms, max_wh, agnostic, _class_mask(classes, nc, p.device))


def nms_rotated_multi_label(prediction, conf_thres=0.25, iou_thres=0.45, classes=None, agnostic=False, max_det=300, nc=0, max_nms=30000, max_wh=7680):
    """The reference's non_max_suppression(..., multi_label=True, rotated=True) (ops.py:270-297; what its OBBValidator runs, obb/val.py:39-51)
    on ey_nms_rotated_ml: (B,4+nc+1,A) predictions of an OBB head -> (rows (B,max_det,7) = x,y,w,h,conf,cls,angle, count (B,), index
    (B,max_det) = anchor of each row), fixed sizes, no host synchronisation.  Every (anchor, class) score above conf_thres is a candidate, so
    an anchor can give several rows; order is descending score, equal scores by ascending anchor * nc + class (the reference's argsort leaves
    ties unspecified); the max_nms best go through fast-NMS on ProbIoU.  nc is required, as for nms_device(rotated=True)."""
    from ..nn import _ops
    assert 0 <= conf_thres <= 1, f"Invalid Confidence threshold {conf_thres}, valid values are between 0.0 and 1.0"
    assert 0 <= iou_thres <= 1, f"Invalid IoU {iou_thres}, valid values are between 0.0 and 1.0"
    if isinstance(prediction, (list, tuple)):
        prediction = prediction[0]
    if not nc:
        raise NotImplementedError("rotated NMS needs nc= (the number of classes: the prediction is 4 + nc + 1 angle channels)")
    if prediction.dim() != 3 or prediction.shape[1] - nc - 4 != 1:
        raise ValueError(f"nms_rotated_multi_label: nc={nc} but the prediction has shape {tuple(prediction.shape)} ((B, 4 + nc + 1 angle, A) expected)")
    with torch.cuda.device(prediction.device):  # launches go to the current device's stream (_lib.stream)
        p = prediction.float().contiguous()
        return _ops.nms_rotated_ml(p, conf_thres, iou_thres, max_det, max_nms, max_wh, agnostic, _class_mask(classes, nc, p.device))


def nms_rotated(boxes, scores, threshold=0.45):
    """Reference signature (ops.py:146-164): boxes (N,5) xywhr, scores (N,) -> indices of the kept boxes in descending score order
    (equal scores: lower index first), fast-NMS on ProbIoU through ey_nms_rotated.  Device tensors; one host read of the count."""
    n = int(boxes.shape[0])
    if n == 0:
        return torch.empty((0,), dtype=torch.long, device=boxes.device)
    # one image of one class whose anchors are the boxes in descending score order (stable: equal scores keep the lower index first); the
    # kernel's own ranking then reproduces that order whatever the scores are: a strictly decreasing stand-in score, ties by anchor
    order = torch.argsort(scores, descending=True, stable=True)
    b = boxes.float()[order]
    s = 0.75 - 0.5 * torch.arange(n, device=b.device, dtype=torch.float64) / n
    pred = torch.cat([b[:, :4].t(), s.float()[None], b[:, 4:5].t()], 0)[None].contiguous()
    _, count, index = _nms_device_rotated(pred, 0.0, threshold, None, True, n, 1, n, 0.0, False)
    return order[index[0, : int(count[0])].long()]


def nms_device(prediction, conf_thres=0.25, iou_thres=0.45, classes=None, agnostic=False, max_det=300, nc=0, max_nms=30000, max_wh=7680,
               multi_label=False, rotated=False):
    """Batched NMS on the device, fixed-size outputs (graph-capturable): returns (boxes (B,max_det,6), count (B,),
    index (B,max_det)).  `prediction` is (B,4+nc,A); fp16 input is promoted to fp32 first (the reference promotes inside
    NMS, ops.py:275; this build keeps head outputs in fp32 end to end).  rotated=True: (B,4+nc+1,A) predictions of an OBB head ->
    rows (B,max_det,7) = x,y,w,h,conf,cls,angle (see _nms_device_rotated)."""
    from ..nn import _ops
    if isinstance(prediction, (list, tuple)):
        prediction = prediction[0]
    if rotated:
        return _nms_device_rotated(prediction, conf_thres, iou_thres, classes, agnostic, max_det, nc, max_nms, max_wh, multi_label)
    if isinstance(prediction, _ops.Candidates):  # built by the fused head decode for (conf, classes): selection + suppression only
        c = prediction
        assert 0 <= iou_thres <= 1, f"Invalid IoU {iou_thres}, valid values are between 0.0 and 1.0"
        if abs(c.conf - float(conf_thres)) > 1e-12 or c.classes != (tuple(classes) if classes is not None else None):
            raise ValueError(f"nms_device: the candidates were built for conf={c.conf} classes={c.classes}, not conf={conf_thres} classes={classes}")
        if multi_label and c.nc > 1:
            raise ValueError("nms_device: fused candidates are single-label (predict mode); validation-mode NMS needs `pred`")
        if c.device.index != torch.cuda.current_device():
            with torch.cuda.device(c.device):
                return _ops.nms_candidates(c, iou_thres, max_det, max_nms, max_wh, agnostic)
        return _ops.nms_candidates(c, iou_thres, max_det, max_nms, max_wh, agnostic)
    assert 0 <= conf_thres <= 1, f"Invalid Confidence threshold {conf_thres}, valid values are between 0.0 and 1.0"
    assert 0 <= iou_thres <= 1, f"Invalid IoU {iou_thres}, valid values are between 0.0 and 1.0"
    if prediction.shape[-1] == 6:
        return _end2end_filter(prediction, conf_thres, classes, max_det)
    nc = nc or (prediction.shape[1] - 4)
    nm = prediction.shape[1] - nc - 4
    if nm < 0:
        raise ValueError(f"nms_device: nc={nc} but the prediction has {prediction.shape[1]} channels")
    if prediction.is_cuda and prediction.device.index != torch.cuda.current_device():
        with torch.cuda.device(prediction.device):  # launches go to the current device's stream (_lib.stream)
            return nms_device(prediction, conf_thres, iou_thres, classes, agnostic, max_det, nc, max_nms, max_wh, multi_label)
    if nm:
        # mask coefficients ride behind the class scores (reference ops.py:232-234,257,266): suppression sees the first 4+nc channels, the
        # kept rows get their nm coefficients appended, gathered by anchor index -> rows of 6+nm (zeros beyond `count`)
        boxes, count, index = nms_device(prediction[:, :4 + nc], conf_thres, iou_thres, classes, agnostic, max_det, nc, max_nms, max_wh, multi_label)
        ok = index >= 0
        idx = index.clamp(min=0).long()[:, None, :].expand(-1, nm, -1)
        coef = torch.gather(prediction[:, 4 + nc:].float(), 2, idx).transpose(1, 2) * ok[..., None]
        return torch.cat([boxes, coef], 2), count, index
    p = prediction.float().contiguous()
    mask = None
    if classes is not None:
        mask = torch.zeros(nc, dtype=torch.uint8)
        mask[torch.as_tensor(list(classes), dtype=torch.long)] = 1
        mask = mask.to(p.device)
    return _ops.nms(p, conf_thres, iou_thres, max_det, max_nms, max_wh, agnostic, mask, multi_label)


def non_max_suppression(prediction, conf_thres=0.25, iou_thres=0.45, classes=None, agnostic=False, multi_label=False, labels=(),
                        max_det=300, nc=0, max_time_img=0.05, max_nms=30000, max_wh=7680, in_place=True, rotated=False):
    """Reference signature (ops.py:167-183); returns a list of (n_i, 6) tensors [x1,y1,x2,y2,conf,cls] -- (n_i, 6+nm) with the mask
    coefficients appended when the prediction carries nm channels behind the nc classes (pass nc=).
    multi_label=True is the validation-mode variant (one candidate per (anchor, class) above conf, ops.py:270-272).
    rotated=True: predictions of an OBB head (B,4+nc+1,A) -> (n_i, 7) rows [x,y,w,h,conf,cls,angle], single label only (multi_label=True
    raises NotImplementedError, and so does the reference's nc-less default, which would score the angle row as a class: pass nc=).
    Differences, all deliberate: no wall-clock abort (:238,:312-314 make the reference output timing dependent);
    the input tensor is not rewritten to xyxy in place; labels (autolabel) is not built and raises."""
    if labels and len(labels):
        raise NotImplementedError("the autolabel NMS variant is not part of the built path")
    if isinstance(prediction, (list, tuple)):
        prediction = prediction[0]
    boxes, count, _ = nms_device(prediction, conf_thres, iou_thres, classes, agnostic, max_det, nc, max_nms, max_wh, multi_label, rotated=rotated)
    n = count.tolist()  # one D2H sync for the whole batch
    return [boxes[i, : n[i]] for i in range(len(n))]


def crop_mask(masks, boxes):
    """masks [n,h,w] * (box indicator), boxes [n,4] xyxy in mask pixels (reference :644-660): column r is kept where r >= x1 and r < x2, row
    c where c >= y1 and c < y2.  A tensor utility for callers that hold masks already; the predict path crops inside ey_process_mask."""
    _, h, w = masks.shape
    x1, y1, x2, y2 = torch.chunk(boxes[:, :, None], 4, 1)
    r = torch.arange(w, device=masks.device, dtype=x1.dtype)[None, None, :]
    c = torch.arange(h, device=masks.device, dtype=x1.dtype)[None, :, None]
    return masks * ((r >= x1) * (r < x2) * (c >= y1) * (c < y2))


def process_mask(protos, masks_in, bboxes, shape, upsample=False):
    """Reference signature (:663-693): protos [nm,mh,mw], masks_in [n,nm], bboxes [n,4] xyxy in `shape` = (ih, iw) pixels -> [n,mh,mw], or
    [n,ih,iw] with upsample=True, on ey_process_mask (coefficient product, crop, bilinear upsampling and the > 0 compare in one launch).
    Returns uint8 0 / 1 where the reference returns the same values as fp32.  upsample=True needs ih/mh == iw/mw in {1, 2, 4, 8} and every
    call nm a multiple of 8 up to 64 (NotImplementedError otherwise)."""
    from ..nn import _ops
    from .. import _lib as L
    nm, mh, mw = protos.shape
    ih, iw = int(shape[0]), int(shape[1])
    n = int(masks_in.shape[0])
    with torch.cuda.device(protos.device):
        proto = L.as_nhwc(protos[None])
        boxes = bboxes[:, :4].float()
        if upsample:
            s = ih // mh
            if s * mh != ih or s * mw != iw:
                raise NotImplementedError(f"process_mask: upsampling {mh}x{mw} -> {ih}x{iw} is not one integer ratio (1, 2, 4 and 8 are built)")
            boxes = boxes.contiguous()
        else:  # the crop happens on the low-resolution grid: scale the boxes exactly as the reference does (:681-688)
            s = 1
            boxes = boxes * torch.tensor([mw / iw, mh / ih, mw / iw, mh / ih], dtype=torch.float32, device=boxes.device)
        if masks_in.dtype not in (torch.float16, torch.float32):
            masks_in = masks_in.float()
        coef = masks_in.contiguous().view(1, n, 1, nm).permute(0, 3, 1, 2)  # one level, one row per "anchor"
        rows = torch.stack([torch.zeros(n, dtype=torch.int32, device=protos.device), torch.arange(n, dtype=torch.int32, device=protos.device)], 1).contiguous()
        if n == 0:
            return torch.empty((0, s * mh, s * mw), dtype=torch.uint8, device=protos.device)
        return _ops.process_mask(proto, [coef], rows, boxes.contiguous(), s)


def process_mask_native(protos, masks_in, bboxes, shape):
    """Reference signature (:696-713): protos [nm,mh,mw], masks_in [n,nm], bboxes [n,4] xyxy in `shape` = (h, w) pixels -> [n,h,w]: the
    product, scale_masks' crop and bilinear resize to `shape` (any ratio), crop_mask on the resized map and the > 0 compare in one
    ey_process_mask_native launch.  Returns uint8 0 / 1 where the reference returns the same values as fp32.  nm a multiple of 8 up to 64
    (NotImplementedError otherwise); an empty crop raises ValueError where the reference's F.interpolate raises."""
    from ..nn import _ops
    from .. import _lib as L
    nm, mh, mw = protos.shape
    h, w = int(shape[0]), int(shape[1])
    n = int(masks_in.shape[0])
    if n == 0:
        return torch.empty((0, h, w), dtype=torch.uint8, device=protos.device)
    with torch.cuda.device(protos.device):
        if masks_in.dtype not in (torch.float16, torch.float32):
            masks_in = masks_in.float()
        coef = masks_in.contiguous().view(1, n, 1, nm).permute(0, 3, 1, 2)  # one level, one row per "anchor"
        rows = torch.stack([torch.zeros(n, dtype=torch.int32, device=protos.device), torch.arange(n, dtype=torch.int32, device=protos.device)], 1).contiguous()
        return _ops.process_mask_native(L.as_nhwc(protos[None]), [coef], rows, bboxes[:, :4].float().contiguous(), [0, n], [(h, w)])[1][0]


def _contours2segment(c, strategy="all"):
    """what masks2segments makes of one mask's contours (reference :809-820): c = a list of (k, 2) integer arrays in cv2.findContours' order."""
    import numpy as np
    if strategy not in ("all", "largest"):
        raise ValueError(f"masks2segments: strategy '{strategy}' (the reference knows 'all' and 'largest')")
    if not len(c):
        return np.zeros((0, 2), dtype=np.float32)  # no segments found
    if strategy == "all":  # merge and concatenate all segments
        from ..data.converter import merge_multi_segment
        seg = np.concatenate(merge_multi_segment([x.reshape(-1, 2) for x in c])) if len(c) > 1 else c[0].reshape(-1, 2)
    else:  # the first contour with the most vertices
        seg = np.array(c[np.array([len(x) for x in c]).argmax()]).reshape(-1, 2)
    return seg.astype("float32")


def masks2segments(masks, strategy="all"):
    """Reference signature (:793-821): masks (n, h, w) on the device -> a list of n float32 (k, 2) segments of x, y in mask pixels.  The
    contours are cv2.findContours(m, RETR_EXTERNAL, CHAIN_APPROX_SIMPLE) per mask, here ey_mask_contours for all masks in one launch; only
    the vertices come to the host.  'all' joins several contours with merge_multi_segment, 'largest' takes the first one with the most
    vertices, no contour gives zeros((0, 2)).  Masks on the host raise: contour extraction has no CPU path."""
    from ..nn import _ops
    if not torch.is_tensor(masks) or not masks.is_cuda:
        raise NotImplementedError("masks2segments: the masks are on the host; polygon extraction runs on the device only (ey_mask_contours), "
                                  "call it before .cpu() / .numpy()")
    if strategy not in ("all", "largest"):
        raise ValueError(f"masks2segments: strategy '{strategy}' (the reference knows 'all' and 'largest')")
    if masks.dtype not in (torch.uint8, torch.bool):
        masks = masks.int() != 0  # (the reference's .int(): a fraction below 1 is not set)
    with torch.cuda.device(masks.device):
        return [_contours2segment(c, strategy) for c in _ops.mask_contours(masks.contiguous())]


def scale_masks(masks, shape, padding=True):
    """Reference signature (:716-737): masks (N,C,H,W) -> (N,C,*shape): the letterbox padding is cropped away (padding=True), then
    F.interpolate(mode="bilinear", align_corners=False), on ey_scale_masks.  uint8 / bool masks give fp32, float16 / float32 keep their
    dtype.  For callers that want masks at the original resolution; the FastSAM prompt path never calls it (see ey_mask_prompt)."""
    from ..nn import _ops
    with torch.cuda.device(masks.device):
        return _ops.scale_masks(masks, shape, padding=padding)


def adjust_bboxes_to_image_border(boxes, image_shape, threshold=20):
    """Reference models/fastsam/utils.py:4-24: boxes (..., 4) xyxy within `threshold` pixels of the image border stick to it; writes `boxes`
    in place and returns it.  Masked fills instead of the reference's boolean-index assignments: the same values without a host sync."""
    h, w = image_shape
    boxes[..., 0].masked_fill_(boxes[..., 0] < threshold, 0)
    boxes[..., 1].masked_fill_(boxes[..., 1] < threshold, 0)
    boxes[..., 2].masked_fill_(boxes[..., 2] > w - threshold, w)
    boxes[..., 3].masked_fill_(boxes[..., 3] > h - threshold, h)
    return boxes


_CORNER_SIGNS = ((1.0, 1.0), (1.0, -1.0), (-1.0, -1.0), (-1.0, 1.0))  # (along w, along h) of the four corners, in the reference's order


def xywhr2xyxyxyxy(x):
    """(..., 5) [cx, cy, w, h, rotation] -> (..., 4, 2) corner points; torch tensors or numpy arrays.  Corner k is the centre plus the
    half extents (sw_k w/2, sh_k h/2) turned by the rotation: x = cx + sw w/2 cos - sh h/2 sin, y = cy + sw w/2 sin + sh h/2 cos, summed in
    that order (the reference's :556-584 adds the w edge vector first, then the h one)."""
    import numpy as np
    xp = torch if isinstance(x, torch.Tensor) else np
    c, s = xp.cos(x[..., 4]), xp.sin(x[..., 4])
    hw, hh = x[..., 2] / 2, x[..., 3] / 2
    ux, uy, vx, vy = hw * c, hw * s, -hh * s, hh * c  # half edge vectors along w and along h
    pts = [xp.stack([(x[..., 0] + ux * sw) + vx * sh, (x[..., 1] + uy * sw) + vy * sh], -1) for sw, sh in _CORNER_SIGNS]
    return xp.stack(pts, -2)


def regularize_rboxes(rboxes):
    """(N,5) xywhr -> the same rectangles with the long side first and the angle in [0, pi) (reference :775-790): where h >= w the sides
    swap and the angle advances by pi/2; every angle is then reduced modulo pi."""
    swap = ~(rboxes[..., 2] > rboxes[..., 3])
    turned = torch.stack([rboxes[..., 0], rboxes[..., 1], rboxes[..., 3], rboxes[..., 2], rboxes[..., 4] + math.pi / 2], -1)
    out = torch.where(swap[..., None], turned, rboxes)
    out[..., 4] = out[..., 4] % math.pi
    return out
