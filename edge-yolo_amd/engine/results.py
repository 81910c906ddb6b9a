"""Minimal `Results` / `Boxes` / `Masks` / `OBB` / `Keypoints` / `Probs` containers with the attribute surface of the reference's engine/results.py
(:187 Results, :938 Boxes, :1093 Masks, :1254 Keypoints, :1378 Probs, :1519 OBB) that predict() callers read.  Plotting/saving are out of scope."""
import numpy as np
import torch


class Boxes:
    """(n,6) rows [x1,y1,x2,y2,conf,cls], or (n,7) rows [x1,y1,x2,y2,track id,conf,cls] behind Model.track(), in original-image pixels
    (reference engine/results.py:938-1010)."""

    def __init__(self, boxes, orig_shape):
        if boxes.ndim == 1:
            boxes = boxes[None, :]
        assert boxes.shape[-1] in {6, 7}, f"expected 6 or 7 values but got {boxes.shape[-1]}"  # xyxy, track_id, conf, cls
        self.data = boxes
        self.orig_shape = orig_shape
        self.is_track = boxes.shape[-1] == 7

    @property
    def id(self):
        """track ids (n,), None without tracks."""
        return self.data[:, -3] if self.is_track else None

    @property
    def xyxy(self):
        return self.data[:, :4]

    @property
    def conf(self):
        return self.data[:, -2]

    @property
    def cls(self):
        return self.data[:, -1]

    @property
    def xywh(self):
        b = self.xyxy
        return torch.cat(((b[:, :2] + b[:, 2:]) / 2, b[:, 2:] - b[:, :2]), 1)

    @property
    def xyxyn(self):
        b = self.xyxy.clone()
        b[:, [0, 2]] /= self.orig_shape[1]
        b[:, [1, 3]] /= self.orig_shape[0]
        return b

    def cpu(self):
        return Boxes(self.data.cpu(), self.orig_shape)

    def numpy(self):
        return Boxes(self.data.cpu().numpy(), self.orig_shape)

    def __getitem__(self, idx):
        """rows `idx` (int, slice, index or bool tensor) as a new container (reference BaseTensor.__getitem__, engine/results.py:167-184)."""
        return self.__class__(self.data[idx], self.orig_shape)

    def __len__(self):
        return len(self.data)


class Masks:
    """(n,h,w) instance masks: at the network-input resolution (retina_masks=False, ey_process_mask), or at the image's original resolution
    (retina_masks=True, ey_process_mask_native: h, w = orig_shape).  `data` is torch.bool -- a view of the uint8 bytes the kernel wrote (the
    reference keeps the same 0 / 1 values as fp32).  `xy` / `xyn`: one polygon per mask from ey_mask_contours (utils.ops.masks2segments), for
    masks on the device; a Masks moved to the host (`cpu()`, `numpy()`) raises there."""

    def __init__(self, masks, orig_shape):
        if masks.ndim == 2:
            masks = masks[None, :]
        if torch.is_tensor(masks) and masks.dtype == torch.uint8:
            masks = masks.view(torch.bool)
        self.data = masks
        self.orig_shape = orig_shape

    @property
    def shape(self):
        return self.data.shape

    def _segments(self, normalize):
        if not torch.is_tensor(self.data) or not self.data.is_cuda:
            raise NotImplementedError("Masks.xy / xyn: these masks are on the host; polygon extraction runs on the device only (ey_mask_contours, no "
                                      "CPU path): read xy / xyn before cpu() / numpy()")
        from ..utils import ops
        return [ops.scale_coords(self.data.shape[1:], x, self.orig_shape, normalize=normalize) for x in ops.masks2segments(self.data)]

    @property
    def xy(self):
        """one float32 (k, 2) polygon per mask in pixels of the original image (reference engine/results.py:1227-1251)."""
        return self._segments(False)

    @property
    def xyn(self):
        """the same polygons divided by the original image's width and height (reference :1202-1225)."""
        return self._segments(True)

    def cpu(self):
        return Masks(self.data.cpu(), self.orig_shape)

    def numpy(self):
        return Masks(self.data.cpu().numpy(), self.orig_shape)

    def __getitem__(self, idx):
        """rows `idx` (int, slice, index or bool tensor) as a new container (reference BaseTensor.__getitem__, engine/results.py:167-184)."""
        return self.__class__(self.data[idx], self.orig_shape)

    def __len__(self):
        return len(self.data)


class OBB:
    """(n,7) rows [cx,cy,w,h,rotation,conf,cls] in original-image pixels (reference :1519; track ids are not built)."""

    def __init__(self, boxes, orig_shape):
        if boxes.ndim == 1:
            boxes = boxes[None, :]
        assert boxes.shape[-1] == 7, f"expected 7 values but got {boxes.shape[-1]}"
        self.data = boxes
        self.orig_shape = orig_shape

    @property
    def xywhr(self):
        return self.data[:, :5]

    @property
    def conf(self):
        return self.data[:, -2]

    @property
    def cls(self):
        return self.data[:, -1]

    @property
    def xyxyxyxy(self):
        """(n,4,2) corner points."""
        from ..utils import ops
        return ops.xywhr2xyxyxyxy(self.xywhr)

    @property
    def xyxyxyxyn(self):
        p = self.xyxyxyxy
        p = p.clone() if isinstance(p, torch.Tensor) else np.copy(p)
        p[..., 0] /= self.orig_shape[1]
        p[..., 1] /= self.orig_shape[0]
        return p

    @property
    def xyxy(self):
        """(n,4) axis-aligned boxes enclosing the corner points."""
        p = self.xyxyxyxy
        x, y = p[..., 0], p[..., 1]
        if isinstance(x, torch.Tensor):
            return torch.stack([x.amin(1), y.amin(1), x.amax(1), y.amax(1)], -1)
        return np.stack([x.min(1), y.min(1), x.max(1), y.max(1)], -1)

    def cpu(self):
        return self if isinstance(self.data, np.ndarray) else OBB(self.data.cpu(), self.orig_shape)

    def numpy(self):
        return self if isinstance(self.data, np.ndarray) else OBB(self.data.cpu().numpy(), self.orig_shape)

    def __getitem__(self, idx):
        """rows `idx` (int, slice, index or bool tensor) as a new container (reference BaseTensor.__getitem__, engine/results.py:167-184)."""
        return self.__class__(self.data[idx], self.orig_shape)

    def __len__(self):
        return len(self.data)


class Keypoints:
    """(n,K,2) or (n,K,3) keypoints [x, y(, confidence)] in original-image pixels (reference :1254-1375).  Points whose confidence is below
    0.5 get x = y = 0, in the tensor handed in (the reference's constructor writes in place too)."""

    def __init__(self, keypoints, orig_shape):
        if keypoints.ndim == 2:
            keypoints = keypoints[None, :]
        if keypoints.shape[2] == 3:  # x, y, conf
            mask = keypoints[..., 2] < 0.5  # points with conf < 0.5 (not visible)
            keypoints[..., :2][mask] = 0
        self.data = keypoints
        self.orig_shape = orig_shape
        self.has_visible = self.data.shape[-1] == 3

    @property
    def shape(self):
        return self.data.shape

    @property
    def xy(self):
        return self.data[..., :2]

    @property
    def xyn(self):
        xy = self.xy.clone() if isinstance(self.xy, torch.Tensor) else np.copy(self.xy)
        xy[..., 0] /= self.orig_shape[1]
        xy[..., 1] /= self.orig_shape[0]
        return xy

    @property
    def conf(self):
        return self.data[..., 2] if self.has_visible else None

    def cpu(self):
        return self if isinstance(self.data, np.ndarray) else Keypoints(self.data.cpu(), self.orig_shape)

    def numpy(self):
        return self if isinstance(self.data, np.ndarray) else Keypoints(self.data.cpu().numpy(), self.orig_shape)

    def __getitem__(self, idx):
        """rows `idx` (int, slice, index or bool tensor) as a new container (reference BaseTensor.__getitem__, engine/results.py:167-184)."""
        return self.__class__(self.data[idx], self.orig_shape)

    def __len__(self):
        return len(self.data)


class Probs:
    """(nc,) class probabilities of one image (reference :1378-1516).  top1 / top5 / top1conf / top5conf are the reference's expressions
    (argmax; (-data).argsort(0)[:5]) unless the head's own top-5 came along (`top`: (index int32 (k,), probability (k,)) from
    ey_classify_linear_softmax, k = min(nc, 5)); those rank equal probabilities by the lower class index."""

    def __init__(self, probs, orig_shape=None, top=None):
        self.data = probs
        self.orig_shape = orig_shape
        self._top = top

    @property
    def shape(self):
        return self.data.shape

    @property
    def top1(self):
        if self._top is not None:
            return int(self._top[0][0])
        return int(self.data.argmax())

    @property
    def top5(self):
        if self._top is not None:
            return [int(v) for v in self._top[0]]
        return (-self.data).argsort(0)[:5].tolist()  # this way works with both torch and numpy.

    @property
    def top1conf(self):
        return self.data[self.top1]

    @property
    def top5conf(self):
        return self.data[self.top5]

    def _like(self, f):
        return Probs(f(self.data), self.orig_shape, None if self._top is None else tuple(f(t) for t in self._top))

    def cpu(self):
        return self if isinstance(self.data, np.ndarray) else self._like(lambda t: t.cpu())

    def numpy(self):
        return self if isinstance(self.data, np.ndarray) else self._like(lambda t: t.cpu().numpy())

    def __getitem__(self, idx):
        """entries `idx` of the probability vector as a new Probs (reference BaseTensor.__getitem__; the head's own top-5 does not carry over)."""
        return Probs(self.data[idx], self.orig_shape)

    def __len__(self):
        return len(self.data)


class Results:
    def __init__(self, orig_img, path, names, boxes=None, masks=None, speed=None, obb=None, keypoints=None, probs=None):
        self.orig_img = orig_img
        self.orig_shape = tuple(orig_img.shape[:2]) if orig_img is not None and hasattr(orig_img, "shape") and orig_img.ndim == 3 else None
        self.boxes = Boxes(boxes, self.orig_shape) if boxes is not None else None
        self.masks = Masks(masks, self.orig_shape) if masks is not None else None
        self.obb = OBB(obb, self.orig_shape) if obb is not None else None
        self.keypoints = Keypoints(keypoints, self.orig_shape) if keypoints is not None else None
        self.probs = (probs if isinstance(probs, Probs) else Probs(probs)) if probs is not None else None
        self.names = names
        self.path = path
        self.speed = speed or {"preprocess": None, "inference": None, "postprocess": None}

    def __getitem__(self, idx):
        """The detections `idx` -- an int, a slice, an index tensor or a bool tensor, on the data's device -- of every attribute present
        (boxes, masks, probs, keypoints, obb) as a new Results (reference engine/results.py:273-288 via _apply)."""
        r = Results(self.orig_img, path=self.path, names=self.names, speed=self.speed)
        r.orig_shape = self.orig_shape
        for k in ("boxes", "masks", "probs", "keypoints", "obb"):
            v = getattr(self, k)
            if v is not None:
                setattr(r, k, v[idx])
        return r

    def __len__(self):
        if self.boxes is not None:
            return len(self.boxes)
        if self.probs is not None:
            return len(self.probs)
        return len(self.obb) if self.obb is not None else 0
