"""Predict loop for the detect task: preprocess -> inference -> postprocess, mirroring the reference's
engine/predictor.py (`BasePredictor.preprocess/inference/postprocess/stream_inference` :116-304) and
models/yolo/detect/predict.py (`DetectionPredictor.postprocess` :23-41).

MI355X-native execution model: the whole per-batch device work (stem ... head decode, NMS) is launched on one HIP
stream and, for a fixed (batch, H, W, dtype), captured ONCE into a hipGraph and replayed (the reference re-dispatches
~300 ATen ops from Python per batch).  NMS results come back as one fixed-size (B,max_det,6)+(B,) device buffer,
so there is exactly one D2H copy per batch.
"""
import contextlib
import gc
import threading
import time

import numpy as np
import torch

from .results import Results
from ..utils import ops


class Profile:
    """Wall timer with device sync (reference utils/ops.py:17-62)."""

    def __init__(self, device=None):
        self.t, self.dt, self.device = 0.0, 0.0, device

    def __enter__(self):
        self.start = self.time()
        return self

    def __exit__(self, *a):
        self.dt = self.time() - self.start
        self.t += self.dt

    def time(self):
        if self.device is not None and self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        return time.perf_counter()


@contextlib.contextmanager
def _capture(graph):
    """torch.cuda.graph(graph) with Python's cyclic garbage collector held off for the duration: a collection that runs in the middle
    of a capture may finalise an unrelated captured graph (a replaced predictor, an exhausted pipeline), and destroying a hipGraph while
    any stream is capturing is an error ("operation not permitted when stream is capturing") that kills the process."""
    gc.collect()
    was = gc.isenabled()
    gc.disable()
    try:
        with torch.cuda.graph(graph):
            yield
    finally:
        if was:
            gc.enable()


class GraphRunner:
    """Captures `fn(static_input) -> tuple of tensors` into a HIP graph per input signature and replays it."""

    def __init__(self, fn, warmup=2):
        self.fn, self.warmup, self.graphs = fn, warmup, {}

    def __call__(self, x):
        key = (tuple(x.shape), x.dtype, x.device)
        g = self.graphs.get(key)
        if g is None:
            static_in = x.clone()
            s = torch.cuda.Stream(device=x.device)
            s.wait_stream(torch.cuda.current_stream(x.device))
            with torch.cuda.stream(s):
                for _ in range(self.warmup):  # packs weights, sizes allocator pools
                    out = self.fn(static_in)
            torch.cuda.current_stream(x.device).wait_stream(s)
            torch.cuda.synchronize(x.device)
            graph = torch.cuda.CUDAGraph()
            with _capture(graph):
                out = self.fn(static_in)
            g = self.graphs[key] = (graph, static_in, out)
        graph, static_in, out = g
        if x.data_ptr() != static_in.data_ptr():  # callers that fill static_input() in place skip the copy
            static_in.copy_(x, non_blocking=True)
        graph.replay()
        return out

    def static_input(self, like):
        """The captured graph's input buffer for tensors shaped like `like` (captures on first use)."""
        self(like)
        return self.graphs[(tuple(like.shape), like.dtype, like.device)][1]


class PipelinedRunner:
    """Software pipeline over consecutive batches: stage s of batch i runs on its own HIP stream while stage s-1 of batch i+1 and
    stage s+1 of batch i-1 run on theirs.  Most kernels of this network at batch 32 are latency-bound (small feature maps, a few
    hundred workgroups), so independent work from neighbouring batches fills the chip.  Each stage is a captured hipGraph; as many
    buffer sets as stages alternate, so nothing is copied between the stages.  Every batch still goes through every stage in full --
    only their placement in time overlaps (throughput mode; stages-1 batches of extra latency).

    PipelinedRunner(f1, f2, ..., example): stage functions chained (stage k gets stage k-1's return value), example = input batch.
    """

    def __init__(self, *args, warmup=2, copy_stream=False, streams=None, extra_sets=None):
        """copy_stream=True: batches handed to submit(x) are copied into the stage-0 input buffer on a stream of their own (host
        tensors: one H2D DMA per batch that overlaps the compute of the batches in flight) instead of on the first stage's stream.
        A pinned host batch must stay unchanged until its results are out (the usual contract of an asynchronous copy).
        streams: HIP streams to run the stages on (>= one per stage).  HIP binds streams to the 4 hardware queues in creation order,
        so callers that build several pipelines (bench.py's start-up auto-tune) create ONE set of streams and hand it to all of
        them: a second set would alias queues of the first and run ~25 % slower."""
        *stages, example = args
        dev = example.device
        self.dev, self.n = dev, len(stages)
        # buffer sets: one per stage -- plus one with a copy stream: the upload of batch i is a pipeline stage of its own (it waits for
        # the batch that used its buffer set before), so with n sets stage 0 idles for the whole transfer of every batch
        self.nsets = self.n + ((1 if copy_stream else 0) if extra_sets is None else int(extra_sets))
        if streams is not None and len(streams) < len(stages):
            raise ValueError(f"PipelinedRunner: {len(stages)} stages need {len(stages)} streams, got {len(streams)}")
        self.streams = list(streams[: len(stages)]) if streams is not None else [torch.cuda.Stream(device=dev) for _ in stages]
        # the upload rides on the FIRST stage's stream (in order before that batch's stage-0 graph; it overlaps the other stages of the
        # batches in flight).  A stream of its own would be the fifth active stream: HIP binds streams to 4 hardware queues, two of the
        # five then share one and the batches stop overlapping altogether (measured: 2.05 ms/batch = the unpipelined step, device-resident
        # input included)
        self.copy_stream = self.streams[0] if copy_stream else None
        self.sf, self.sp = self.streams[0], self.streams[-1]
        self.sets = []
        cur = torch.cuda.current_stream(dev)
        for _ in range(self.nsets):
            static_in = example.clone()
            self.sf.wait_stream(cur)
            with torch.cuda.stream(self.sf):
                for _ in range(warmup):
                    v = static_in
                    for f in stages:
                        v = f(v)
            cur.wait_stream(self.sf)
            torch.cuda.synchronize(dev)
            graphs, v = [], static_in
            for f in stages:
                g = torch.cuda.CUDAGraph()
                with _capture(g):
                    v = f(v)
                graphs.append(g)
            self.sets.append(dict(x=static_in, graphs=graphs, out=v, done=[torch.cuda.Event() for _ in stages]))
        self.i = 0
        for st in self.sets:  # events start in the signalled state
            for e in st["done"]:
                e.record(cur)
        for st in self.sets:
            st["post_done"] = st["done"][-1]

    def static_input(self, j=None):
        return self.sets[self.i % self.nsets if j is None else j]["x"]

    def submit(self, x=None, upload=None, side_copy=False):
        """Enqueue one batch (x=None: the batch already sits in static_input()).  Returns the buffer-set index; its outputs
        are valid after `wait(j)` / a device synchronise.  upload(dst, x, j): brings x to the device in place of the plain copy into the
        stage-0 input buffer `dst` of buffer set j; runs on the copy stream when there is one and may return a callable that is then run
        on the FIRST STAGE's stream right before its graph (e.g. raw uint8 bytes over PCIe on the copy stream, the conversion kernel
        on the stage stream).  side_copy=True: the plain copy goes to a stream of its own instead of the first stage's -- right for
        DMA uploads of big host batches (measured, 78.6 MB f16 batches: 2.2 vs 2.8 ms per batch), wrong for everything else: a fifth
        active stream shares one of HIP's 4 hardware queues with a stage and the batches stop overlapping (device-resident input:
        2.05 vs 1.35 ms per batch)."""
        j = self.i % self.nsets
        self.i += 1
        st = self.sets[j]
        cur = torch.cuda.current_stream(self.dev)
        self.streams[0].wait_stream(cur)
        copied, finish = None, None
        if self.copy_stream is not None and x is not None and x.data_ptr() != st["x"].data_ptr():
            cs = self.copy_stream
            if side_copy:
                if getattr(self, "_side_copy", None) is None:
                    self._side_copy = torch.cuda.Stream(device=self.dev)
                cs = self._side_copy
            cs.wait_stream(cur)
            cs.wait_event(st["done"][-1])  # every stage of the batch that used this buffer set n submits ago is done (stage 0 read its input long before)
            with torch.cuda.stream(cs):
                if upload is not None:
                    finish = upload(st["x"], x, j)
                else:
                    st["x"].copy_(x, non_blocking=True)
                if x.is_cuda:
                    # x was allocated on the caller's stream and is read here on the copy stream: without this the caching allocator hands its
                    # block to the caller's next allocation (e.g. the next batch's converted input) as soon as the caller drops x, while
                    # this copy may not have run yet -- the batch would silently receive the next batch's pixels
                    x.record_stream(cs)
                copied = torch.cuda.Event()
                copied.record(cs)
            x = None
        for s, (stream, g) in enumerate(zip(self.streams, st["graphs"])):
            with torch.cuda.stream(stream):
                # stage 0 waits for the LAST stage of the batch that used this buffer set n submits ago; stage s for stage s-1 of this batch
                stream.wait_event(st["done"][-1] if s == 0 else st["done"][s - 1])
                if s == 0 and copied is not None:
                    stream.wait_event(copied)
                    if finish is not None:
                        finish()
                if s == 0 and x is not None and x.data_ptr() != st["x"].data_ptr():
                    if upload is not None:
                        finish = upload(st["x"], x, j)
                        if finish is not None:
                            finish()
                    else:
                        st["x"].copy_(x, non_blocking=True)
                g.replay()
                st["done"][s].record(stream)
        return j

    def outputs(self, j):
        return self.sets[j]["out"]

    def wait(self, j=None):
        cur = torch.cuda.current_stream(self.dev)
        for k in ([j] if j is not None else range(self.nsets)):
            cur.wait_event(self.sets[k]["done"][-1])


class DetectionPredictor:
    # What the facade reads from a predictor class (an injected class without these gets the values here):
    imgsz = 640  # letterbox target of ndarray sources (reference cfg default); predict(imgsz=) sets it on the instance
    refused_options = {}  # predict() keyword -> the NotImplementedError text it raises when the keyword is set
    # augment=True: None = test-time augmentation is built (DetectionModel._predict_augment); ("warn", model class name) = that model has none,
    # the reference warns and runs single-scale (tasks.py:374-376); ("raise", task name) = refused
    augment_policy = None

    def __init__(self, model, device, half=False, conf=0.25, iou=0.7, max_det=300, agnostic_nms=False, classes=None, graph=True, validate_input=None, keep_pred=False,
                 augment=False):
        """This signature is the contract for classes injected through `YOLO.predict(predictor=...)` (reference engine/model.py:505,552):
        the facade constructs `cls(model, device, half=, conf=, iou=, max_det=, agnostic_nms=, classes=, graph=, augment=)` and calls the
        instance with the source; subclasses usually override `preprocess` / `postprocess` (reference BasePredictor hooks).

        validate_input: the reference's value-range check of tensor sources (LoadTensor._single_check, data/loaders.py:560-566: a tensor
        whose max exceeds 1 is divided by 255 with a warning).  None (default) = reference behaviour for HOST tensors (the check runs on
        the host, no device sync) and NO check for DEVICE tensors (it would cost a device reduction + a host sync per call -- a
        deliberate divergence: a 0..255 device tensor is fed to the network as is); True = check device tensors too; False = never.
        augment: scale / flip test-time augmentation (DetectionModel._predict_augment; cfg/default.yaml `augment`), as far as the class's
        `augment_policy` has it."""
        if augment and self.augment_policy is not None:
            action, who = self.augment_policy
            if action == "raise":
                raise NotImplementedError(f"{type(self).__name__}: augment=True (test-time augmentation) is not built for the {who} task")
            import warnings
            warnings.warn(f"{who} does not support 'augment=True', reverting to single-scale prediction.")
            augment = False
        self.model,self.device, self.half, self.validate_input, self.keep_pred, self.augment = model, device, half, validate_input, keep_pred, bool(augment)
        self.conf, self.iou, self.max_det, self.agnostic_nms, self.classes = conf, iou, max_det, agnostic_nms, classes
        self._lock = threading.Lock()
        self.runner = GraphRunner(self._device_step) if graph else self._device_step

    def close(self):
        """Drop the captured graphs now (the runner and this predictor reference each other: without this they live until the cyclic
        collector runs, possibly in the middle of somebody's capture)."""
        self.runner = None

    # ---- device side (captured)
    def _device_step(self, im):
        if self.augment:  # three forwards + descale / clip / concat (reference tasks.py:372-408), then the ordinary NMS on the concatenated anchors
            pred = self.model(im, augment=True)[0]
            boxes, count, index = ops.nms_device(pred, self.conf, self.iou, self.classes, self.agnostic_nms, self.max_det)
            return boxes, count, index, pred
        # the head decode builds the NMS candidates for (conf, classes) in the same pass: the (B,4+nc,A) prediction tensor is only
        # written when the caller asked for it (keep_pred)
        preds = self.model(im, head_nms={"conf": self.conf, "classes": self.classes, "keep_pred": self.keep_pred})
        pred = preds[0] if isinstance(preds, (list, tuple)) else preds
        boxes, count, index = ops.nms_device(pred, self.conf, self.iou, self.classes, self.agnostic_nms, self.max_det)
        return boxes, count, index, getattr(pred, "pred", pred)

    def preprocess(self, im):
        """Tensor sources: BCHW float in [0,1] (reference LoadTensor, data/loaders.py:516-586).  ndarray / list sources:
        HWC uint8 BGR images, letterboxed to a common stride-32 shape on the host (reference predictor.py:116-161)."""
        if not isinstance(im, torch.Tensor):
            return self._letterbox_batch(im, self.imgsz)
        shape = (1, *im.shape) if im.dim() == 3 else tuple(im.shape)  # (a CHW tensor is a batch of one)
        if len(shape) != 4 or shape[2] % 32 or shape[3] % 32:
            raise ValueError(f"input tensor should be BCHW with H,W multiples of 32, got {shape}")
        check = (not im.is_cuda) if self.validate_input is None else bool(self.validate_input)
        if check and im.numel() and im.is_floating_point():  # (an integer tensor is refused below, whatever its values)
            mx = float(im.max())
            if mx > 1.0 + float(torch.finfo(im.dtype).eps):  # reference LoadTensor._single_check (data/loaders.py:560-566): warn and rescale
                import warnings
                warnings.warn(f"torch.Tensor inputs should be normalized 0.0-1.0 but max value is {mx}. Dividing input by 255.")
                im = im.float() / 255.0
        return self._tensor_source(im, "(uint8 HWC BGR images go in as numpy arrays)")

    def _tensor_source(self, im, integer_sources):
        """The tail of every task's tensor source, behind the task's own checks of a CHW / BCHW tensor: leading axis, floating-point check
        (`integer_sources`: where the task's integer images go instead, for the error text), device, dtype, contiguous."""
        if im.dim() == 3:
            im = im[None]
        if not im.is_floating_point():
            raise TypeError(f"tensor sources must be floating point images in [0,1] {integer_sources}")
        im = im.to(self.device, non_blocking=True)
        return (im.half() if self.half else im.float()).contiguous()

    def _letterbox_batch(self, ims, new_shape=640):
        """reference pre_transform + preprocess (predictor.py:123-161) on the GPU: LetterBox geometry on the host, one
        `ey_letterbox` launch per image (resize + pad 114 + BGR->RGB + CHW + /255) into the batch tensor."""
        from ..data.augment import LetterBox
        ims = ims if isinstance(ims, (list, tuple)) else [ims]
        self._orig = [np.asarray(a) for a in ims]
        same_shapes = len({a.shape for a in self._orig}) == 1
        lb = LetterBox(new_shape, auto=same_shapes, stride=int(max(self.model.stride)) if hasattr(self.model, "stride") else 32)
        return lb.batch(self._orig, self.device, torch.float16 if self.half else torch.float32)

    def __call__(self, source):
        with self._lock, torch.cuda.device(self.device):  # kernels go to the CURRENT device's stream (_lib.stream)
            self._orig = None
            prof = (Profile(self.device), Profile(self.device), Profile(self.device))
            with prof[0]:
                im = self.preprocess(source)
            with prof[1]:
                out = self.runner(im)
            with prof[2]:
                results = self._results(out, im, source)
            n = len(results)
            for r in results:
                r.speed = {"preprocess": prof[0].dt * 1e3 / n, "inference": prof[1].dt * 1e3 / n, "postprocess": prof[2].dt * 1e3 / n}
            return results

    def _results(self, out, im, source):
        """device-step outputs -> list of Results (subclasses with more outputs than boxes override this)."""
        return self.postprocess(out[0], out[1], im, source)

    def _boxes_in_image(self, boxes, count, shape):
        """Hook for subclasses: the clipped (B, max_det, 6+) rows of a batch whose originals all have the network input's `shape`, before they are
        cut into Results (FastSAMPredictor sticks them to the border here).  Nothing for the other tasks."""

    def _assemble(self, count, img, one_image, whole_batch=None):
        """The one path from a batch's device-step outputs to its list of Results, for every task.
        count: (B,) rows kept per image, read back here (the one host sync of the batch); None for a task without rows (n_i is None then).
        whole_batch(shape): the task's arithmetic over the whole batch at once, called when there is one and every original has the network
        input's `shape` (tensor sources; images that already have it: scaling is gain 1, pad 0), so it is a handful of launches, not that per image.
        one_image(i, n_i, shape) -> the keyword arguments of image i's Results; `shape` is the (h, w) its rows still have to be scaled to,
        None once whole_batch has done it."""
        n = count.tolist() if count is not None else [None] * img.shape[0]
        inp = tuple(img.shape[2:])
        same = whole_batch is not None and (self._orig is None or all(tuple(o.shape[:2]) == inp for o in self._orig))
        if same:
            whole_batch(inp)
        results = []
        for i in range(len(n)):
            orig = self._orig[i] if self._orig is not None else None
            shape = inp if orig is None else tuple(orig.shape[:2])
            r = Results(orig, path=f"image{i}.jpg", names=self.model.names, **one_image(i, n[i], None if same else shape))
            if orig is None:  # tensor sources: the frame of the result and of every field it carries is the network input
                r.orig_shape = inp
                for field in (r.boxes, r.masks, r.keypoints, r.obb, r.probs):
                    if field is not None:
                        field.orig_shape = inp
            results.append(r)
        return results

    def postprocess(self, boxes, count, img, source):
        """reference detect/predict.py:23-41: per image rows -> scale_boxes to the original shape -> Results."""
        boxes = boxes.clone()

        def whole_batch(shape):  # one clip over the whole batch (4 launches, not 4 per image)
            ops.clip_boxes(boxes, shape)
            self._boxes_in_image(boxes, count, shape)

        def one_image(i, k, shape):
            det = boxes[i, :k]
            if shape is not None:
                det[:, :4] = ops.scale_boxes(img.shape[2:], det[:, :4], shape)
            return {"boxes": det}

        return self._assemble(count, img, one_image, whole_batch)


class SegmentationPredictor(DetectionPredictor):
    """reference models/yolo/segment/predict.py:9-57.  The device step is DetectionPredictor's captured graph plus the Proto and cv4 launches
    of the Segment head; `postprocess` assembles the masks of the whole batch with ONE launch sized by the true number of kept boxes (it
    runs after the count came back, outside the graph).  retina_masks=False (default): ey_process_mask, masks at the network-input
    resolution, cropped by the boxes before scale_boxes.  retina_masks=True (:48-50): the boxes are scaled to each original image first,
    then ey_process_mask_native resizes every mask to its image's original shape -- the images of a batch may all differ -- and crops it
    there; tensor sources have original == input shape and still take that path (resize, then crop).  retina_masks is a constructor
    argument; through the facade it is the predictor class RetinaMasksPredictor (`YOLO.predict(source, predictor=RetinaMasksPredictor)`),
    the facade's `retina_masks=True` keyword itself still raises."""

    augment_policy = ("warn", "SegmentationModel")
    # (cfg/default.yaml `retina_masks`: the keyword of YOLO.predict stays refused; the built path is named in the text)
    refused_options = {"retina_masks": "retina_masks=True is not a keyword of predict(): masks at the original image resolution (ops.process_mask_native) come "
                                       "from predict(source, predictor=RetinaMasksPredictor) or SegmentationPredictor(model, device, retina_masks=True)"}

    def __init__(self, model, device, *args, retina_masks=False, **kwargs):
        super().__init__(model, device, *args, **kwargs)
        self.retina_masks = bool(retina_masks)

    def _device_step(self, im):
        cand, (_, mcs, p) = self.model(im, head_nms={"conf": self.conf, "classes": self.classes, "keep_pred": self.keep_pred})
        boxes, count, index = ops.nms_device(cand, self.conf, self.iou, self.classes, self.agnostic_nms, self.max_det)
        return (boxes, count, index, getattr(cand, "pred", None), p, *mcs)

    def _results(self, out, im, source):
        boxes, count, index, _, p, *mcs = out
        return self.postprocess(boxes, count, im, source, index=index, proto=p, coefs=mcs)

    def postprocess(self, boxes, count, img, source, index=None, proto=None, coefs=None):
        from ..nn import _ops
        from .results import Masks
        n = count.tolist()  # (the one host sync of the batch; everything below is sized by it)
        B, max_det = index.shape
        ih, iw = img.shape[2:]
        mh, mw = proto.shape[2:]
        s = ih // mh
        if not self.retina_masks and (s * mh != ih or s * mw != iw):
            raise NotImplementedError(f"SegmentationPredictor: input {ih}x{iw} over proto {mh}x{mw} is not one integer ratio")
        total = sum(n)
        masks, rows = None, None
        if total:
            # rows (image, anchor) and boxes of the kept detections, image after image, built on the device from count and index
            keep = ops.kept_rows(count, max_det)
            rows = torch.stack([torch.arange(B, dtype=torch.int32, device=index.device)[:, None].expand(B, max_det)[keep], index[keep]], 1).contiguous()
            if not self.retina_masks:
                masks = _ops.process_mask(proto, coefs, rows, boxes[keep][:, :4].contiguous(), s)  # boxes in network-input pixels, before scale_boxes
        self._masks, self._mask_counts = masks, n  # the batch's masks as ONE uint8 tensor, image after image (FastSAMPredictor scores them in one launch)
        results = super().postprocess(boxes, count, img, source)
        off = [0]
        for k in n:
            off.append(off[-1] + k)
        if total and self.retina_masks:  # (segment/predict.py:48-50) the boxes are in original-image pixels now: one launch for all originals
            scaled = torch.cat([r.boxes.xyxy for r in results if len(r.boxes)], 0).float().contiguous()
            masks = _ops.process_mask_native(proto, coefs, rows, scaled, off, [r.orig_shape for r in results])[1]
        for i, r in enumerate(results):
            if n[i]:
                r.masks = Masks(masks[i] if self.retina_masks else masks[off[i]:off[i + 1]], r.orig_shape)
        return results


class RetinaMasksPredictor(SegmentationPredictor):
    """SegmentationPredictor with retina_masks=True, as a class the facade can be handed: `YOLO.predict(source, predictor=RetinaMasksPredictor)`
    returns `masks.data` of shape (n_i, H0_i, W0_i) per image; boxes as without it."""

    refused_options = {}

    def __init__(self, model, device, *args, retina_masks=True, **kwargs):
        super().__init__(model, device, *args, retina_masks=retina_masks, **kwargs)


class FastSAMPredictor(SegmentationPredictor):
    """reference models/fastsam/predict.py:13-159.  SegmentationPredictor's device step and mask assembly; `postprocess` then sticks boxes
    near the image border to it, replaces boxes that cover more than 0.9 of the image by the full image, and selects the instances the
    prompts ask for: boxes and points in ORIGINAL-image pixels, shared by all images of the batch.  The reference resizes every mask to
    the original image (scale_masks) and sums slices of that tensor per prompt; here ONE ey_mask_prompt call scores the network-resolution
    masks of the whole batch (the resize is folded into per-axis weights) and nothing of the original resolution is allocated.  Text
    prompts need the CLIP encoder, which is not part of the build."""

    # the prompt kernel scores one (mh, mw) stack of the whole batch; masks at the original resolutions are not built for it
    refused_options = {"retina_masks": "FastSAM: retina_masks=True (masks at the original image resolution) is not built: ey_mask_prompt scores the "
                                       "network-resolution masks; use retina_masks=False"}

    def __init__(self, model, device, *args, retina_masks=False, **kwargs):
        if retina_masks:
            raise NotImplementedError(self.refused_options["retina_masks"])
        super().__init__(model, device, *args, **kwargs)
        self.prompts = {}

    def set_prompts(self, prompts):
        """Prompts of the NEXT call (reference :157-159): a dict with any of bboxes, points, labels, texts; postprocess consumes them."""
        self.prompts = dict(prompts or {})

    @staticmethod
    def check_prompts(bboxes=None, points=None, labels=None, texts=None, shapes=()):
        """Host-side form of the prompts -> (boxes int32 (P,4) or None, points int32 (Q,2) or None, labels int32 (Q,) or None), converted as
        the reference does (torch.as_tensor(..., dtype=int32): fractions are cut off; a single box / point gains a leading axis; labels
        default to 1).  Raises what ey_mask_prompt refuses, before anything runs: the reference slices with Python's rules for boxes with
        x2 <= x1, y2 <= y1 or negative coordinates (predict.py:80) and raises an IndexError for points outside the image (:101)."""
        if texts is not None:
            raise NotImplementedError("FastSAM: text prompts need the CLIP text and image encoders, which are not part of this build; use bboxes= / points=")
        if bboxes is None and points is None:
            if labels is not None:
                raise ValueError("FastSAM: labels= without points=")
            return None, None, None
        b = q = lab = None
        if bboxes is not None:
            b = np.asarray(bboxes).astype(np.int32)
            b = b[None] if b.ndim == 1 else b
            if b.ndim != 2 or b.shape[1] != 4 or b.shape[0] == 0:
                raise ValueError(f"FastSAM: bboxes must be (P,4) rows x1,y1,x2,y2 with P >= 1, got shape {tuple(b.shape)}")
            bad = (b[:, :2] < 0).any(1) | (b[:, 2] <= b[:, 0]) | (b[:, 3] <= b[:, 1])
            if bad.any():
                raise ValueError(f"FastSAM: box prompt {b[bad][0].tolist()} needs 0 <= x1 < x2 and 0 <= y1 < y2 (original-image pixels)")
        if points is not None:
            q = np.asarray(points).astype(np.int32)
            q = q[None] if q.ndim == 1 else q
            if q.ndim != 2 or q.shape[1] != 2 or q.shape[0] == 0:
                raise ValueError(f"FastSAM: points must be (Q,2) rows x,y with Q >= 1, got shape {tuple(q.shape)}")
            lab = np.ones(len(q), np.int32) if labels is None else np.asarray(labels).astype(np.int32).reshape(-1)
            if len(lab) != len(q):
                raise ValueError(f"FastSAM: expected as many labels as points, got {len(lab)} and {len(q)}")
            for h, w in shapes:
                out = (q[:, 0] < 0) | (q[:, 1] < 0) | (q[:, 0] >= w) | (q[:, 1] >= h)
                if out.any():
                    raise ValueError(f"FastSAM: point prompt {q[out][0].tolist()} lies outside the {h}x{w} image")
        elif labels is not None:
            raise ValueError("FastSAM: labels= without points=")
        return b, q, lab

    @staticmethod
    def stick_to_border(xyxy, shape, threshold=20, valid=None):
        """reference :36-44, in place on xyxy (n,4) -- or (B,n,4) with valid (B,n), the rows that exist --: adjust_bboxes_to_image_border, then
        every box whose IoU with the full image exceeds 0.9 becomes the full image.  box_iou(full, boxes) is utils/metrics.py:54-77 in fp32;
        the intersection with the full image is the clamped box.  The reference flattens the (row, column) pairs that torch.nonzero returns
        for the (1, n) IoU matrix (:42), so its index list holds a 0 for every match: box 0 becomes the full image too whenever any box
        qualifies.  Kept, so that rows equal the reference's.  No host sync."""
        h, w = shape
        ops.adjust_bboxes_to_image_border(xyxy, shape, threshold)
        inter = (xyxy[..., 2].clamp(max=w) - xyxy[..., 0].clamp(min=0)).clamp_(0) * (xyxy[..., 3].clamp(max=h) - xyxy[..., 1].clamp(min=0)).clamp_(0)
        iou = inter / (float(w) * float(h) + (xyxy[..., 2] - xyxy[..., 0]) * (xyxy[..., 3] - xyxy[..., 1]) - inter + 1e-7)
        sel = iou > 0.9
        if valid is not None:
            sel &= valid
        sel[..., 0] |= sel.any(-1)
        xyxy.copy_(torch.where(sel[..., None], torch.tensor([0, 0, w, h], dtype=xyxy.dtype, device=xyxy.device), xyxy))
        return xyxy

    def _boxes_in_image(self, boxes, count, shape):
        """original == network input for the whole batch: the border step over all images at once (a handful of launches, not per image)."""
        self.stick_to_border(boxes[..., :4], shape, valid=ops.kept_rows(count, boxes.shape[1]))
        self._stuck = True

    def postprocess(self, boxes, count, img, source, index=None, proto=None, coefs=None):
        from ..nn import _ops
        prompts, self.prompts = self.prompts, {}
        self.check_prompts(texts=prompts.get("texts"))  # (before the device work below)
        self._stuck = False
        results = super().postprocess(boxes, count, img, source, index=index, proto=proto, coefs=coefs)
        if not self._stuck:  # originals of other shapes: image by image, after scale_boxes
            for r in results:
                if len(r):
                    self.stick_to_border(r.boxes.xyxy, r.orig_shape)  # in place: xyxy is a view of the result's rows
        n = self._mask_counts
        b, q, lab = self.check_prompts(prompts.get("bboxes"), prompts.get("points"), prompts.get("labels"), None, [r.orig_shape for r in results])
        if (b is None and q is None) or not sum(n):
            return results
        off = [0]
        for k in n:
            off.append(off[-1] + k)
        keep = _ops.mask_prompt(self._masks, off, [r.orig_shape for r in results], b, q, lab)["keep"].view(torch.bool)
        return [r[keep[off[i]:off[i + 1]]] if n[i] else r for i, r in enumerate(results)]


class OBBPredictor(DetectionPredictor):
    """reference models/yolo/obb/predict.py:10-53.  The device step (forward, OBB decode, ey_nms_rotated) is one captured graph; after the one
    read-back of the counts the kept rows are regularised (w >= h, angle in [0, pi)) and scaled to the original image as xywh.
    Results carry `obb` rows [cx,cy,w,h,rotation,conf,cls]; `boxes` is None."""

    augment_policy = ("warn", "OBBModel")

    def _device_step(self, im):
        pred = self.model(im)[0]
        rows, count, index = ops.nms_device(pred, self.conf, self.iou, self.classes, self.agnostic_nms, self.max_det, nc=len(self.model.names), rotated=True)
        return rows, count, index, pred

    def postprocess(self, rows, count, img, source):
        def one_image(i, k, shape):  # (no whole-batch form: the kept rows are regularised and rebuilt image by image, whatever the frame)
            det = rows[i, :k]
            rboxes = ops.regularize_rboxes(torch.cat([det[:, :4], det[:, -1:]], dim=-1))
            rboxes[:, :4] = ops.scale_boxes(img.shape[2:], rboxes[:, :4], shape, xywh=True)
            return {"obb": torch.cat([rboxes, det[:, 4:6]], dim=-1)}

        return self._assemble(count, img, one_image)


class PosePredictor(DetectionPredictor):
    """reference models/yolo/pose/predict.py:8-56.  The device step is DetectionPredictor's captured graph (fused head decode, candidate NMS)
    plus the cv4 launches of the Pose head and ONE ey_kpts_decode_rows launch that decodes the keypoints of the kept rows by anchor index:
    a fixed (B, max_det, K, ndim) tensor, nothing is decoded for the anchors NMS dropped.  After the one read-back of the counts the boxes
    are scaled and rounded (pose/predict.py:50; detect does not round) and the keypoints go through scale_coords."""

    augment_policy = ("warn", "PoseModel")

    def _device_step(self, im):
        from ..nn import _ops
        head = self.model.model[-1]
        cand, (_, maps) = self.model(im, head_nms={"conf": self.conf, "classes": self.classes, "keep_pred": self.keep_pred})
        boxes, count, index = ops.nms_device(cand, self.conf, self.iou, self.classes, self.agnostic_nms, self.max_det)
        kpts = _ops.kpts_decode_rows(head.kpt_levels(maps), head.kpt_shape, index, count)
        return boxes, count, index, getattr(cand, "pred", None), kpts

    def _results(self, out, im, source):
        return self.postprocess(out[0], out[1], im, source, kpts=out[4])

    def postprocess(self, boxes, count, img, source, kpts=None):
        boxes, kpts = boxes.clone(), kpts.clone()

        def whole_batch(shape):  # one clip (and one rounding of the boxes) over the whole batch
            ops.clip_boxes(boxes, shape)
            boxes[..., :4] = boxes[..., :4].round()
            ops.clip_coords(kpts, shape)

        def one_image(i, k, shape):
            det, kp = boxes[i, :k], kpts[i, :k]
            if shape is not None:
                det[:, :4] = ops.scale_boxes(img.shape[2:], det[:, :4], shape).round()
                kp = ops.scale_coords(img.shape[2:], kp, shape)
            return {"boxes": det, "keypoints": kp}

        return self._assemble(count, img, one_image, whole_batch)


class ClassificationPredictor(DetectionPredictor):
    """reference models/yolo/classify/predict.py:12-60.  Float BCHW tensors in [0,1] go to the network as they are (any H, W: the model has
    no stride constraint); ndarray sources (HWC uint8 BGR) and uint8 (B,h,w,3) tensors go through ClassifyTransform(imgsz) on the device.  The
    device step -- for uint8 tensors the transform too -- is one captured graph: backbone, ey_classify_pool, ey_classify_linear_softmax.
    Results carry `probs` only; its top-5 comes from the head's kernel.  conf, iou, max_det, classes and agnostic_nms are accepted and
    ignored, as in the reference; augment=True raises."""

    # the crop size of ClassifyTransform (the reference's 640 only holds until a checkpoint's train args override it: every released -cls
    # checkpoint says 224)
    imgsz = 224
    augment_policy = ("raise", "classify")

    def _device_step(self, im):
        if im.dtype == torch.uint8:  # a decoded batch: the transform is part of the captured graph
            from ..data.augment import ClassifyTransform
            im = ClassifyTransform(self._u8_size).batch_tensor(im, torch.float16 if self.half else torch.float32)
        probs, logits = self.model(im)
        topi, topp = self.model.model[-1].top5
        return probs, logits, topi, topp

    def preprocess(self, im):
        from ..data.augment import ClassifyTransform
        size = self.imgsz
        if isinstance(im, torch.Tensor) and im.dtype == torch.uint8:
            if im.dim() != 4 or im.shape[3] != 3:
                raise ValueError(f"uint8 tensor sources must be (B,h,w,3) BGR image stacks, got {tuple(im.shape)}")
            if getattr(self, "_u8_size", size) != size and hasattr(self.runner, "graphs"):
                self.runner.graphs.clear()  # the crop size is baked into the captured transform
            self._u8_size = size
            self._orig = [a for a in im.cpu().numpy()]
            return im.contiguous().to(self.device, non_blocking=True)
        if not isinstance(im, torch.Tensor):
            ims = im if isinstance(im, (list, tuple)) else [im]
            self._orig = [np.asarray(a) for a in ims]
            return ClassifyTransform(size).batch(self._orig, self.device, torch.float16 if self.half else torch.float32)
        if im.dim() not in (3, 4):
            raise ValueError(f"input tensor should be BCHW, got {tuple(im.shape)}")
        return self._tensor_source(im, "or uint8 (B,h,w,3) BGR stacks")

    def _results(self, out, im, source):
        return self.postprocess(out[0], im, source, top=(out[2], out[3]))

    def postprocess(self, probs, img, source, top=None):
        """reference classify/predict.py:51-60: one Results with `probs` per image.  One D2H copy each of the probabilities and the top-5."""
        from .results import Probs
        probs = probs.clone()
        top = tuple(t.clone() for t in top) if top is not None else None
        return self._assemble(None, img, lambda i, k, shape: {"probs": Probs(probs[i], top=None if top is None else (top[0][i], top[1][i]))})
