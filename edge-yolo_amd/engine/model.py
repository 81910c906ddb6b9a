"""`YOLO(...)` facade for the detect, segment, obb, pose and classify tasks, mirroring the reference's engine/model.py (`Model.__init__` :84-151,
`_new` :231-264, `_load` :266-302, `predict` :501-560, `val` :599-655) and models/yolo/model.py (:11-59)."""
from pathlib import Path

import torch

from .predictor import ClassificationPredictor, DetectionPredictor, FastSAMPredictor, OBBPredictor, PosePredictor, SegmentationPredictor
from .validator import ClassificationValidator, DetectionValidator, FastSAMValidator, OBBValidator, PoseValidator, SegmentationValidator  # noqa: F401 (OBBValidator: re-exported)
from ..nn.tasks import ClassificationModel, DetectionModel, OBBModel, PoseModel, SegmentationModel, WorldModel, guess_model_task, torch_safe_load_state, yaml_model_load


def _plain(o):
    """YAML dict -> containers torch.load(weights_only=True) accepts (dict / list / str / int / float / bool / None)."""
    if isinstance(o, dict):
        return {str(k): _plain(v) for k, v in o.items()}
    if isinstance(o, (list, tuple)):
        return [_plain(v) for v in o]
    if isinstance(o, (str, int, float, bool)) or o is None:
        return o
    return str(o)


_TASK_MAP = {"detect": {"model": DetectionModel, "predictor": DetectionPredictor, "validator": DetectionValidator},
             "segment": {"model": SegmentationModel, "predictor": SegmentationPredictor, "validator": SegmentationValidator}}
# tasks outside `task_map` (whose key set is pinned to the two tasks above): `_task_entry()` falls back to this table.  A row without a
# "validator" has none that val() picks by itself: the obb row stays that way because the plain `val(loader)` refusal is pinned, and its
# validator is handed in by name, `val(loader, validator=OBBValidator)` (rotated mAP on ey_nms_rotated_ml and ey_probiou_batch)
_PREDICT_TASKS = {"obb": {"model": OBBModel, "predictor": OBBPredictor},
                  "pose": {"model": PoseModel, "predictor": PosePredictor, "validator": PoseValidator},
                  "classify": {"model": ClassificationModel, "predictor": ClassificationPredictor, "validator": ClassificationValidator}}


class Model(torch.nn.Module):
    def __init__(self, model="yolo11n.yaml", task=None, verbose=False, nc=None):
        """nc (extension): number of classes for a model built from a YAML (the reference takes it from the dataset YAML at train time,
        engine/trainer.py; checkpoints written by save() carry it)."""
        super().__init__()
        self.predictor = None
        self.model = None
        self.overrides = {}
        self.ckpt_path = None
        self.task = task
        if isinstance(model, dict):  # (extension) an already loaded YAML dict
            self._new(model, task=task, verbose=verbose, nc=nc)
            return
        model = str(model).strip()
        if Path(model).suffix in {".yaml", ".yml"}:
            self._new(model, task=task, verbose=verbose, nc=nc)
        else:
            self._load(model, task=task)

    def _new(self, cfg, task=None, model=None, verbose=False, nc=None):
        cfg_dict = cfg if isinstance(cfg, dict) else yaml_model_load(cfg)
        self.cfg = cfg
        # the reference raises NotImplementedError here for GFLHeadv2_uniH YAMLs unless task="detect" is passed
        # (engine/model.py:1096-1103 via tasks.py:1198-1210); the argument is accepted but not required
        self.task = task or guess_model_task(cfg_dict)
        if self.task not in self.task_map and self.task not in _PREDICT_TASKS:
            raise NotImplementedError(f"task '{self.task}': only {sorted(self.task_map) + sorted(_PREDICT_TASKS)} are built")
        self.model = self._task_entry()["model"](cfg_dict, nc=nc, verbose=verbose)
        if guess_model_task(self.model) != self.task:
            raise ValueError(f"task '{self.task}' does not match the model's head ({type(self.model.model[-1]).__name__})")
        self.overrides["model"] = self.cfg
        self.overrides["task"] = self.task
        self.model.task = self.task
        self.model_name = cfg_dict.get("yaml_file", "model") if isinstance(cfg, dict) else cfg

    def _load(self, weights, task=None):
        """Tensor-only checkpoints written by `save()`: {'yaml': <name or dict>, 'nc': int, 'fused': bool, 'state_dict': {...}}.
        Pickled reference checkpoints (module objects, tasks.py:815-955) are never unpickled here; tools/export_reference_weights.py
        turns one into this format on a machine that has the reference installed."""
        ck = torch_safe_load_state(weights)
        if not isinstance(ck, dict) or "state_dict" not in ck or "yaml" not in ck:
            raise ValueError(f"{weights}: expected a tensor-only checkpoint with 'yaml' and 'state_dict' entries (see YOLO.save)")
        cfg = ck["yaml"]
        if ck.get("nc") is not None:
            cfg = dict(yaml_model_load(cfg)) if not isinstance(cfg, dict) else dict(cfg)
            cfg["nc"] = int(ck["nc"])
        self._new(cfg, task=task)
        if bool(ck.get("fused", False)):
            self.model.fuse()  # the checkpoint holds BN-folded conv weights + biases (saved after predict()): same module layout first
        loaded, own = self.model.load(ck["state_dict"])
        if loaded != own:
            missing = sorted(set(self.model.state_dict()) - set(ck["state_dict"]))[:5]
            raise ValueError(f"{weights}: only {loaded} of {own} model tensors were found in the checkpoint (e.g. missing {missing}); "
                             "was it saved from a different YAML / nc, or fused without the 'fused' flag?")
        self._restore_extra(ck)
        self.ckpt_path = weights

    def save(self, filename):
        """Tensor-only checkpoint (readable with torch.load(weights_only=True)).  predict() folds BatchNorm into the convs in place
        (reference AutoBackend does the same, autobackend.py:144-155); the 'fused' flag records which layout the tensors have."""
        m = self.model
        sd = {k: v.detach().float().cpu() if v.is_floating_point() else v.detach().cpu() for k, v in m.state_dict().items()}
        # a model built from a dict (a custom architecture, or any model that went through _load) is saved WITH that dict: a path string
        # would only reload where a file of that name exists under cfg/models and still describes the same graph
        cfg = _plain(m.yaml) if isinstance(self.cfg, dict) else self.cfg
        torch.save({"yaml": cfg, "nc": int(m.yaml["nc"]),
                    "fused": bool(m.convs_folded()), "state_dict": sd, **self._checkpoint_extra()}, filename)

    def _checkpoint_extra(self):
        """Further checkpoint entries of a subclass (YOLOWorld: the class names); none here, so other checkpoints keep their exact content."""
        return {}

    def _restore_extra(self, ck):
        """Counterpart of _checkpoint_extra, called by _load behind the state_dict."""

    def load(self, weights):
        """Load a flat state_dict (dict or tensor-only file) keyed like the reference's `model.N....` entries."""
        sd = torch_safe_load_state(weights) if isinstance(weights, (str, Path)) else weights
        self.model.load(sd)
        self.predictor = None
        return self

    @property
    def task_map(self):
        """task -> {model class, predictor class, validator class} (reference engine/model.py:1062-1064, models/yolo/model.py:24-59)."""
        return _TASK_MAP

    def _task_entry(self):
        """classes of this model's task: its `task_map` row, or its row of the side table (which may lack a "validator")."""
        return self.task_map[self.task] if self.task in self.task_map else _PREDICT_TASKS[self.task]

    @property
    def names(self):
        return self.model.names

    @property
    def device(self):
        return next(self.model.parameters()).device

    def fuse(self):
        self.model.fuse()
        return self

    def _select_device(self, device):
        if device in (None, ""):
            device = "cuda:0"
        if isinstance(device, int):
            device = f"cuda:{device}"
        device = torch.device(device)
        if device.type != "cuda" or not torch.cuda.is_available():
            raise RuntimeError(f"device '{device}': edge-yolo_amd runs on MI355X (ROCm 'cuda' devices) only; there is no CPU path. "
                               "(BASELINE configs[0], the CPU plumbing case, is the reference's own CPU predictor.)")
        return device

    def _ready(self, device, half):
        """The model on `device`, fused, in the run's dtype, in eval mode -- in AutoBackend's order (reference nn/autobackend.py:144-155):
        to(device) -> fuse() -> half()/float()."""
        m = self.model.to(device)
        m.fuse()
        m = m.half() if half else m.float()
        return m.eval()

    @staticmethod
    def _options(caller, defaults, kwargs, ignored):
        """defaults overridden by the caller's kwargs; names outside `defaults` and `ignored` (accepted for the reference's sake, unused) raise."""
        unknown = set(kwargs) - set(defaults) - set(ignored)
        if unknown:
            raise TypeError(f"{caller}() got unsupported arguments {sorted(unknown)}")
        return {**defaults, **{k: v for k, v in kwargs.items() if k in defaults}}

    def predict(self, source=None, stream=False, predictor=None, prompts=None, **kwargs):
        """prompts (reference engine/model.py:554-555): handed to the predictor's `set_prompts` where it has one (FastSAM).  kwargs (reference cfg/default.yaml:51-65 names): imgsz, half, conf, iou, max_det, agnostic_nms, classes, device, augment.
        predictor (reference engine/model.py:505,552: `(predictor or self._smart_load("predictor"))(overrides=...)`): a predictor CLASS to use
        instead of the task's default; it is constructed with DetectionPredictor's signature (see there) and called with the source."""
        if source is None:
            raise ValueError("predict() needs a source: a BCHW float tensor in [0,1] or HWC uint8 BGR ndarray(s)")
        if predictor is not None and not callable(predictor):
            raise TypeError(f"predict(predictor=...): expected a predictor class (constructed like DetectionPredictor), got {type(predictor).__name__}")
        pcls = predictor or self._task_entry()["predictor"]
        for name, why in getattr(pcls, "refused_options", {}).items():  # the task's keywords that may only be switched off
            if kwargs.pop(name, False):
                raise NotImplementedError(why)
        args = self._options("predict", {"conf": 0.25, "iou": 0.7, "max_det": 300, "half": False, "agnostic_nms": False, "classes": None, "device": None,
                                         "graph": True, "augment": False}, kwargs, {"imgsz", "verbose", "batch", "save", "mode"})
        device = self._select_device(args["device"] if args["device"] is not None else (source.device if isinstance(source, torch.Tensor) and source.is_cuda else None))
        key = tuple((k, str(v)) for k, v in sorted(args.items())) + (("dev", str(device)), ("predictor", pcls))
        if self.predictor is None or self._pred_key != key:
            if self.predictor is not None:  # options changed: release the old predictor's graphs before anything new is captured
                self.predictor.close()
                self.predictor = None
            m = self._ready(device, args["half"])
            self.predictor = pcls(m, device, half=args["half"], conf=args["conf"], iou=args["iou"], max_det=args["max_det"],
                                  agnostic_nms=args["agnostic_nms"], classes=args["classes"], graph=args["graph"], augment=args["augment"])
            self._pred_key = key
        # the size ndarray sources are brought to: this call's, or the default the predictor's class states
        self.predictor.imgsz = kwargs.get("imgsz", getattr(pcls, "imgsz", DetectionPredictor.imgsz))
        if prompts and hasattr(self.predictor, "set_prompts"):
            self.predictor.set_prompts(prompts)
        results = self.predictor(source)
        return iter(results) if stream else results

    __call__ = predict

    def track(self, source=None, stream=False, persist=False, tracker=None, **kwargs):
        """predict() followed by ByteTrack (reference engine/model.py `track`, trackers/track.py:53-87): image i of the batch is video stream i,
        and every call is the next frame of each stream.  All streams advance in ONE ey_bytetrack_update launch, on the rows predict() returns
        (original-image pixels); the tracks never leave the device.  An image with detections and returned tracks becomes `results[i][idx]`
        (masks and keypoints follow their rows) with boxes [x1, y1, x2, y2, id, conf, cls]; an image without detections, or without returned
        tracks, keeps its untracked Results (`boxes.id is None`).
        persist: keep the tracks from the last call (a new batch size, max_det, device or tracker settings start afresh); without it every call
        starts new trackers, as the reference does.  tracker: None, a dict or a YAML path with ByteTrack's settings (trackers.load_settings).
        kwargs: predict()'s, conf defaults to 0.1 (ByteTrack wants the low-score detections); max_tracks (extension): slots per stream, 1024."""
        from ..trackers import BYTETracker, load_settings
        if self.task in ("obb", "classify"):
            raise NotImplementedError(f"track(): the '{self.task}' task is not tracked (built: detect, segment, pose)")
        settings = load_settings(tracker)
        max_tracks = int(kwargs.pop("max_tracks", 1024))
        kwargs.setdefault("conf", 0.1)
        results = self.predict(source, **kwargs)
        B, cap, dev = len(results), int(self.predictor.max_det), self.predictor.device
        key = (B, cap, max_tracks, str(dev), tuple(sorted(settings.items())))
        if not persist or getattr(self, "_tracker", None) is None or self._tracker_key != key:
            self._tracker, self._tracker_key = BYTETracker(settings, streams=B, max_det=cap, max_tracks=max_tracks, device=dev), key
        with torch.cuda.device(dev):
            rows = torch.zeros((B, cap, 6), dtype=torch.float32, device=dev)
            n = [min(len(r.boxes), cap) for r in results]
            for i, r in enumerate(results):
                if n[i]:
                    rows[i, :n[i]] = r.boxes.data[:n[i], :6]
            tracks, _, counts = self._tracker.update(rows, torch.tensor(n, dtype=torch.int32).to(dev))
            for i, k in enumerate(counts.tolist()):
                if n[i] == 0 or k == 0:
                    continue
                r = results[i][tracks[i, :k, 7].long()]
                r.boxes = type(r.boxes)(tracks[i, :k, :7].to(results[i].boxes.data.dtype), r.boxes.orig_shape)
                results[i] = r
        return iter(results) if stream else results

    def val(self, dataloader=None, validator=None, **kwargs):
        """Validate on an iterable of batches in the reference's collate format (engine/validator.py::DetectionValidator; the segment task
        adds "masks", see SegmentationValidator; the pose task "keypoints", see PoseValidator) and return the results dict (reference
        engine/model.py:599-655 returns validator.metrics; datasets and dataloaders are the caller's).  kwargs (reference cfg/default.yaml
        names): conf (default 0.001), iou, max_det, half, single_cls, agnostic_nms, device, and what the validator class adds in its
        `val_options` (segment: overlap_mask -- True: one index map per image --; save_json / save_txt / plots, which are not built and raise
        when set).  validator: a validator CLASS to use instead of the task's; the obb task has no default one and takes
        `validator=OBBValidator` (engine.validator: rotated mAP, batches with (N, 5) "bboxes" = normalised xywh + angle)."""
        if validator is None and "validator" not in self._task_entry():
            raise NotImplementedError(f"val(): the '{self.task}' task has no default validator (obb: pass the class, "
                                      "val(loader, validator=OBBValidator) from engine.validator, for rotated mAP)")
        if dataloader is None:
            raise ValueError("val() needs an iterable of batch dicts (see DetectionValidator); datasets are not part of this build")
        vcls = validator or self._task_entry()["validator"]
        args = self._options("val", {"conf": 0.001, "iou": 0.7, "max_det": 300, "half": False, "single_cls": False, "agnostic_nms": False, "device": None,
                                     **getattr(vcls, "val_options", {})}, kwargs, {"imgsz", "verbose", "batch", "mode"})
        device = self._select_device(args.pop("device"))
        if self.predictor is not None:  # the model's dtype may change below: a captured predict graph must not outlive it
            self.predictor.close()
            self.predictor = None
        v = vcls(self._ready(device, args["half"]), device=device, **args)
        self.metrics = v(dataloader)
        self.validator = v
        return self.metrics

    def predict_batches(self, batches, stages=4, **kwargs):
        """Throughput form of predict(): a generator over an iterable of BCHW float tensors in [0,1] (all of one shape; host or device,
        pinned host fp16/fp32 tensors upload fastest) -- or of decoded image batches, uint8 tensors (B,h,w,3) in BGR order like a stack
        of cv2 images (3 bytes per pixel over PCIe instead of 6; LetterBox to `imgsz` (default 640, minimum rectangle) + BGR->RGB + CHW + /255
        run on the device in one launch, boxes are scaled back to (h,w) like the reference does for image sources) -- that yields one list of
        Results per batch, in order.  The layer list is cut into
        `stages` pipeline stages (engine/predictor.py::PipelinedRunner: one hipGraph and one HIP stream per stage; batch i's head/NMS
        run beside batch i+1's neck and batch i+2's backbone), host batches are uploaded on a copy stream under the batches in flight,
        and the detection counts come back through a pinned buffer, so the only host waits are on events.  The results of a batch
        arrive `stages` submissions later (one buffer set per stage plus one for the upload in flight).  Same kwargs as predict() (conf, iou, max_det, half, agnostic_nms, classes, device).
        The reference has no counterpart (its stream=True generator still runs one batch at a time)."""
        from .predictor import PipelinedRunner
        from ..utils import ops
        if self.task != "detect":
            raise NotImplementedError(f"predict_batches: pipelined throughput is built for the detect task only, not '{self.task}' (use predict(); "
                                      "built tasks: detect, segment, obb, pose, classify)")
        if isinstance(self.model.model[0], torch.nn.Identity):
            raise NotImplementedError("predict_batches: layer 0 of this model is nn.Identity, not a conv (yolov9e): a later layer reads the input image itself "
                                      "and the CBLinear layers hand tuples on, which the pipeline stages' static buffers do not carry; use predict()")
        args = self._options("predict_batches", {"conf": 0.25, "iou": 0.7, "max_det": 300, "half": False, "agnostic_nms": False, "classes": None, "device": None},
                             kwargs, {"imgsz", "verbose", "cuts"})
        pipe, post, pending, nset, dev_ctx = None, None, [], 0, None
        u8, lb, stage_u8, origs, upload = False, None, None, None, None
        try:
            for x in batches:
                if pipe is None:
                    u8 = x.dtype == torch.uint8
                    if u8 and (x.dim() != 4 or x.shape[3] != 3):
                        raise ValueError(f"predict_batches: uint8 batches must be (B,h,w,3) image stacks, got {tuple(x.shape)}")
                    device = self._select_device(args["device"] if args["device"] is not None else (x.device if x.is_cuda else None))
                    dev_ctx = torch.cuda.device(device)
                    dev_ctx.__enter__()
                    m = self._ready(device, args["half"])
                    post = DetectionPredictor(m, device, half=args["half"], conf=args["conf"], iou=args["iou"], max_det=args["max_det"],
                                              agnostic_nms=args["agnostic_nms"], classes=args["classes"], graph=False)
                    n = len(m.model)
                    stages = max(2, min(int(stages), n))
                    cuts = sorted({max(1, round(0.39 * (n - 1))), max(2, round(0.87 * (n - 1))), n - 1})[-(stages - 1):]
                    if kwargs.get("cuts"):
                        cuts = sorted(int(c) for c in kwargs["cuts"])
                    bounds = [0] + cuts + [n]
                    hn = {"conf": args["conf"], "classes": args["classes"]}  # the head stage also builds the NMS candidates (fused decode)
                    fns = [(lambda st, lo=lo, hi=hi: m.forward_layers(st if lo else (st, []), lo, hi, head_nms=hn)) for lo, hi in zip(bounds[:-1], bounds[1:])]
                    last = fns.pop()
                    fns.append(lambda st, last=last: ops.nms_device(last(st)[0][0], args["conf"], args["iou"], args["classes"], args["agnostic_nms"], args["max_det"])[:2])
                    head = m.model[-1]
                    fork, head.head_streams = getattr(head, "head_streams", False), False  # the head is a pipeline stage of its own: no fork inside it
                    dt = torch.float16 if args["half"] else torch.float32
                    if u8:
                        from ..data.augment import LetterBox
                        stride = int(max(m.stride)) if hasattr(m, "stride") else 32
                        lb = LetterBox(kwargs.get("imgsz", DetectionPredictor.imgsz), auto=True, stride=stride)  # as predict() letterboxes a list of same-shape images
                        example = lb.batch_tensor(x.contiguous().to(device), dt)
                        u8_shape = tuple(x.shape)
                    else:
                        example = post.preprocess(x)
                    try:
                        pipe = PipelinedRunner(*fns, example, copy_stream=True)
                    finally:
                        head.head_streams = fork
                    nset = pipe.nsets
                    counts = [torch.empty(x.shape[0], dtype=torch.int32).pin_memory() for _ in range(nset)]
                    ready = [torch.cuda.Event() for _ in range(nset)]
                    # Image batches in pinned memory are NOT uploaded with a copy: the conversion kernel reads them over PCIe itself (pinned
                    # memory is mapped into the device's address space): 2.2 ms per batch instead of 2.9 with a DMA copy + conversion.
                    # On this stack neither form of transfer overlaps much with the kernels of other streams (a host-reading kernel beside
                    # 400 matmuls: 5.6 ms of transfers stretch them from 11.4 to 14.7 ms; DMA copies wait for them altogether), so a
                    # host batch costs about compute + transfer; 3 bytes per pixel is what helps.
                    if u8:
                        stage_u8 = [None] * nset
                        origs = [None] * nset

                        def upload(dst, src, j):  # ONE conversion launch (LetterBox + BGR->RGB + CHW + /255) on the first stage's stream
                            if not src.is_cuda and src.is_pinned():
                                return lambda: lb.batch_tensor(src, dt, out=dst)
                            if stage_u8[j] is None:
                                stage_u8[j] = torch.empty(u8_shape, dtype=torch.uint8, device=device)
                            stage_u8[j].copy_(src, non_blocking=True)
                            return lambda: lb.batch_tensor(stage_u8[j], dt, out=dst)
                    else:
                        origs = [None] * nset
                if u8:
                    if x.dtype != torch.uint8 or tuple(x.shape) != u8_shape:
                        raise ValueError(f"predict_batches: every batch must be a uint8 tensor of shape {u8_shape}, got {x.dtype} {tuple(x.shape)}")
                    x = x.contiguous()
                else:
                    if x.dim() != 4 or tuple(x.shape) != tuple(pipe.static_input(0).shape):  # checked for EVERY float batch, converted or not
                        raise ValueError(f"predict_batches: every batch must have shape {tuple(pipe.static_input(0).shape)}, got {tuple(x.shape)}")
                    if not x.is_cuda and x.dtype != dt:  # a dtype-changing H2D copy would convert on the host: upload as is, convert on the device
                        x = post.preprocess(x)
                while pending and (len(pending) >= nset or pending[0] == pipe.i % nset):  # the buffer set about to be reused must be read first
                    yield self._finish(pipe, post, pending.pop(0), counts, ready, origs)
                # float host batches: DMA on a stream of its own (measured faster than the host-reading copy kernel for 6-byte pixels);
                # image batches: the conversion kernel reads pinned memory itself; device batches: a device copy ahead of stage 0
                j = pipe.submit(x, upload=upload, side_copy=not u8 and not x.is_cuda)
                origs[j] = x  # (keeps a pinned host batch alive and, for image batches, is what the Results refer to)
                with torch.cuda.stream(pipe.sp):  # counts -> pinned host memory right behind this batch's NMS; the host later waits on the event only
                    counts[j].copy_(pipe.outputs(j)[1], non_blocking=True)
                    ready[j].record(pipe.sp)
                pending.append(j)
            while pending:
                yield self._finish(pipe, post, pending.pop(0), counts, ready, origs)
        finally:
            if dev_ctx is not None:
                dev_ctx.__exit__(None, None, None)

    @staticmethod
    def _finish(pipe, post, j, counts, ready, origs=None):
        ready[j].synchronize()
        boxes, _ = pipe.outputs(j)
        # image sources: boxes go back to the original image frame (reference detect/predict.py:36-39); the originals are views of the host batch
        src = origs[j] if origs is not None else None
        if src is not None and src.dtype != torch.uint8:
            src = None  # (float tensors are network inputs, not images: tensor-source semantics)
        post._orig = [src[i].numpy() if not src.is_cuda else src[i] for i in range(src.shape[0])] if src is not None else None
        return post.postprocess(boxes, counts[j], pipe.static_input(j), None)


class YOLO(Model):
    """YOLO detect model (reference models/yolo/model.py:11-59)."""

    def __init__(self, model="yolo11n.yaml", task=None, verbose=False, nc=None):
        super().__init__(model=model, task=task, verbose=verbose, nc=nc)

    @property
    def task_map(self):
        return _TASK_MAP


_WORLD_TASK_MAP = {"detect": {"model": WorldModel, "predictor": DetectionPredictor, "validator": DetectionValidator}}


class YOLOWorld(Model):
    """YOLO-World open-vocabulary detect model (reference models/yolo/model.py:62-111).  predict(), val(), save() and loading work as for any
    detect model; `set_classes` chooses the vocabulary at run time.  The CLIP text encoder is not part of the build, so `set_classes` takes the
    embeddings of the class names next to the names."""

    def __init__(self, model="yolov8s-worldv2.yaml", verbose=False):
        super().__init__(model=model, task="detect", verbose=verbose)

    @property
    def task_map(self):
        return _WORLD_TASK_MAP

    def set_classes(self, classes, txt_feats=None):
        """classes: the class names; txt_feats: their embeddings (n, 512) or (1, n, 512) (required: WorldModel.set_classes).  A " " background
        entry keeps its embedding and is removed from the names, as in the reference (:102-106).  A live predictor is closed: its captured
        graphs were recorded for the old vocabulary."""
        classes = list(classes)
        self.model.set_classes(classes, txt_feats)
        background = " "
        if background in classes:
            classes.remove(background)
        self.model.names = dict(enumerate(classes))
        if self.predictor is not None:
            self.predictor.model.names = self.model.names
            self.predictor.close()
            self.predictor = None

    def _checkpoint_extra(self):
        return {"names": [str(self.model.names[i]) for i in sorted(self.model.names)]}

    def _restore_extra(self, ck):
        if ck.get("names") is not None:
            self.model.names = dict(enumerate(str(n) for n in ck["names"]))

    def predict_batches(self, batches, stages=4, **kwargs):
        raise NotImplementedError("predict_batches: the pipelined stages are built and verified for fixed-vocabulary detect models only; a YOLOWorld model, "
                                  "whose neck and head depend on the vocabulary set at run time, runs through predict()")


_FASTSAM_TASK_MAP = {"segment": {"model": SegmentationModel, "predictor": FastSAMPredictor, "validator": FastSAMValidator}}
_FASTSAM_YAMLS = {"FastSAM-s": "yolov8s-seg.yaml", "FastSAM-x": "yolov8x-seg.yaml"}


class FastSAM(Model):
    """FastSAM (reference models/fastsam/model.py:11-55): a single-class yolov8{s,x}-seg whose predictor returns only the instances that box
    and point prompts select.  `model`: a tensor-only checkpoint (see YOLO.save), or -- unlike the reference, which ships weights and refuses
    YAMLs (:28) while this build downloads nothing -- a YAML: "FastSAM-s.yaml" / "FastSAM-x.yaml" are yolov8s-seg.yaml / yolov8x-seg.yaml
    with nc = 1, and any other segment YAML is built with nc = 1 too.  The class is named "object"."""

    def __init__(self, model="FastSAM-x.yaml", verbose=False):
        name = str(model).strip() if not isinstance(model, dict) else None
        if name == "FastSAM.pt":
            name = "FastSAM-x.pt"
        if name is not None and Path(name).suffix in {".yaml", ".yml"}:
            cfg = dict(yaml_model_load(_FASTSAM_YAMLS.get(Path(name).stem, name)))
            cfg["yaml_file"] = name
            model = cfg
        elif name is not None:
            model = name
        super().__init__(model=model, task="segment", verbose=verbose, nc=1 if isinstance(model, dict) else None)
        if len(self.model.names) == 1:
            self.model.names = {0: "object"}

    @property
    def task_map(self):
        return _FASTSAM_TASK_MAP

    def predict(self, source=None, stream=False, bboxes=None, points=None, labels=None, texts=None, **kwargs):
        """predict() of the segment task plus prompts in ORIGINAL-image pixels, shared by all images of the call (reference :34-50): bboxes
        (P,4) x1,y1,x2,y2 -- each keeps the mask of the highest IoU with it --, points (Q,2) x,y with labels (Q,) (1 = keep the masks
        under the point, 0 = drop them; default 1).  Without prompts every instance is returned.  texts raises NotImplementedError: the
        CLIP encoder is not part of the build (as YOLOWorld.set_classes takes embeddings)."""
        FastSAMPredictor.check_prompts(bboxes, points, labels, texts)
        return super().predict(source, stream=stream, prompts=dict(bboxes=bboxes, points=points, labels=labels, texts=texts), **kwargs)

    __call__ = predict

    def predict_batches(self, batches, stages=4, **kwargs):
        raise NotImplementedError("predict_batches: pipelined throughput is built for the detect task only, not 'segment' (use predict())")
