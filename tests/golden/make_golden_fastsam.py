"""Golden vectors for FastSAM: scale_masks (reference ultralytics/utils/ops.py:716-737), FastSAMPredictor.prompt and the border / full-box
step of FastSAMPredictor.postprocess (models/fastsam/predict.py:29-103, utils.py:4-24), and a yolov8n-seg nc = 1 model with its prompt
selections, from the real reference imported through _ref_import.  CPU fp32; masks, prompts and weights are synthetic and regenerated
from seeds by tests/fastsam_synth.py / tests/seg_synth.py, so the files hold results only.

    python tests/golden/make_golden_fastsam.py

writes fastsam_ops.npz and fastsam_yolov8n_64x96.npz.  Next to every area the file holds the reference's own fp32 error against the
float64 restatement (tests/fp64_fastsam_ref.py).  The conditions that make the selections decidable are asserted HERE, on the
reference's side: best and second-best IoU of every box prompt at least 1e-3 apart in the op cases (0.05 in the model fixture; the two
tie cases hold an exact tie of a duplicated mask instead), every point robust, no case skipped.  `prompt` runs on CPU on hand-built
Results through object.__new__(FastSAMPredictor).  torchvision.ops.nms is the documented stand-in of make_golden.py (oracle/nms.py).
Runs only where the reference exists.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
import _ref_import  # noqa: E402

tv = _ref_import.setup()
import numpy as np  # noqa: E402
import torch  # noqa: E402
import yaml  # noqa: E402

import fastsam_synth as fs  # noqa: E402
import fp64_fastsam_ref as f64  # noqa: E402
import seg_synth  # noqa: E402
import synthdata as synth  # noqa: E402
from oracle.nms import tv_nms  # noqa: E402

tv.ops.nms = lambda b, s, t: torch.as_tensor(tv_nms(b.numpy(), s.numpy(), t), dtype=torch.long)
from ultralytics.engine.results import Results  # noqa: E402
from ultralytics.models.fastsam.predict import FastSAMPredictor  # noqa: E402
from ultralytics.models.fastsam.utils import adjust_bboxes_to_image_border  # noqa: E402
from ultralytics.nn.tasks import SegmentationModel, guess_model_task  # noqa: E402
from ultralytics.utils import ops as rops  # noqa: E402
from ultralytics.utils.metrics import box_iou  # noqa: E402

torch.set_grad_enabled(False)
CFG = os.path.join(ROOT, "edge-yolo_amd", "cfg", "models", "v8", "yolov8-seg.yaml")


def cfg(scale):
    d = yaml.safe_load(open(CFG, encoding="utf-8"))
    d["scale"] = scale
    return d


def predictor():
    p = object.__new__(FastSAMPredictor)
    p.device = torch.device("cpu")
    return p


def results_of(masks, shapes, boxes=None):
    """hand-built Results: float 0 / 1 masks at the network resolution (what process_mask returns), any boxes of the right count."""
    out = []
    for i, (m, s) in enumerate(zip(masks, shapes)):
        n = len(m)
        b = torch.zeros((n, 6)) if boxes is None else torch.as_tensor(boxes[i], dtype=torch.float32)
        out.append(Results(np.zeros((*s, 3), np.uint8), path=f"image{i}.jpg", names={0: "object"}, boxes=b, masks=torch.tensor(m, dtype=torch.float32) if n else None))
    return out


def selection(before, after):
    """The rows of `before` that `prompt` kept, as a 0 / 1 vector (the masks are compared: boxes are all alike in the op cases)."""
    if len(before) == 0:
        return np.zeros(0, np.uint8)
    kept = np.zeros(len(before), np.uint8)
    a = after.masks.data.numpy() if after.masks is not None else np.zeros((0,))
    j = 0
    for i, m in enumerate(before.masks.data.numpy()):  # result[idx] keeps the order
        if j < len(a) and np.array_equal(a[j], m) and i >= j:
            kept[i] = 1
            j += 1
    assert j == len(a)
    return kept


def reference_areas(m, shape, boxes):
    """predict.py:72-81 in the reference's own fp32: the resized masks, their full sums and their sums inside every box."""
    masks = torch.tensor(m, dtype=torch.float32)
    if tuple(masks.shape[1:]) != tuple(shape):
        masks = rops.scale_masks(masks[None], shape)[0]
    full = torch.sum(masks, dim=(1, 2))
    inter = torch.stack([masks[:, b[1]:b[3], b[0]:b[2]].sum(dim=(1, 2)) for b in torch.as_tensor(boxes, dtype=torch.int32)]) if len(boxes) else torch.zeros((0, len(m)))
    return full.numpy(), inter.numpy()


def check_decidable(tag, c, ref, gap):
    for b, d in enumerate(ref):
        if d is None:
            continue
        for p in range(len(c["boxes"])):
            if c["dup"] and b == 0:
                srt = np.sort(d["iou"][p])
                assert d["iou"][p][c["dup"][0]] == d["iou"][p][c["dup"][1]] == srt[-1] and d["best"][p] == c["dup"][0] and srt[-1] - srt[-3] >= gap, (tag, p)
            else:
                assert d["gap"][p] >= gap, (tag, b, p, d["gap"][p])
    for x, y in c["points"]:
        assert all(f64.robust_point(m, s, int(x), int(y)) for m, s in zip(c["masks"], c["shapes"])), (tag, x, y)


def ops_file():
    d = {}
    for tag, shape, target, padding in fs.SCALE_CASES:
        x = fs.scale_input(tag, shape, "f32")
        got = rops.scale_masks(torch.tensor(x), target, padding=padding).numpy()
        want = f64.scale_masks64(x, target, padding=padding)
        step = max(1, int(np.ceil((got.size / 20000) ** 0.5)))
        d[tag], d[tag + "_step"] = got[..., ::step, ::step], np.int64(step)
        d[tag + "_err"] = np.float64(np.abs(got - want).max())  # the reference's own fp32 error against the restatement
        assert d[tag + "_err"] < 1e-5, (tag, d[tag + "_err"])
        print(tag, got.shape, "err", d[tag + "_err"])
    p = predictor()
    for tag in fs.OP_CASES:
        c = fs.op_case(tag)
        ref = f64.prompt64(c["masks"], c["shapes"], c["boxes"], c["points"], c["labels"])
        check_decidable(tag, c, ref, 1e-3)
        before = results_of(c["masks"], c["shapes"])
        kw = dict(bboxes=c["boxes"] if len(c["boxes"]) else None, points=c["points"] if len(c["points"]) else None, labels=c["labels"] if len(c["points"]) else None)
        after = p.prompt(results_of(c["masks"], c["shapes"]), **kw)
        d[tag + "_seed"] = np.int64(c["seed"])
        for i, (b4, af, m, s, r) in enumerate(zip(before, after, c["masks"], c["shapes"], ref)):
            keep = selection(b4, af)
            d[f"{tag}_keep{i}"] = keep
            if r is None:
                assert len(keep) == 0
                continue
            if not c["dup"]:  # (a tie: the reference's argmax may take either twin; the restatement takes the lower index)
                np.testing.assert_array_equal(keep.astype(bool), r["keep"], err_msg=tag)
            full, inter = reference_areas(m, s, c["boxes"])
            d[f"{tag}_full{i}"], d[f"{tag}_inter{i}"] = full, inter
            d[f"{tag}_full{i}_err"] = np.abs(full - r["full"]) / np.maximum(r["full"], 1e-300)
            d[f"{tag}_inter{i}_err"] = np.abs(inter - r["inter"]) / np.maximum(r["inter"], 1e-300) * (r["inter"] > 0)
            print(tag, i, "kept", keep.tolist(), "max rel err full", float(d[f"{tag}_full{i}_err"].max()), "inter", float(d[f"{tag}_inter{i}_err"].max(initial=0)))
    # the border and full-box step of postprocess (predict.py:36-44) on boxes around every threshold
    for tag, (h, w) in (("border_64x96", (64, 96)), ("border_480x640", (480, 640))):
        r = np.random.default_rng([7, h])
        b = np.concatenate([r.uniform(0, [w, h, w, h], (24, 4)), [[5, 3, w - 4, h - 2], [19.5, 20, w - 20, h - 19.5], [20, 19.9, w - 20.5, h - 21], [0, 0, w, h * 0.91],
                                                                  [0, 0, w * 0.89, h], [30, 0, w, h], [21, 21, w - 21, h - 21]]]).astype(np.float32)
        b[:, 2:] = np.maximum(b[:, 2:], b[:, :2] + 1)
        boxes = adjust_bboxes_to_image_border(torch.tensor(b), (h, w))
        full = torch.tensor([0, 0, w, h], dtype=torch.float32)
        idx = torch.nonzero(box_iou(full[None], boxes) > 0.9).flatten()
        boxes[idx] = full
        d[tag + "_in"], d[tag + "_out"] = b, boxes.numpy()
        assert len(idx) >= 2 and len(idx) < len(b)
    # yolov8s-seg at nc = 1: what FastSAM("FastSAM-s.yaml") must build
    m = SegmentationModel(cfg("s"), ch=3, nc=1, verbose=False)
    assert guess_model_task(m) == "segment"
    d["structure_s_keys"] = np.array(list(m.state_dict()))
    d["structure_s_shapes"] = np.array([",".join(str(v) for v in t.shape) for t in m.state_dict().values()])
    d["structure_s_types"] = np.array([l.type for l in m.model])
    d["structure_s_params"] = np.int64(sum(p.numel() for p in m.parameters()))
    path = os.path.join(HERE, "fastsam_ops.npz")
    np.savez_compressed(path, **d)
    print("fastsam_ops", len(d), os.path.getsize(path))
    assert os.path.getsize(path) < 1 << 20


def model_prompts(masks, dets, shape):
    """Box prompts -- the extents of the kept masks first, then seeded random boxes -- whose best IoU leads by 0.05 in EVERY image under the
    float64 restatement (the prompts are shared by the batch), and robust points inside masks of the first image."""
    h, w = shape
    ms = [mm.numpy() for mm in masks]
    cand = []
    for m in ms:
        for mk in m:
            ys, xs = np.nonzero(mk)
            if len(ys):
                cand.append([int(xs.min()), int(ys.min()), int(xs.max()) + 1, int(ys.max()) + 1])
    r = np.random.default_rng(20)
    for _ in range(2000):
        x1, y1 = int(r.integers(0, w - 1)), int(r.integers(0, h - 1))
        cand.append([x1, y1, int(r.integers(x1 + 1, w + 1)), int(r.integers(y1 + 1, h + 1))])
    ref = f64.prompt64(ms, [shape] * len(ms), cand)
    gap = np.min([d["gap"] for d in ref], 0)
    boxes = []
    for k in np.nonzero(gap >= 0.05)[0]:
        if cand[k] not in boxes and len(boxes) < 3:
            boxes.append(cand[k])
    pts = []
    for mk in ms[0]:
        ys, xs = np.nonzero(mk)
        if len(ys) and len(pts) < 3:
            x, y = int(xs[len(xs) // 2]), int(ys[len(ys) // 2])
            if [x, y] not in pts and all(f64.robust_point(m, shape, x, y) for m in ms):
                pts.append([x, y])
    assert len(boxes) >= 2 and len(pts) >= 2, (boxes, pts, float(gap.max()))
    return np.array(boxes, np.int32), np.array(pts, np.int32), np.array([1, 0, 1][:len(pts)], np.int32)


def model_file():
    b, h, w = fs.MODEL_SHAPE
    m = SegmentationModel(cfg("n"), ch=3, nc=1, verbose=False).eval()
    m.load_state_dict(seg_synth.state_dict(m.state_dict()))
    m.fuse(verbose=False)
    x = synth.synth_images(b, h, w)
    y, (raw, mc, p) = m(x)
    assert torch.isfinite(y).all() and tuple(p.shape[2:]) == (h // 4, w // 4)
    d = {"y": y, "mc": mc, "p": p, "conf": np.float64(fs.MODEL_CONF), "iou": np.float64(fs.MODEL_IOU)}
    dets = rops.non_max_suppression(y.clone(), fs.MODEL_CONF, fs.MODEL_IOU, nc=1, max_det=300, max_time_img=1e6)
    masks = [rops.process_mask(p[i], det[:, 6:], det[:, :4].clone(), (h, w), upsample=True) for i, det in enumerate(dets)]
    assert sum(len(t) for t in dets) >= 5 and all(len(t) >= 2 for t in dets), [len(t) for t in dets]
    boxes, pts, labs = model_prompts(masks, dets, (h, w))
    d["bboxes"], d["points"], d["labels"] = boxes, pts, labs
    fp = predictor()
    for i, det in enumerate(dets):
        d[f"det{i}"] = det
        d[f"masks{i}"] = np.packbits(masks[i].numpy().astype(np.uint8))
    # postprocess (predict.py:29-46) from the Results on: scale_boxes is the identity for a tensor source, clip_boxes is applied by super()
    res = []
    for i, det in enumerate(dets):
        rows = det[:, :6].clone()
        rops.clip_boxes(rows[:, :4], (h, w))
        res.append(Results(np.zeros((h, w, 3), np.uint8), path=f"image{i}.jpg", names={0: "object"}, boxes=rows, masks=masks[i]))
    for r in res:
        full = torch.tensor([0, 0, r.orig_shape[1], r.orig_shape[0]], dtype=torch.float32)
        bx = adjust_bboxes_to_image_border(r.boxes.xyxy, r.orig_shape)
        idx = torch.nonzero(box_iou(full[None], bx) > 0.9).flatten()
        if idx.numel() != 0:
            r.boxes.xyxy[idx] = full
    for i, r in enumerate(res):
        d[f"post_boxes{i}"] = r.boxes.data.clone()
    ref = f64.prompt64([mm.numpy() for mm in masks], [(h, w)] * b, boxes, pts, labs)
    for kind, kw in (("boxes", dict(bboxes=boxes)), ("points", dict(points=pts, labels=labs)), ("both", dict(bboxes=boxes, points=pts, labels=labs))):
        out = fp.prompt(list(res), **kw)
        want = f64.prompt64([mm.numpy() for mm in masks], [(h, w)] * b, kw.get("bboxes"), kw.get("points"), kw.get("labels"))
        for i, (b4, af) in enumerate(zip(res, out)):
            keep = selection(b4, af)
            np.testing.assert_array_equal(keep.astype(bool), want[i]["keep"])
            d[f"keep_{kind}{i}"] = keep
            print("model", kind, i, keep.tolist())
    assert all(r["gap"].min() >= 0.05 for r in ref)
    path = os.path.join(HERE, "fastsam_yolov8n_64x96.npz")
    np.savez_compressed(path, **{k: (v.numpy() if torch.is_tensor(v) else v) for k, v in d.items()})
    print("fastsam_yolov8n_64x96", len(d), [len(t) for t in dets], os.path.getsize(path))
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    ops_file()
    model_file()
