"""-m gpu: FastSAM end to end.  yolov8n-seg at nc = 1 with synthetic weights, B = 2 at 64 x 96, against the reference's forward, kept rows
(after the border / full-box step) and prompt selections (tests/golden/fastsam_yolov8n_64x96.npz; bars of tests/test_gpu_seg_model.py),
with and without the captured graph; a letterboxed ndarray source against the float64 restatement on that run's own masks; and the
memory bound: prompt selection never allocates anything of the original resolution."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import fastsam_synth as fs  # noqa: E402
import fp64_fastsam_ref as f64  # noqa: E402
import seg_synth  # noqa: E402
import synthdata as synth  # noqa: E402

LAYER_TOL = dict(rtol=1e-4, atol=2e-4)  # tests/test_gpu_seg_model.py, fp32


@pytest.fixture(scope="module")
def model():
    import edge_yolo_amd
    m = edge_yolo_amd.FastSAM(fs.MODEL_YAML)
    m.model.load_state_dict(seg_synth.state_dict(m.model.state_dict()))
    return m


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "fastsam_yolov8n_64x96.npz"))


def test_forward_vs_reference_golden(model, gold):
    m = model.model.to("cuda").fuse().float().eval()
    y, (raw, mc, p) = m(synth.synth_images(*fs.MODEL_SHAPE).cuda())
    for name, got in (("y", y), ("mc", mc), ("p", p)):
        np.testing.assert_allclose(got.float().cpu().numpy(), gold[name], err_msg=name, **LAYER_TOL)


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
def test_prompts_select_the_references_instances(model, gold, graph):
    x = synth.synth_images(*fs.MODEL_SHAPE)
    kw = dict(conf=float(gold["conf"]), iou=float(gold["iou"]), device="cuda:0", graph=graph)
    prompts = {"none": {}, "boxes": dict(bboxes=gold["bboxes"]), "points": dict(points=gold["points"], labels=gold["labels"]),
               "both": dict(bboxes=gold["bboxes"], points=gold["points"], labels=gold["labels"])}
    for kind, pk in prompts.items():
        res = model.predict(x, **kw, **pk)
        assert len(res) == fs.MODEL_SHAPE[0]
        for i, r in enumerate(res):
            rows = gold[f"post_boxes{i}"]
            keep = np.ones(len(rows), bool) if kind == "none" else gold[f"keep_{kind}{i}"].astype(bool)
            assert len(r) == int(keep.sum()) and 0 < keep.sum() and (kind == "none" or keep.sum() < len(rows)), (kind, i)
            np.testing.assert_allclose(r.boxes.data.cpu().numpy(), rows[keep], err_msg=f"{kind} image {i}", **LAYER_TOL)
            masks = np.unpackbits(gold[f"masks{i}"])[: len(rows) * 64 * 96].reshape(len(rows), 64, 96)[keep]
            got = r.masks.data.cpu().numpy()
            assert got.shape == masks.shape and r.masks.orig_shape == (64, 96) and r.names == {0: "object"}
            assert float((got != masks.astype(bool)).mean()) < 2e-3  # (bits next to a zero crossing may differ: tests/test_gpu_seg_model.py decides those against float64)
    assert model.predictor.prompts == {}  # consumed: the next call is unprompted
    with pytest.raises(NotImplementedError, match="CLIP"):
        model.predict(x, texts="a dog", **kw)
    with pytest.raises(ValueError, match="outside"):
        model.predict(x, points=[[96, 1]], **kw)
    empty = model.predict(x, conf=0.9999, device="cuda:0", bboxes=gold["bboxes"])  # images without detections pass through untouched
    assert all(len(r) == 0 and r.masks is None for r in empty)


def _decidable_prompts(masks, shape):
    """Box prompts with a float64 gap of 1e-3, far above the kernel's propagated bound (about 1e-5), and robust points, searched on this run's own masks."""
    h, w = shape
    r = np.random.default_rng(3)
    cand = []
    for _ in range(400):
        x1, y1 = int(r.integers(0, w - 1)), int(r.integers(0, h - 1))
        cand.append([x1, y1, int(r.integers(x1 + 1, w + 8)), int(r.integers(y1 + 1, h + 8))])
    ref = f64.prompt64([masks], [shape], cand)[0]
    boxes = [cand[k] for k in np.nonzero(ref["gap"] >= 1e-3)[0][:3]]
    pts = []
    while len(pts) < 3:
        x, y = int(r.integers(0, w)), int(r.integers(0, h))
        if f64.robust_point(masks, shape, x, y):
            pts.append([x, y])
    return boxes, pts, [1, 0, 1]


@pytest.mark.parametrize("orig", [(50, 75), (135, 240)], ids=["50x75", "135x240"])
def test_letterboxed_source_and_memory(model, orig):
    """An ndarray source of another shape is letterboxed to 64 x 96: the prompts are in ORIGINAL pixels and the original-shape geometry
    (for 135 x 240: cropped rows) runs end to end.  The selection equals the float64 restatement on the unprompted run's own masks, and
    the rise of the peak memory during postprocess stays below N H0 W0 bytes -- the resized masks alone, in one byte per pixel, which
    any resize-and-sum implementation exceeds."""
    img = np.random.default_rng(orig[0]).integers(0, 256, (*orig, 3), dtype=np.uint8)
    kw = dict(conf=fs.MODEL_CONF, iou=fs.MODEL_IOU, device="cuda:0", imgsz=96, max_det=50)  # (max_det: the clone of the fixed-size NMS rows stays small)
    base = model.predict(img, **kw)[0]
    n = len(base)
    assert n >= 2 and base.orig_shape == orig and tuple(base.masks.shape) == (n, 64, 96)
    masks = base.masks.data.cpu().numpy().astype(np.uint8)
    boxes, pts, labs = _decidable_prompts(masks, orig)
    assert len(boxes) >= 1
    for pk in (dict(bboxes=boxes), dict(points=pts, labels=labs), dict(bboxes=boxes, points=pts, labels=labs)):
        want = f64.prompt64([masks], [orig], pk.get("bboxes"), pk.get("points"), pk.get("labels"))[0]["keep"]
        r = model.predict(img, **kw, **pk)[0]
        assert len(r) == int(want.sum())
        np.testing.assert_array_equal(r.masks.data.cpu().numpy(), masks[want].astype(bool)) if want.any() else None
        np.testing.assert_array_equal(r.boxes.data.cpu().numpy(), base.boxes.data.cpu().numpy()[want])
    # memory: the device step first, then postprocess alone under the peak counter
    pred = model.predictor
    with torch.cuda.device(pred.device):
        pred._orig = None
        im = pred.preprocess(img)
        out = pred.runner(im)
        torch.cuda.synchronize()
        pred.set_prompts(dict(bboxes=boxes, points=pts, labels=labs))
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        res = pred._results(out, im, img)
        torch.cuda.synchronize()
        rise = torch.cuda.max_memory_allocated() - before
    print(f"{orig}: {n} masks, peak rise during postprocess {rise} bytes, N H0 W0 = {n * orig[0] * orig[1]}")
    assert len(res) == 1
    if orig == (135, 240):  # (at 50 x 75 the network-resolution masks themselves are larger than the original)
        assert rise < n * orig[0] * orig[1]
