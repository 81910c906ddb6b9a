"""-m gpu: YOLO-World v2 end to end.  yolov8n-worldv2 (64x96, B = 2, synthetic weights, a 5-text vocabulary set after construction) against
the reference's forward (tests/golden/yolov8n_worldv2_64x96.npz) at the parity bars of tests/test_gpu_yolov12.py (y: rtol 1e-4, atol 1e-3; raw
levels: rtol 1e-4, atol 2e-4) and the f16 bar of tests/test_gpu_obb_model.py (scores within 2e-2, boxes within 1.5 % of the image size); the
modules against tests/golden/world_ops.npz at the fp32 layer bar; YOLOWorld.predict() with and without the captured graph, against the
reference's NMS rows, and across a change of vocabulary; val(); and predict_batches, which a world model refuses."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import synthdata as synth  # noqa: E402
import world_synth as ws  # noqa: E402

LAYER_TOL = dict(rtol=1e-4, atol=2e-4)  # tests/test_gpu_yolov12.py, tests/test_gpu_obb_model.py: fp32 layers and raw levels
Y_TOL = dict(rtol=1e-4, atol=1e-3)  # tests/test_gpu_yolov12.py: the decoded prediction
TAG, SHAPE, N = ws.MODEL_TAG, ws.MODEL_SHAPE, ws.MODEL_TEXTS


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, TAG + ".npz"))


def _facade(n=N, tag=TAG):
    import edge_yolo_amd
    y = edge_yolo_amd.YOLOWorld("yolov8n-worldv2.yaml")
    y.model.load_state_dict(ws.state_dict(y.model.state_dict()), strict=False)
    y.set_classes(ws.names(n), ws.text(tag, n))
    return y


def _build(dtype):
    m = _facade().model.to("cuda")
    m.fuse()
    return (m.half() if dtype == torch.float16 else m.float()).eval()


def test_fp32_vs_reference_golden(golden):
    g = golden
    m = _build(torch.float32)
    y, raw = m(synth.synth_images(*SHAPE).cuda())
    assert y.dtype == torch.float32 and tuple(y.shape) == g["y"].shape == (2, 4 + N, 126)
    got = y.cpu().numpy()
    print(f"{TAG} y: max abs err {float(np.abs(got - g['y']).max()):.3e}")
    np.testing.assert_allclose(got, g["y"], err_msg="y", **Y_TOL)
    for i, r in enumerate(raw):
        print(f"{TAG} raw{i}: max abs err {float(np.abs(r.float().cpu().numpy() - g[f'raw{i}']).max()):.3e}")
        np.testing.assert_allclose(r.float().cpu().numpy(), g[f"raw{i}"], err_msg=f"raw{i}", **LAYER_TOL)


def test_fp16_vs_reference_golden(golden):
    g = golden
    m = _build(torch.float16)
    y, _ = m(synth.synth_images(*SHAPE).cuda().half())
    y = y.cpu().numpy()
    assert y.dtype == np.float32 and y.shape == g["y"].shape and np.isfinite(y).all()
    print(f"{TAG} f16: scores {float(np.abs(y[:, 4:] - g['y'][:, 4:]).max()):.3e} boxes {float(np.abs(y[:, :4] - g['y'][:, :4]).max()):.3e}")
    assert float(np.abs(y[:, 4:] - g["y"][:, 4:]).max()) < 2e-2
    assert float(np.abs(y[:, :4] - g["y"][:, :4]).max()) < 0.015 * max(SHAPE[1:])


def test_txt_feats_override_equals_the_stored_text(golden):
    m = _build(torch.float32)
    x = synth.synth_images(*SHAPE).cuda()
    y0, _ = m(x)
    y1, _ = m.predict(x, txt_feats=m.txt_feats.clone())
    assert torch.equal(y0, y1)
    y2, _ = m.predict(x, txt_feats=ws.normalized(ws.text("other", N)))
    assert not torch.equal(y0, y2)
    assert torch.equal(m(x)[0], y0)  # the override is gone afterwards
    with pytest.raises(NotImplementedError, match="per-image"):
        m.predict(x, txt_feats=m.txt_feats.repeat(2, 1, 1))


@pytest.mark.parametrize("tag,kw,shape,n", ws.ATTN_CASES + [ws.C2FATTN_CASE], ids=lambda v: v if isinstance(v, str) else None)
def test_modules_fp32_vs_reference_golden(golden_dir, tag, kw, shape, n):
    from edge_yolo_amd.nn import modules as M
    g = np.load(os.path.join(golden_dir, "world_ops.npz"))
    cls = M.C2fAttn if tag == ws.C2FATTN_CASE[0] else M.MaxSigmoidAttnBlock
    m = cls(**kw)
    m.load_state_dict(ws.state_dict(m.state_dict(), prefix=tag + "."))
    m = m.cuda().float().eval()
    (m.attn if cls is M.C2fAttn else m).set_text(ws.normalized(ws.text(tag, n)))
    y = m(ws.case_input(tag, shape).cuda())
    print(f"{tag}: max abs err {float(np.abs(y.cpu().numpy() - g[tag + '_y']).max()):.3e}")
    np.testing.assert_allclose(y.cpu().numpy(), g[tag + "_y"], err_msg=tag, **LAYER_TOL)


def test_head_module_vs_reference_golden(golden_dir):
    from edge_yolo_amd.nn import modules as M
    g = np.load(os.path.join(golden_dir, "world_ops.npz"))
    tag, kw, shapes, n = ws.HEAD_CASE
    M.WorldDetect.legacy = True
    m = M.WorldDetect(**kw)
    m.stride = torch.tensor([8.0, 16.0, 32.0])
    m.load_state_dict(ws.state_dict(m.state_dict(), prefix=tag + "."))
    m = m.cuda().float().eval()
    m.set_text(ws.text(tag, n)[None])
    assert m.nc == n and m.no == n + 64
    y, raw = m([ws.case_input(f"{tag}{i}", s).cuda() for i, s in enumerate(shapes)])
    np.testing.assert_allclose(y.cpu().numpy(), g[tag + "_y"], **Y_TOL)
    for i, r in enumerate(raw):
        np.testing.assert_allclose(r.float().cpu().numpy(), g[f"{tag}_raw{i}"], err_msg=f"raw{i}", **LAYER_TOL)


@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
def test_predict_graph_vocabulary_change_and_back(golden, half):
    g = golden
    conf = float(g["conf"])
    model = _facade()
    assert model.task == "detect" and type(model.model).__name__ == "WorldModel"
    x = synth.synth_images(*SHAPE)
    kw = dict(conf=conf, iou=0.7, half=half, device="cuda:0")
    first = model.predict(x, **kw)
    assert len(first) == 2 and first[0].names == dict(enumerate(ws.names(N)))
    replay = model.predict(x, **kw)
    eager = model.predict(x, graph=False, **kw)
    for a, b, c in zip(first, replay, eager):
        assert torch.equal(a.boxes.data, b.boxes.data) and torch.equal(a.boxes.data, c.boxes.data)
    if not half:
        # fp32: the reference's NMS rows at the project's box / score bar (tests/test_gpu_obb_model.py: the fp32 layer bar on the rows, classes equal)
        for i, r in enumerate(first):
            want = g[f"det{i}"]
            assert tuple(r.boxes.data.shape) == want.shape and len(want) >= 5
            np.testing.assert_array_equal(r.boxes.cls.cpu().numpy(), want[:, 5])
            np.testing.assert_allclose(r.boxes.data.cpu().numpy(), want, rtol=1e-4, atol=1e-3)
    # a second vocabulary of another size, then back: no stale guide, fold or graph survives
    model.set_classes(ws.names(ws.OTHER_TEXTS), ws.text("second", ws.OTHER_TEXTS))
    assert model.predictor is None and model.model.model[-1].nc == ws.OTHER_TEXTS
    other = model.predict(x, **kw)
    assert other[0].names == dict(enumerate(ws.names(ws.OTHER_TEXTS)))
    assert not all(a.boxes.data.shape == b.boxes.data.shape and torch.equal(a.boxes.data, b.boxes.data) for a, b in zip(first, other))
    model.set_classes(ws.names(N), ws.text(TAG, N))
    back = model.predict(x, **kw)
    for a, b in zip(first, back):
        assert torch.equal(a.boxes.data, b.boxes.data)


def test_val_runs_through_the_detection_validator():
    from edge_yolo_amd.engine.validator import DetectionValidator, KEYS
    from edge_yolo_amd.utils import metrics, ops as uops
    model = _facade()
    x = synth.synth_images(*SHAPE)
    res = model.predict(x, conf=0.25, iou=0.7, device="cuda:0")
    h, w = SHAPE[1:]
    cls, box, bi = [], [], []
    for i, r in enumerate(res):  # labels: the three best rows of each image, as normalised xywh
        d = r.boxes.data[:3].cpu()
        xyxy = d[:, :4]
        box.append(torch.stack([(xyxy[:, 0] + xyxy[:, 2]) / 2 / w, (xyxy[:, 1] + xyxy[:, 3]) / 2 / h, (xyxy[:, 2] - xyxy[:, 0]) / w, (xyxy[:, 3] - xyxy[:, 1]) / h], 1))
        cls.append(d[:, 5:6])
        bi.append(torch.full((len(d),), float(i)))
    batch = {"img": x, "cls": torch.cat(cls).numpy(), "bboxes": torch.cat(box).numpy(), "batch_idx": torch.cat(bi).numpy(), "ori_shape": [(h, w)] * SHAPE[0]}
    out = dict(model.val([batch], device="cuda:0"))
    v = model.validator
    assert isinstance(v, DetectionValidator) and set(KEYS) <= set(out) and v.seen == SHAPE[0]
    tp = np.concatenate(v.stats["tp"])
    assert tp.any() and out[KEYS[2]] > 0
    # the same rows, matched by hand
    m = model.model
    rows = uops.non_max_suppression(m(x.cuda())[0], 0.001, 0.7, multi_label=True, max_det=300)
    want = []
    for i, r in enumerate(rows):
        r = r.float().cpu().reshape(-1, 6).clone()
        uops.scale_boxes((h, w), r[:, :4], (h, w))  # (what the validator does with ori_shape == imgsz: a clip to the image)
        r = r.numpy()
        gt = batch["bboxes"][batch["batch_idx"] == i].astype(np.float32)
        gxyxy = uops.scale_boxes((h, w), uops.xywh2xyxy(torch.from_numpy(gt)) * torch.tensor([w, h, w, h], dtype=torch.float32), (h, w))
        want.append(metrics.match_predictions(r[:, 5], batch["cls"][batch["batch_idx"] == i].reshape(-1).astype(np.float32),
                                              metrics.box_iou(gxyxy.numpy(), r[:, :4]), metrics.IOUV))
    np.testing.assert_array_equal(tp, np.concatenate(want))


def test_predict_batches_raises():
    model = _facade()
    with pytest.raises(NotImplementedError, match="vocabulary"):
        next(iter(model.predict_batches([torch.zeros(1, 3, 64, 64)])))
