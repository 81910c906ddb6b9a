"""-m gpu: the YOLOv8 task models end to end (synthetic weights, tests/resnet_synth.py) against the reference's CPU fp32 forward
(tests/golden/yolov8n_*.npz): yolov8n-cls, -seg, -pose and -obb at 64x64, yolov8n-seg-p6 and -pose-p6 (four levels) at 128x128.

* fp32: every head output (the decoded prediction, the raw level maps, mask coefficients and prototypes / keypoint logits / angles) at the
  fp32 layer bar of the yolo11 tests of the same task (rtol 1e-4, atol 2e-4).
* f16: the f16 rule of those tests -- scores within 2e-2, boxes within 1.5 % of the image size.
* YOLO(...).predict() through the task's own predictor: in fp32 the kept rows are the reference's NMS rows on its own output (as many rows,
  the same classes in the same order, confidences at the layer bar, box corners within one pixel: the predictor rounds them, and a
  coordinate 1e-4 from a half may round the other way); graph replay and the eager route give the same bits in fp32 and f16."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import resnet_synth as rs  # noqa: E402
import synthdata as synth  # noqa: E402

LAYER_TOL = dict(rtol=1e-4, atol=2e-4)  # tests/test_gpu_seg_model.py, test_gpu_pose_model.py, test_gpu_obb_model.py, test_gpu_cls_model.py
DET = [n for n in rs.V8_MODELS if rs.task_of(n) != "classify"]


def _model_class(task):
    from edge_yolo_amd.nn import tasks as T
    return {"classify": T.ClassificationModel, "segment": T.SegmentationModel, "pose": T.PoseModel, "obb": T.OBBModel}[task]


def _build(name, dtype):
    task = rs.task_of(name)
    m = _model_class(task)(name, nc=rs.RESNET_NC) if task == "classify" else _model_class(task)(name)
    m.load_state_dict(rs.state_dict(m.state_dict()))
    m = m.to("cuda")
    m.fuse()
    return (m.half() if dtype == torch.float16 else m.float()).eval()


def _golden(golden_dir, name):
    return np.load(os.path.join(golden_dir, rs.V8_MODELS[name][0] + ".npz"))


def _aux(task, aux):
    """(golden key, tensor) of the head's auxiliary outputs behind the raw level maps."""
    if task == "segment":
        return (("mc", aux[1]), ("p", aux[2]))
    return (("kpt" if task == "pose" else "angle", aux[1]),)


@pytest.mark.parametrize("name", DET)
def test_fp32_head_outputs_vs_reference(golden_dir, name):
    g, task = _golden(golden_dir, name), rs.task_of(name)
    m = _build(name, torch.float32)
    assert [float(s) for s in m.stride] == g["stride"].tolist()
    y, aux = m(synth.synth_images(*rs.V8_MODELS[name][1]).cuda())
    got = y.float().cpu().numpy()
    assert got.shape == g["y"].shape
    print(f"{name} y {got.shape}: max abs err {float(np.abs(got - g['y']).max()):.3e}")
    np.testing.assert_allclose(got, g["y"], err_msg="y", **LAYER_TOL)
    assert len(aux[0]) == len(m.stride)
    for i, r in enumerate(aux[0]):
        np.testing.assert_allclose(r.float().cpu().numpy(), g[f"raw{i}"], err_msg=f"raw{i}", **LAYER_TOL)
    for key, t in _aux(task, aux):
        np.testing.assert_allclose(t.float().cpu().numpy(), g[key], err_msg=key, **LAYER_TOL)


def test_fp32_cls_vs_reference(golden_dir):
    name = "yolov8n-cls.yaml"
    g = _golden(golden_dir, name)
    m = _build(name, torch.float32)
    probs, logits = m(synth.synth_images(*rs.V8_MODELS[name][1]).cuda())
    np.testing.assert_allclose(logits.cpu().numpy(), g["logits"], err_msg="logits", **LAYER_TOL)
    np.testing.assert_allclose(probs.cpu().numpy(), g["probs"], err_msg="probs", **LAYER_TOL)
    np.testing.assert_array_equal(m.model[-1].top5[0].cpu().numpy(), g["top5"])


@pytest.mark.parametrize("name", DET)
def test_fp16_within_the_f16_bar(golden_dir, name):
    g = _golden(golden_dir, name)
    nc, shape = int(g["nc"]), rs.V8_MODELS[name][1]
    m = _build(name, torch.float16)
    y, _ = m(synth.synth_images(*shape).cuda().half())
    y = y.cpu().numpy()
    assert y.dtype == np.float32 and y.shape == g["y"].shape and np.isfinite(y).all()
    assert float(np.abs(y[:, 4:4 + nc] - g["y"][:, 4:4 + nc]).max()) < 2e-2
    assert float(np.abs(y[:, :4] - g["y"][:, :4]).max()) < 0.015 * max(shape[1:])


@pytest.mark.parametrize("name", list(rs.V8_MODELS))
def test_predict_through_the_task_predictor(golden_dir, name):
    import edge_yolo_amd
    g, task = _golden(golden_dir, name), rs.task_of(name)
    shape = rs.V8_MODELS[name][1]
    model = edge_yolo_amd.YOLO(name, nc=rs.RESNET_NC) if task == "classify" else edge_yolo_amd.YOLO(name)
    assert model.task == task
    model.model.load_state_dict(rs.state_dict(model.model.state_dict()))
    x = synth.synth_images(*shape)
    kw = dict() if task == "classify" else dict(conf=float(g["conf"]), iou=0.7, device="cuda:0")
    data = (lambda r: r.probs.data) if task == "classify" else (lambda r: r.obb.data) if task == "obb" else (lambda r: r.boxes.data)
    for half in (False, True):
        res = model.predict(x.cuda() if task == "classify" else x, half=half, **kw)
        again = model.predict(x.cuda() if task == "classify" else x, half=half, **kw)  # graph replay
        eager = model.predict(x.cuda() if task == "classify" else x, half=half, graph=False, **kw)
        assert len(res) == shape[0]
        for a, b, c in zip(res, again, eager):
            assert torch.equal(data(a), data(b)) and torch.equal(data(a), data(c))
            if task == "segment" and len(a):
                assert torch.equal(a.masks.data, c.masks.data) and tuple(a.masks.shape) == (len(a),) + tuple(shape[1:])
            if task == "pose":
                assert torch.equal(a.keypoints.data, c.keypoints.data) and tuple(a.keypoints.data.shape) == (len(a), 17, 3)
        if half:
            continue
        for i, r in enumerate(res):
            if task == "classify":
                assert r.probs.top5 == g["top5"][i].tolist()
                np.testing.assert_allclose(r.probs.data.cpu().numpy(), g["probs"][i], **LAYER_TOL)
                continue
            want, rows = g[f"det{i}"], data(r).cpu().numpy()
            print(f"{name} image {i}: kept {len(rows)} reference {len(want)}")
            assert len(rows) == len(want) >= 3
            if task == "obb":  # rows (x, y, w, h, angle, conf, cls) after regularize_rboxes; the reference's NMS rows are (x, y, w, h, conf, cls, angle)
                np.testing.assert_array_equal(rows[:, 6], want[:, 5])
                np.testing.assert_allclose(rows[:, 5], want[:, 4], **LAYER_TOL)
                continue
            np.testing.assert_array_equal(rows[:, 5], want[:, 5])
            np.testing.assert_allclose(rows[:, 4], want[:, 4], **LAYER_TOL)
            H, W = shape[1:]
            ref = np.round(np.clip(want[:, :4], 0, [W, H, W, H]))
            assert float(np.abs(rows[:, :4] - ref).max()) <= 1.0
