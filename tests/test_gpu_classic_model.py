"""-m gpu: YOLOv3, YOLOv5 and YOLOv6 end to end.  The modules against the reference's outputs (tests/golden/classic_ops.npz) at the fp32 layer
bar of tests/test_gpu_ghost_model.py (rtol 1e-4, atol 2e-4); yolov5n (64x96, B = 2), yolov5n-p6 (64x128: four levels, a 1x2 map at stride 64),
yolov3-tiny (64x96, B = 2: two levels), yolov3 and yolov3-spp at a quarter of the width (64x96) and yolov6n (64x96, ReLU) with synthetic
weights against the reference's forward at that file's parity bars (y: rtol 1e-4, atol 1e-3; raw levels: the layer bar) and its f16 bar
(scores within 2e-2, boxes within 1.5 % of the image size); YOLO.predict() with and without the captured graph against the reference's NMS
rows; predict(half=True) and predict(augment=True); val(); predict_batches; and one traced batch-2 640x640 f16 forward per family: no
conv_direct launch, no layout copy in front of layer 0, and for yolov3-tiny exactly six max-pool launches and no padded copy."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import synthdata as synth  # noqa: E402
import classic_synth as cs  # noqa: E402
from gpu_util import _traced  # noqa: E402

LAYER_TOL = dict(rtol=1e-4, atol=2e-4)  # tests/test_gpu_ghost_model.py: fp32 layers and raw levels
Y_TOL = dict(rtol=1e-4, atol=1e-3)  # tests/test_gpu_ghost_model.py: the decoded prediction


@pytest.fixture(scope="module")
def ops_golden(golden_dir):
    return np.load(os.path.join(golden_dir, "classic_ops.npz"))


def _cfg(tag):
    from edge_yolo_amd.nn.tasks import yaml_model_load
    return cs.model_cfg(tag, yaml_model_load)


def _facade(tag):
    import edge_yolo_amd
    y = edge_yolo_amd.YOLO(_cfg(tag))
    y.model.load_state_dict(cs.model_weights(tag, y.model.state_dict()))
    return y


def _build(tag, dtype):
    m = _facade(tag).model.to("cuda")
    m.fuse()
    return (m.half() if dtype == torch.float16 else m.float()).eval()


def _close(name, got, want, tol):
    got = got.float().cpu().numpy()
    print(f"{name}: max abs err {float(np.abs(got - want).max()):.3e}")
    np.testing.assert_allclose(got, want, err_msg=name, **tol)


def _own_ns():
    from edge_yolo_amd.nn import modules as M
    from edge_yolo_amd.nn.tasks import parse_model
    return {"Conv": M.Conv, "SPP": M.SPP, "MaxPool2d": M.MaxPool2d, "ZeroPad2d": M.ZeroPad2d, "ConvTranspose2d": M.ConvTranspose2d, "parse": parse_model}


# ---------------------------------------------------------------------------------------------------------------- modules
@pytest.mark.parametrize("tag", list(cs.OPS_CASES))
def test_modules_fp32_vs_reference_golden(ops_golden, tag):
    m = cs.prepare(cs.make_module(tag, _own_ns()), tag).cuda().float()
    x = cs.ops_input(tag).cuda()
    y, labels = _traced(lambda: m(x))
    print(tag, labels)
    assert "conv_direct_kernel" not in labels
    if tag in ("stem6", "stem3s1"):
        assert labels == [tag + "_kernel"]  # fp32: the VALU form, straight from the planar image
    if tag in ("zeropad_maxpool", "maxpool_s2"):  # a maximum: exact (stand-alone the pad is a copy of its own)
        assert torch.equal(y.cpu(), torch.from_numpy(ops_golden[tag + "_y"]))
    _close(tag, y, ops_golden[tag + "_y"], LAYER_TOL)


# ---------------------------------------------------------------------------------------------------------------- whole models
@pytest.mark.parametrize("tag", list(cs.MODEL_CASES))
def test_fp32_vs_reference_golden(golden_dir, tag):
    g = np.load(os.path.join(golden_dir, tag + ".npz"))
    m = _build(tag, torch.float32)
    y, raw = m(cs.model_images(tag).cuda())
    assert y.dtype == torch.float32 and tuple(y.shape) == g["y"].shape
    assert len(raw) == len(m.stride) == cs.NL[tag] == sum(f"raw{i}" in g for i in range(5))  # two, three or four pyramid levels
    _close(f"{tag} y", y, g["y"], Y_TOL)
    for i, r in enumerate(raw):
        _close(f"{tag} raw{i}", r, g[f"raw{i}"], LAYER_TOL)


@pytest.mark.parametrize("tag", list(cs.MODEL_CASES))
def test_fp16_vs_reference_golden(golden_dir, tag):
    g = np.load(os.path.join(golden_dir, tag + ".npz"))
    shape = cs.MODEL_CASES[tag][1]
    m = _build(tag, torch.float16)
    y, _ = m(cs.model_images(tag).cuda().half())
    y = y.cpu().numpy()
    assert y.dtype == np.float32 and y.shape == g["y"].shape and np.isfinite(y).all()
    print(f"{tag} f16: scores {float(np.abs(y[:, 4:] - g['y'][:, 4:]).max()):.3e} boxes {float(np.abs(y[:, :4] - g['y'][:, :4]).max()):.3e}")
    assert float(np.abs(y[:, 4:] - g["y"][:, 4:]).max()) < 2e-2
    assert float(np.abs(y[:, :4] - g["y"][:, :4]).max()) < 0.015 * max(shape[1:])


# ---------------------------------------------------------------------------------------------------------------- the facade
@pytest.mark.parametrize("tag", list(cs.MODEL_CASES))
def test_predict_with_and_without_graph(golden_dir, tag):
    g = np.load(os.path.join(golden_dir, tag + ".npz"))
    shape = cs.MODEL_CASES[tag][1]
    model = _facade(tag)
    assert model.task == "detect"
    x = cs.model_images(tag)
    kw = dict(conf=float(g["conf"]), iou=0.7, device="cuda:0")
    first = model.predict(x, **kw)
    replay = model.predict(x, **kw)
    eager = model.predict(x, graph=False, **kw)
    assert len(first) == shape[0]
    for i, (a, b, c) in enumerate(zip(first, replay, eager)):
        assert torch.equal(a.boxes.data, b.boxes.data) and torch.equal(a.boxes.data, c.boxes.data)
        want = g[f"det{i}"]  # the reference's NMS rows: exact classes and order
        assert tuple(a.boxes.data.shape) == want.shape and len(want) >= 5
        np.testing.assert_array_equal(a.boxes.cls.cpu().numpy(), want[:, 5])
        np.testing.assert_allclose(a.boxes.data.cpu().numpy(), want, rtol=1e-4, atol=1e-3)
    half = model.predict(x, half=True, **kw)
    assert len(half) == shape[0] and all(bool(torch.isfinite(r.boxes.data).all()) for r in half)
    aug = model.predict(x, augment=True, **kw)
    assert len(aug) == shape[0] and all(bool(torch.isfinite(r.boxes.data).all()) and len(r) >= 1 for r in aug)


@pytest.mark.parametrize("tag", ["yolov5n_64x96", "yolov3-tiny_64x96"])
def test_val_returns_finite_metrics(tag):
    from edge_yolo_amd.engine.validator import DetectionValidator, KEYS
    shape = cs.MODEL_CASES[tag][1]
    model = _facade(tag)
    x = cs.model_images(tag)
    res = model.predict(x, conf=0.05, iou=0.7, device="cuda:0")
    h, w = shape[1:]
    cls, box, bi = [], [], []
    for i, r in enumerate(res):  # labels: the three best rows of each image, as normalised xywh
        d = r.boxes.data[:3].cpu()
        xyxy = d[:, :4]
        box.append(torch.stack([(xyxy[:, 0] + xyxy[:, 2]) / 2 / w, (xyxy[:, 1] + xyxy[:, 3]) / 2 / h, (xyxy[:, 2] - xyxy[:, 0]) / w, (xyxy[:, 3] - xyxy[:, 1]) / h], 1))
        cls.append(d[:, 5:6])
        bi.append(torch.full((len(d),), float(i)))
    batch = {"img": x, "cls": torch.cat(cls).numpy(), "bboxes": torch.cat(box).numpy(), "batch_idx": torch.cat(bi).numpy(), "ori_shape": [(h, w)] * shape[0]}
    out = dict(model.val([batch], device="cuda:0"))
    v = model.validator
    assert isinstance(v, DetectionValidator) and set(KEYS) <= set(out) and v.seen == shape[0]
    assert all(np.isfinite(float(out[k])) for k in KEYS) and out[KEYS[2]] > 0


@pytest.mark.parametrize("tag", ["yolov5n_64x96", "yolov3-tiny_64x96", "yolov6n_64x96"])
def test_predict_batches_equals_predict(tag):
    shape = cs.MODEL_CASES[tag][1]
    model = _facade(tag)
    xs = [synth.synth_images(*shape, seed=s) for s in range(3)]
    kw = dict(conf=0.05, iou=0.7, device="cuda:0")
    want = [model.predict(x, **kw) for x in xs]
    got = list(_facade(tag).predict_batches(xs, **kw))
    assert len(got) == 3
    for a, b in zip(want, got):
        for ra, rb in zip(a, b):
            assert torch.equal(ra.boxes.data, rb.boxes.data) and len(ra) >= 1


# ---------------------------------------------------------------------------------------------------------------- the launches of a 640x640 forward
@pytest.mark.parametrize("tag,stem", [("yolov5n_64x96", "stem6_mfma_kernel"), ("yolov3-tiny_64x96", "stem3s1_mfma_kernel"), ("yolov6n_64x96", None)])
def test_traced_640_f16_forward_runs_on_the_built_kernels(tag, stem):
    m = _build(tag, torch.float16)
    x = synth.synth_images(2, 640, 640, seed=9).cuda().half()
    (y, _), labels = _traced(lambda: m(x))
    assert bool(torch.isfinite(y).all())
    print(tag, len(labels), sorted(set(labels)))
    assert "conv_direct_kernel" not in labels
    # the first launch is a stem kernel: those read the planar NCHW image themselves (no NCHW -> NHWC copy in front of layer 0)
    if stem is not None:
        assert labels[0] == stem and labels.count(stem) == 1
    else:  # yolov6: layers 0 + 1 are 3x3 stride-2 convs: the existing stem kernels
        assert labels[0].startswith("stem")
    if tag.startswith("yolov3-tiny"):
        assert labels.count("maxpool_kernel") == 6 and "zeropad_kernel" not in labels
    if tag.startswith("yolov6"):
        assert labels.count("deconv2x2_kernel") == 2
