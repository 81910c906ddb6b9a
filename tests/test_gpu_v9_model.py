"""-m gpu: YOLOv9 (GELAN) end to end.  The modules against the reference's outputs (tests/golden/v9_ops.npz) at the fp32 layer bar of
tests/test_gpu_world_model.py (rtol 1e-4, atol 2e-4); yolov9t (64x96, B = 2: ELAN1, AConv, SPPELAN), yolov9e (64x64, B = 2: nn.Identity, ADown,
CBLinear, CBFuse with up to 6 sources), yolov9c-seg (64x96, B = 1) and yolov9m (64x96, B = 1: hidden widths that are no multiples of 8) with
synthetic weights against the reference's forward at the parity bars of tests/test_gpu_yolov12.py (y: rtol 1e-4, atol 1e-3; raw levels: the layer bar) and the f16 bar of tests/test_gpu_obb_model.py (scores
within 2e-2, boxes within 1.5 % of the image size); YOLO.predict() with and without the captured graph against the reference's NMS rows;
val() for the detect and the segment task; predict_batches; and yolov9e-seg through predict()."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import synthdata as synth  # noqa: E402
import v9_synth as vs  # noqa: E402

LAYER_TOL = dict(rtol=1e-4, atol=2e-4)  # tests/test_gpu_world_model.py: fp32 layers and raw levels
Y_TOL = dict(rtol=1e-4, atol=1e-3)  # tests/test_gpu_yolov12.py: the decoded prediction


@pytest.fixture(scope="module")
def ops_golden(golden_dir):
    return np.load(os.path.join(golden_dir, "v9_ops.npz"))


def _facade(tag):
    import edge_yolo_amd
    name, _, gain = vs.MODEL_CASES[tag]
    y = edge_yolo_amd.YOLO(name)
    y.model.load_state_dict(vs.state_dict(y.model.state_dict(), gain=gain))
    return y


def _build(tag, dtype):
    m = _facade(tag).model.to("cuda")
    m.fuse()
    return (m.half() if dtype == torch.float16 else m.float()).eval()


def _close(name, got, want, tol):
    got = got.float().cpu().numpy()
    print(f"{name}: max abs err {float(np.abs(got - want).max()):.3e}")
    np.testing.assert_allclose(got, want, err_msg=name, **tol)


# ---------------------------------------------------------------------------------------------------------------- modules
@pytest.mark.parametrize("tag,cls,args,kw,shape", vs.MODULE_CASES, ids=[c[0] for c in vs.MODULE_CASES])
def test_modules_fp32_vs_reference_golden(ops_golden, tag, cls, args, kw, shape):
    from edge_yolo_amd.nn import modules as M
    m = getattr(M, cls)(*args, **kw)
    m.load_state_dict(vs.state_dict(m.state_dict(), prefix=tag + "."))
    m = m.cuda().float().eval()
    x = vs.case_input(tag, shape).cuda()
    _close(tag, m(x), ops_golden[tag + "_y"], LAYER_TOL)
    if cls == "RepConv":  # before and after fuse_convs: the same single 3x3 conv
        m.fuse_convs()
        assert list(m.state_dict()) == ["conv.weight", "conv.bias"]
        _close(tag + " fused", m(x), ops_golden[tag + "_y"], LAYER_TOL)
        _close(tag + " fused vs fused", m(x), ops_golden[tag + "_fused_y"], LAYER_TOL)


def test_cblinear_and_cbfuse_vs_reference_golden(ops_golden):
    from edge_yolo_amd import _lib as L
    from edge_yolo_amd.nn import modules as M
    tag, args, shape = vs.CBLINEAR_CASE
    m = M.CBLinear(*args)
    m.load_state_dict(vs.state_dict(m.state_dict(), prefix=tag + "."))
    ys = m.cuda().float().eval()(vs.case_input(tag, shape).cuda())
    assert isinstance(ys, tuple) and [y.shape[1] for y in ys] == args[1]
    assert len({L.cstride(y) for y in ys}) == 1 and L.cstride(ys[0]) == sum(args[1])  # views of one output
    for i, y in enumerate(ys):
        _close(f"{tag} {i}", y, ops_golden[f"{tag}_y{i}"], LAYER_TOL)
    tag, idx, _, _ = vs.CBFUSE_CASE
    xs = [tuple(t.cuda() for t in x) if isinstance(x, tuple) else x.cuda() for x in vs.cbfuse_inputs()]
    _close(tag, M.CBFuse(idx)(xs), ops_golden[tag + "_y"], LAYER_TOL)


# ---------------------------------------------------------------------------------------------------------------- whole models
@pytest.mark.parametrize("tag", list(vs.MODEL_CASES))
def test_fp32_vs_reference_golden(golden_dir, tag):
    g = np.load(os.path.join(golden_dir, tag + ".npz"))
    name, shape, _ = vs.MODEL_CASES[tag]
    m = _build(tag, torch.float32)
    y, rest = m(synth.synth_images(*shape).cuda())
    seg = vs.TASK[name] == "segment"
    raw, mc, p = rest if seg else (rest, None, None)
    assert y.dtype == torch.float32 and tuple(y.shape) == g["y"].shape
    _close(f"{tag} y", y, g["y"], Y_TOL)
    for i, r in enumerate(raw):
        _close(f"{tag} raw{i}", r, g[f"raw{i}"], LAYER_TOL)
    if seg:
        _close(f"{tag} mc", mc, g["mc"], LAYER_TOL)
        _close(f"{tag} p", p, g["p"], LAYER_TOL)


@pytest.mark.parametrize("tag", ["yolov9t_64x96", "yolov9e_64"])
def test_fp16_vs_reference_golden(golden_dir, tag):
    g = np.load(os.path.join(golden_dir, tag + ".npz"))
    _, shape, _ = vs.MODEL_CASES[tag]
    m = _build(tag, torch.float16)
    y, _ = m(synth.synth_images(*shape).cuda().half())
    y = y.cpu().numpy()
    assert y.dtype == np.float32 and y.shape == g["y"].shape and np.isfinite(y).all()
    print(f"{tag} f16: scores {float(np.abs(y[:, 4:] - g['y'][:, 4:]).max()):.3e} boxes {float(np.abs(y[:, :4] - g['y'][:, :4]).max()):.3e}")
    assert float(np.abs(y[:, 4:] - g["y"][:, 4:]).max()) < 2e-2
    assert float(np.abs(y[:, :4] - g["y"][:, :4]).max()) < 0.015 * max(shape[1:])


# ---------------------------------------------------------------------------------------------------------------- the facade
@pytest.mark.parametrize("tag", ["yolov9t_64x96", "yolov9e_64", "yolov9m_64x96"])
def test_predict_with_and_without_graph(golden_dir, tag):
    g = np.load(os.path.join(golden_dir, tag + ".npz"))
    _, shape, _ = vs.MODEL_CASES[tag]
    model = _facade(tag)
    assert model.task == "detect"
    x = synth.synth_images(*shape)
    kw = dict(conf=float(g["conf"]), iou=0.7, device="cuda:0")
    first = model.predict(x, **kw)
    replay = model.predict(x, **kw)
    eager = model.predict(x, graph=False, **kw)
    assert len(first) == shape[0]
    for i, (a, b, c) in enumerate(zip(first, replay, eager)):
        assert torch.equal(a.boxes.data, b.boxes.data) and torch.equal(a.boxes.data, c.boxes.data)
        want = g[f"det{i}"]  # the reference's NMS rows at the bars of tests/test_gpu_world_model.py
        assert tuple(a.boxes.data.shape) == want.shape and len(want) >= 5
        np.testing.assert_array_equal(a.boxes.cls.cpu().numpy(), want[:, 5])
        np.testing.assert_allclose(a.boxes.data.cpu().numpy(), want, rtol=1e-4, atol=1e-3)
    half = model.predict(x, half=True, **kw)
    assert len(half) == shape[0] and all(bool(torch.isfinite(r.boxes.data).all()) for r in half)


def test_segment_predict_returns_masks(golden_dir):
    tag = "yolov9c_seg_64x96"
    g = np.load(os.path.join(golden_dir, tag + ".npz"))
    _, shape, _ = vs.MODEL_CASES[tag]
    model = _facade(tag)
    assert model.task == "segment"
    x = synth.synth_images(*shape)
    res = model.predict(x, conf=float(g["conf"]), iou=0.7, device="cuda:0")
    eager = model.predict(x, conf=float(g["conf"]), iou=0.7, device="cuda:0", graph=False)
    want = g["det0"]
    assert len(res) == 1 and len(res[0]) == len(want) >= 5
    assert torch.equal(res[0].boxes.data, eager[0].boxes.data) and torch.equal(res[0].masks.data, eager[0].masks.data)
    np.testing.assert_array_equal(res[0].boxes.cls.cpu().numpy(), want[:, 5])
    np.testing.assert_allclose(res[0].boxes.data.cpu().numpy(), want[:, :6], rtol=1e-4, atol=1e-3)
    assert res[0].masks.data.dtype == torch.bool and tuple(res[0].masks.data.shape) == g["masks0"].shape and bool(res[0].masks.data.any())


def test_val_returns_finite_metrics():
    from edge_yolo_amd.engine.validator import DetectionValidator, KEYS
    tag = "yolov9t_64x96"
    _, shape, _ = vs.MODEL_CASES[tag]
    model = _facade(tag)
    x = synth.synth_images(*shape)
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


def test_predict_batches_equals_predict():
    tag = "yolov9t_64x96"
    _, shape, _ = vs.MODEL_CASES[tag]
    model = _facade(tag)
    xs = [synth.synth_images(*shape, seed=s) for s in range(3)]
    kw = dict(conf=0.05, iou=0.7, device="cuda:0")
    want = [model.predict(x, **kw) for x in xs]
    got = list(_facade(tag).predict_batches(xs, **kw))
    assert len(got) == 3
    for a, b in zip(want, got):
        for ra, rb in zip(a, b):
            assert torch.equal(ra.boxes.data, rb.boxes.data) and len(ra) >= 1
    with pytest.raises(NotImplementedError, match="nn.Identity"):
        next(iter(_facade("yolov9e_64").predict_batches([xs[0][:, :, :64, :64]], **kw)))


def test_segment_val_returns_finite_metrics(golden_dir):
    """YOLO("yolov9c-seg.yaml").val() on the images and labels of tests/golden/segval_case.npz (the fixture of tests/test_gpu_segval_model.py)."""
    from test_segval_cpu import KEYS10, segval_batch
    g = np.load(os.path.join(golden_dir, "segval_case.npz"))
    batch = segval_batch(g, True)
    batch["img"] = synth.synth_images(len(g["ori_shape"]), 128, 160, seed=9)
    model = _facade("yolov9c_seg_64x96")
    out = dict(model.val([batch], overlap_mask=True, device="cuda:0"))
    assert type(model.validator).__name__ == "SegmentationValidator" and model.validator.seen == len(g["ori_shape"])
    assert set(KEYS10) <= set(out) and all(np.isfinite(float(out[k])) for k in KEYS10)


def test_yolov9e_seg_predict_graph_equals_eager():
    import edge_yolo_amd
    model = edge_yolo_amd.YOLO("yolov9e-seg.yaml")
    assert model.task == "segment"
    model.model.load_state_dict(vs.state_dict(model.model.state_dict(), gain=vs.MODEL_CASES["yolov9e_64"][2]))
    x = synth.synth_images(1, 64, 64)
    res = model.predict(x, conf=0.05, iou=0.7, device="cuda:0")
    eager = model.predict(x, conf=0.05, iou=0.7, device="cuda:0", graph=False)
    assert len(res) == 1 and len(res[0]) >= 1 and bool(torch.isfinite(res[0].boxes.data).all())
    assert torch.equal(res[0].boxes.data, eager[0].boxes.data) and torch.equal(res[0].masks.data, eager[0].masks.data)
