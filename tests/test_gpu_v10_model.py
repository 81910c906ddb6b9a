"""-m gpu: YOLOv10 end to end.  The modules against the reference's outputs (tests/golden/v10_ops.npz) at the fp32 layer bar of
tests/test_gpu_v9_model.py (rtol 1e-4, atol 2e-4), RepVGGDW before and after fuse(); yolov10n (64x96, B = 2: SCDown x3, the 2-head PSA, C2fCIB
with the 7x7 branch) and yolov10x (64x64, B = 1: C2fCIB in the backbone, the 5-head PSA, the 320 / 640 widths) with synthetic weights against
the reference's forward: the raw maps of both branches at rtol 1e-4, atol 3e-4 and the end2end rows at the bars of
test_e2e_detect_vs_reference_golden (scores rtol 1e-4, atol 1e-5, sorted descending; boxes rtol 1e-4, atol 1e-3) -- with exact classes and
exact row order on the rows the generator found separated by more than 1e-3; the f16 mode (scores within 2e-2); YOLO.predict() with and
without the captured graph against the reference's filtered rows; max_det and classes=; val(); predict_batches."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import v10_synth as vs  # noqa: E402

LAYER_TOL = dict(rtol=1e-4, atol=2e-4)
RAW_TOL = dict(rtol=1e-4, atol=3e-4)


@pytest.fixture(scope="module")
def ops_golden(golden_dir):
    return np.load(os.path.join(golden_dir, "v10_ops.npz"))


def _facade(tag):
    import edge_yolo_amd
    y = edge_yolo_amd.YOLO(vs.MODEL_CASES[tag][0])
    y.model.load_state_dict(vs.model_weights(tag, y.model.state_dict()))
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
    for mod in m.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.eps = 1e-3
    m.load_state_dict(vs.state_dict(m.state_dict(), prefix=tag + "."))
    m = m.cuda().float().eval()
    x = vs.case_input(tag, shape).cuda()
    _close(tag, m(x), ops_golden[tag + "_y"], LAYER_TOL)
    if cls == "RepVGGDW":  # before and after fuse(): the same single depthwise 7x7
        m.fuse()
        assert list(m.state_dict()) == ["conv.weight", "conv.bias"]
        _close(tag + " fused", m(x), ops_golden[tag + "_y"], LAYER_TOL)
        _close(tag + " fused vs fused", m(x), ops_golden[tag + "_fused_y"], LAYER_TOL)


# ---------------------------------------------------------------------------------------------------------------- whole models
def _check_rows(tag, y, g):
    """y (B, k, 6) against the golden rows: scores everywhere; class, order and boxes on the rows the generator found separated."""
    conf = float(g["conf"])
    np.testing.assert_allclose(y[..., 4], g["y"][..., 4], rtol=1e-4, atol=1e-5)
    assert (np.diff(y[..., 4], axis=1) <= 0).all()
    for i in range(y.shape[0]):
        n, gap = vs.separated_rows(g["y"][i, :, 4], conf)
        assert n >= vs.MIN_ROWS and gap > vs.ROW_GAP
        np.testing.assert_array_equal(y[i, :n + 1, 5], g["y"][i, :n + 1, 5])  # exact classes in exact order, no share of mismatches
        np.testing.assert_allclose(y[i, :n + 1, :4], g["y"][i, :n + 1, :4], rtol=1e-4, atol=1e-3)
    same = y[..., 5] == g["y"][..., 5]
    print(f"{tag}: rows with the reference's class at the reference's rank: {float(same.mean()):.4f}")
    np.testing.assert_allclose(y[..., :4][same], g["y"][..., :4][same], rtol=1e-4, atol=1e-3)


@pytest.mark.parametrize("tag", list(vs.MODEL_CASES))
def test_fp32_vs_reference_golden(golden_dir, tag):
    g = np.load(os.path.join(golden_dir, tag + ".npz"))
    m = _build(tag, torch.float32)
    assert m.end2end
    m.model[-1].one2many_in_inference = True
    y, aux = m(vs.model_images(tag).cuda())
    assert y.dtype == torch.float32 and tuple(y.shape) == g["y"].shape
    for br in ("one2one", "one2many"):
        assert len(aux[br]) == 3
        for i, r in enumerate(aux[br]):
            _close(f"{tag} {br}{i}", r, g[f"{br}{i}"], RAW_TOL)
    _check_rows(tag, y.cpu().numpy(), g)


@pytest.mark.parametrize("tag", list(vs.MODEL_CASES))
def test_fp16_vs_reference_golden(golden_dir, tag):
    g = np.load(os.path.join(golden_dir, tag + ".npz"))
    m = _build(tag, torch.float16)
    y, aux = m(vs.model_images(tag).cuda().half())
    assert aux["one2many"] is None
    y = y.cpu().numpy()
    assert y.dtype == np.float32 and y.shape == g["y"].shape and np.isfinite(y).all()
    print(f"{tag} f16: scores {float(np.abs(y[..., 4] - g['y'][..., 4]).max()):.3e}")
    assert float(np.abs(y[..., 4] - g["y"][..., 4]).max()) < 2e-2


# ---------------------------------------------------------------------------------------------------------------- the facade
@pytest.mark.parametrize("tag", list(vs.MODEL_CASES))
def test_predict_with_and_without_graph(golden_dir, tag):
    g = np.load(os.path.join(golden_dir, tag + ".npz"))
    shape = vs.MODEL_CASES[tag][1]
    model = _facade(tag)
    assert model.task == "detect"
    x = vs.model_images(tag)
    kw = dict(conf=float(g["conf"]), iou=0.7, device="cuda:0")
    first = model.predict(x, **kw)
    replay = model.predict(x, **kw)
    eager = model.predict(x, graph=False, **kw)
    assert type(model.predictor).__name__ == "DetectionPredictor" and len(first) == shape[0]
    for i, (a, b, c) in enumerate(zip(first, replay, eager)):
        assert torch.equal(a.boxes.data, b.boxes.data) and torch.equal(a.boxes.data, c.boxes.data)
        want = g[f"det{i}"]  # the reference's filtered rows (no NMS stage: utils/ops.py:224-228)
        assert tuple(a.boxes.data.shape) == want.shape and len(want) >= vs.MIN_ROWS
        np.testing.assert_array_equal(a.boxes.cls.cpu().numpy(), want[:, 5])
        np.testing.assert_allclose(a.boxes.data.cpu().numpy(), want, rtol=1e-4, atol=1e-3)
    half = model.predict(x, half=True, **kw)
    assert len(half) == shape[0] and all(bool(torch.isfinite(r.boxes.data).all()) for r in half)


def test_predict_max_det_and_classes_filter(golden_dir):
    """max_det and classes= act as the end2end filter does (`pred[pred[:, 4] > conf][:max_det]`, then the class filter)."""
    tag = "yolov10n_64x96"
    g = np.load(os.path.join(golden_dir, tag + ".npz"))
    model = _facade(tag)
    x = vs.model_images(tag)
    cl = [int(c) for c in g["detc_classes"]]
    res = model.predict(x, conf=float(g["conf"]), iou=0.7, device="cuda:0", max_det=3, classes=cl)
    for i, r in enumerate(res):
        want = g[f"detc{i}"]
        assert len(r) == len(want) <= 3
        np.testing.assert_array_equal(r.boxes.cls.cpu().numpy(), want[:, 5])
        np.testing.assert_allclose(r.boxes.conf.cpu().numpy(), want[:, 4], rtol=1e-4, atol=1e-5)
    assert len(res[0]) >= 1 and all(int(c) in cl for r in res for c in r.boxes.cls.tolist())
    top2 = model.predict(x, conf=float(g["conf"]), iou=0.7, device="cuda:0", max_det=2)
    for i, r in enumerate(top2):
        assert len(r) == 2
        np.testing.assert_allclose(r.boxes.conf.cpu().numpy(), g["y"][i, :2, 4], rtol=1e-4, atol=1e-5)


def test_val_returns_finite_metrics():
    from edge_yolo_amd.engine.validator import DetectionValidator, KEYS
    tag = "yolov10n_64x96"
    shape = vs.MODEL_CASES[tag][1]
    model = _facade(tag)
    x = vs.model_images(tag)
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
    assert all(np.isfinite(float(out[k])) for k in KEYS)


def test_predict_batches_equals_predict():
    import synthdata as synth
    tag = "yolov10n_64x96"
    shape = vs.MODEL_CASES[tag][1]
    model = _facade(tag)
    xs = [synth.synth_images(*shape, seed=s) for s in range(3)]
    kw = dict(conf=0.8, iou=0.7, device="cuda:0")
    want = [model.predict(x, **kw) for x in xs]
    got = list(_facade(tag).predict_batches(xs, **kw))
    assert len(got) == 3
    for a, b in zip(want, got):
        for ra, rb in zip(a, b):
            assert torch.equal(ra.boxes.data, rb.boxes.data) and len(ra) >= 1
