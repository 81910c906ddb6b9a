"""-m gpu: the obb task end to end.  yolo11n-obb (64x96, synthetic weights) against the reference's forward (tests/golden, the parity bars
of tests/test_gpu_seg_model.py for the head output; the angle row under the rule of tests/test_gpu_obb_exact.py), rotated NMS on the golden's
own prediction, YOLO(...).predict() against the reference's final rows, the refusals, and an OBB row on the EdgeLine backbone."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import fp64_obb_ref as f64  # noqa: E402
import obb_synth  # noqa: E402
import synthdata as synth  # noqa: E402

LAYER_TOL = dict(rtol=1e-4, atol=2e-4)  # tests/test_gpu_seg_model.py, fp32 layers
TAG, SHAPE = "yolo11n_obb_64x96", (1, 64, 96)


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, TAG + ".npz"))


def _build(cfg, dtype):
    from edge_yolo_amd.nn.tasks import OBBModel
    m = OBBModel(cfg)
    m.load_state_dict(obb_synth.state_dict(m.state_dict()))
    m = m.to("cuda")
    m.fuse()
    return (m.half() if dtype == torch.float16 else m.float()).eval()


def test_fp32_vs_reference_golden(golden):
    g = golden
    m = _build("yolo11n-obb.yaml", torch.float32)
    y, (raw, angle) = m(synth.synth_images(*SHAPE).cuda())
    assert y.dtype == torch.float32 and tuple(y.shape) == g["y"].shape == (1, 85, 126) and tuple(angle.shape) == g["angle"].shape == (1, 1, 126)
    got = y.cpu().numpy()
    print(f"{TAG} y: max abs err {float(np.abs(got - g['y']).max()):.3e}")
    np.testing.assert_allclose(got, g["y"], err_msg="y", **LAYER_TOL)
    np.testing.assert_array_equal(angle.cpu().numpy(), got[:, 84:])
    for i, r in enumerate(raw):
        np.testing.assert_allclose(r.float().cpu().numpy(), g[f"raw{i}"], err_msg=f"raw{i}", **LAYER_TOL)


def test_fp16_vs_reference_golden(golden):
    """Throughput mode, the f16 rule of tests/test_gpu_model.py: scores within 2e-2, boxes within 1.5 % of the image size; the angle, a
    sigmoid output scaled by pi, within pi * 2e-2."""
    g = golden
    m = _build("yolo11n-obb.yaml", torch.float16)
    y, (raw, angle) = m(synth.synth_images(*SHAPE).cuda().half())
    y = y.cpu().numpy()
    assert y.dtype == np.float32 and y.shape == g["y"].shape
    assert float(np.abs(y[:, 4:84] - g["y"][:, 4:84]).max()) < 2e-2
    assert float(np.abs(y[:, :4] - g["y"][:, :4]).max()) < 0.015 * max(SHAPE[2:])
    assert float(np.abs(y[:, 84:] - g["y"][:, 84:]).max()) < np.pi * 2e-2


def test_head_module_angle_row_under_the_rule(golden_dir):
    """The OBB head on small maps with the reference's weights: y at the fp32 layer bar; the angle row, recomputed in float64 from this run's
    own angle logits, under 4 E + 2 ulp with E = the reference's fp32 error against float64 on the same logits."""
    from edge_yolo_amd import _lib as L
    from edge_yolo_amd.nn import modules as M
    g = np.load(os.path.join(golden_dir, "obb_ops.npz"))
    tag, kw, shapes = obb_synth.HEAD_CASE
    M.OBB.legacy = False
    m = M.OBB(**kw)
    m.stride = torch.tensor([8.0, 16.0, 32.0])
    m.load_state_dict(obb_synth.state_dict(m.state_dict(), prefix=tag + "."))
    m = m.cuda().float().eval()
    xs = [obb_synth.case_input(f"{tag}{i}", s).cuda() for i, s in enumerate(shapes)]
    y, (raw, angle) = m(xs)
    got = y.cpu().numpy()
    np.testing.assert_allclose(got, g[tag + "_y"], **LAYER_TOL)
    for i, r in enumerate(raw):
        np.testing.assert_allclose(r.float().cpu().numpy(), g[f"{tag}_raw{i}"], **LAYER_TOL)
    # the angle row from this run's own logits
    logits = torch.cat([a.float().flatten(2) for a in m.angle_maps([L.as_nhwc(t) for t in xs])], 2).cpu().numpy().astype(np.float64)
    ref64 = (1.0 / (1.0 + np.exp(-logits)) - 0.25) * np.pi
    l32 = torch.tensor(logits.astype(np.float32))
    ref32 = ((l32.sigmoid() - 0.25) * float(np.pi)).numpy().astype(np.float64)  # the reference's expression (head.py:388) in fp32
    E = float(np.abs(ref32 - ref64).max())
    err = np.abs(got[:, 84:].astype(np.float64) - ref64)
    print(f"{tag} angle: E {E:.3e} achieved {float(err.max()):.3e}")
    assert (err <= f64.bound(E, ref64)).all()


def test_nms_on_the_golden_prediction(golden):
    from edge_yolo_amd.utils import ops as uops
    g = golden
    out = uops.non_max_suppression(torch.tensor(g["y"]).cuda(), float(g["conf"]), 0.7, nc=80, rotated=True)
    assert g["margin0"].min() > 1e-3 and len(g["det0"]) >= 5
    np.testing.assert_array_equal(out[0].cpu().numpy(), g["det0"])


@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
def test_predict_end_to_end(golden, half):
    import edge_yolo_amd
    g = golden
    model = edge_yolo_amd.YOLO("yolo11n-obb.yaml")
    assert model.task == "obb"
    model.model.load_state_dict(obb_synth.state_dict(model.model.state_dict()))
    x = synth.synth_images(*SHAPE)
    res = model.predict(x, conf=float(g["conf"]), iou=0.7, half=half, device="cuda:0")
    assert len(res) == 1 and res[0].boxes is None and res[0].masks is None and res[0].obb is not None
    r = res[0].obb
    assert r.orig_shape == (64, 96) and tuple(r.data.shape)[1] == 7 and len(res[0]) == len(r)
    # what the predictor must have done with its own device step: regularise, scale (gain 1, no padding: a clip), append conf and cls
    from edge_yolo_amd.utils import ops as uops
    rows, count, index, pred = model.predictor._device_step(model.predictor.preprocess(x))
    n = int(count[0])
    det = rows[0, :n]
    rb = uops.regularize_rboxes(torch.cat([det[:, :4], det[:, -1:]], -1))
    rb[:, :4] = uops.scale_boxes((64, 96), rb[:, :4], (64, 96), xywh=True)
    assert torch.equal(r.data, torch.cat([rb, det[:, 4:6]], -1)) and n >= 5
    assert bool((r.xywhr[:, 2] >= r.xywhr[:, 3]).all()) and bool((r.xywhr[:, 4] >= 0).all()) and bool((r.xywhr[:, 4] < np.pi).all())
    assert tuple(r.xyxyxyxy.shape) == (n, 4, 2) and tuple(r.xyxy.shape) == (n, 4)
    if not half:
        # fp32: the reference's final rows.  The forward agrees to ~1e-4, which cannot flip a column here (smallest margin > 1e-3 in the
        # golden) nor the score order of the kept rows; values at the fp32 layer bar
        want = g["obb0"]
        assert r.data.shape == want.shape
        np.testing.assert_array_equal(r.cls.cpu().numpy(), want[:, 6])
        np.testing.assert_allclose(r.data.cpu().numpy(), want, **LAYER_TOL)
        np.testing.assert_allclose(r.xyxy.cpu().numpy(), g["obb0_xyxy"], rtol=1e-4, atol=1e-3)
    again = model.predict(x, conf=float(g["conf"]), iou=0.7, half=half, device="cuda:0")  # graph replay
    assert torch.equal(again[0].obb.data, r.data)
    eager = model.predict(x, conf=float(g["conf"]), iou=0.7, half=half, device="cuda:0", graph=False)
    assert torch.equal(eager[0].obb.data, r.data)
    none = model.predict(synth.synth_images(2, 64, 96), conf=0.9999, device="cuda:0", half=half)
    assert len(none) == 2 and all(len(q) == 0 and q.obb is not None and q.boxes is None for q in none)
    with pytest.warns(UserWarning, match="augment"):
        aug = model.predict(x, conf=float(g["conf"]), iou=0.7, half=half, device="cuda:0", augment=True)
    assert torch.equal(aug[0].obb.data, r.data)


def test_predict_ndarray_source_of_another_aspect(golden):
    """uint8 HWC images taller than wide (120x70 at imgsz 96: a 96x64 network input, gain 0.8, padded left and right), so
    scale_boxes(..., xywh=True) runs with a gain and a pad.  Graph on and off agree exactly; the results are what the reference's
    post-process makes of the predictor's own device step."""
    import edge_yolo_amd
    from edge_yolo_amd.utils import ops as uops
    model = edge_yolo_amd.YOLO("yolo11n-obb.yaml")
    model.model.load_state_dict(obb_synth.state_dict(model.model.state_dict()))
    r = np.random.default_rng(3)
    ims = [r.integers(0, 256, (120, 70, 3), dtype=np.uint8) for _ in range(2)]
    kw = dict(conf=float(golden["conf"]), iou=0.7, imgsz=96, device="cuda:0")  # the golden's conf
    res = model.predict(ims, **kw)
    eager = model.predict(ims, graph=False, **kw)
    p = model.predictor
    im = p.preprocess(ims)
    assert tuple(im.shape) == (2, 3, 96, 64)
    rows, count, index, _ = p._device_step(im)
    for i, (a, e) in enumerate(zip(res, eager)):
        n = int(count[i])
        print(f"image {i}: kept {n}")
        assert a.boxes is None and len(a) == len(a.obb) == n >= 1 and a.orig_shape == a.obb.orig_shape == (120, 70)
        assert torch.equal(a.obb.data, e.obb.data)
        det = rows[i, :n]
        rb = uops.regularize_rboxes(torch.cat([det[:, :4], det[:, -1:]], -1))
        rb[:, :4] = uops.scale_boxes(im.shape[2:], rb[:, :4], (120, 70), xywh=True)
        assert torch.equal(a.obb.data, torch.cat([rb, det[:, 4:6]], -1))


@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
def test_predict_with_class_filter(golden, half):
    """predict(classes=[...]) through the captured graph: the class mask is uploaded by the warm-up calls, never inside the capture; the
    capture's own result and its replay equal the eager run, and only the asked classes come back."""
    import edge_yolo_amd
    g = golden
    model = edge_yolo_amd.YOLO("yolo11n-obb.yaml")
    model.model.load_state_dict(obb_synth.state_dict(model.model.state_dict()))
    x = synth.synth_images(*SHAPE)
    conf = float(g["conf"])
    allc = model.predict(x, conf=conf, iou=0.7, half=half, device="cuda:0", graph=False)[0].obb
    seen = sorted(set(int(c) for c in allc.cls.cpu().tolist()))
    assert len(seen) >= 2
    classes = seen[::2]  # every other class that occurs: some rows stay, some go
    eager = model.predict(x, conf=conf, iou=0.7, half=half, device="cuda:0", classes=classes, graph=False)[0].obb
    first = model.predict(x, conf=conf, iou=0.7, half=half, device="cuda:0", classes=classes)[0].obb  # warm-up, capture, first replay
    replay = model.predict(x, conf=conf, iou=0.7, half=half, device="cuda:0", classes=classes)[0].obb
    assert 0 < len(eager) < len(allc) and set(int(c) for c in eager.cls.cpu().tolist()) <= set(classes)
    assert torch.equal(first.data, eager.data) and torch.equal(replay.data, eager.data)
    # the filter removes candidates BEFORE suppression (reference ops.py:277-279): the rows of the asked classes that survive without a
    # filter survive with it too (class offsets keep other classes from suppressing them)
    keep = torch.isin(allc.cls, torch.tensor(classes, device=allc.cls.device, dtype=allc.cls.dtype))
    assert torch.equal(eager.data, allc.data[keep])


def test_val_and_predict_batches_raise():
    import edge_yolo_amd
    model = edge_yolo_amd.YOLO("yolo11n-obb.yaml")
    x = torch.zeros(1, 3, 64, 64, device="cuda")
    with pytest.raises(NotImplementedError, match="obb"):
        model.val([{"img": x}])
    with pytest.raises(NotImplementedError, match="obb"):
        next(iter(model.predict_batches([x])))
    head = model.model.model[-1]
    with pytest.raises(NotImplementedError):
        model.model.to("cuda").fuse().float().eval()(x, head_nms={"conf": 0.25, "classes": None})
    assert head.__class__.__name__ == "OBB"


@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
def test_obb_row_on_the_edgeline_backbone(half):
    from edge_yolo_amd.nn.tasks import yaml_model_load
    from edge_yolo_amd.utils import ops as uops
    m = _build(obb_synth.edgeline_obb_cfg(yaml_model_load("yolo11n-test.yaml")), torch.float16 if half else torch.float32)
    x = synth.synth_images(2, 64, 64).cuda()
    y, (raw, angle) = m(x.half() if half else x)
    assert tuple(y.shape) == (2, 85, 84) and y.dtype == torch.float32 and bool(torch.isfinite(y).all()) and len(raw) == 3
    a = y[:, 84]
    assert bool((a >= -np.pi / 4).all()) and bool((a <= 3 * np.pi / 4).all()) and bool((y[:, 4:84] >= 0).all()) and bool((y[:, 4:84] <= 1).all())
    rows, count, index = uops.nms_device(y, 0.05, 0.7, nc=80, rotated=True)
    o = f64.nms_rotated64(y.cpu().numpy(), 0.05, 0.7)
    for b in range(2):
        if o[b]["margin"].size == 0 or o[b]["margin"].min() > 1e-4:
            np.testing.assert_array_equal(rows[b, :int(count[b])].cpu().numpy(), o[b]["rows"])
