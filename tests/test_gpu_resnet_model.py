"""-m gpu: the ResNet classifiers end to end (synthetic weights, tests/resnet_synth.py) against the reference's CPU fp32 forward
(tests/golden/resnet50_cls.npz, resnet101_cls.npz, resnetval_case.npz; the fp32 parity bars of tests/test_gpu_cls_model.py).

* yolov8n-cls-resnet50, fp32: the output of every layer at 2x3x32x32, logits and probabilities at 2x3x32x32 and 2x3x64x64, the top-5
  classes, and the launches of one forward (2 for the stem, 3 per identity block, 4 per projection block with its shortcut conv, 2 for the
  head: 56 in fp32; 55 in f16, where the first projection block closes with one ey_resnet_tail launch).
* yolov8n-cls-resnet101, fp32: logits (and what follows from them).
* f16: top-1 equal and top-5 equal as a set.  Decidable on the reference alone: the generator asserts that the reference, run with weights and
  image rounded to f16, keeps both.
* YOLO(...).predict() and .val() on a two-batch fixture: the reference validator's top-1 / top-5 accuracy exactly; graph replay and the eager
  route give the same bits."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import resnet_synth as rs  # noqa: E402
import synthdata as synth  # noqa: E402

LAYER_TOL = dict(rtol=1e-4, atol=2e-4)  # tests/test_gpu_cls_model.py, fp32 layers
R50, R101 = "yolov8n-cls-resnet50.yaml", "yolov8n-cls-resnet101.yaml"


@pytest.fixture(scope="module")
def g50(golden_dir):
    return np.load(os.path.join(golden_dir, "resnet50_cls.npz"))


@pytest.fixture(scope="module")
def g101(golden_dir):
    return np.load(os.path.join(golden_dir, "resnet101_cls.npz"))


@pytest.fixture(scope="module")
def case(golden_dir):
    return np.load(os.path.join(golden_dir, "resnetval_case.npz"))


def _build(name, dtype, nc=rs.RESNET_NC):
    from edge_yolo_amd.nn.tasks import ClassificationModel
    m = ClassificationModel(name, nc=nc)
    m.load_state_dict(rs.state_dict(m.state_dict(), seed=rs.RESNET_SEED[name]))
    m = m.to("cuda")
    m.fuse()
    return (m.half() if dtype == torch.float16 else m.float()).eval()


@pytest.fixture(scope="module")
def m50_fp32():
    return _build(R50, torch.float32)


def test_resnet50_fp32_layers_at_32(g50, m50_fp32):
    m = m50_fp32
    x = synth.synth_images(*rs.RESNET_LAYER_SHAPE).cuda()
    t = x
    for layer in m.model[:-1]:
        t = layer(t)
        got, want = t.float().cpu().numpy(), g50[f"layer{layer.i}"]
        assert got.shape == want.shape, (layer.i, got.shape)
        print(f"resnet50 layer {layer.i} {got.shape}: max abs err {float(np.abs(got - want).max()):.3e} max |x| {float(np.abs(want).max()):.2f}")
        np.testing.assert_allclose(got, want, err_msg=f"layer {layer.i}", **LAYER_TOL)
    probs, logits = m(x)
    np.testing.assert_allclose(logits.cpu().numpy(), g50["logits32"], err_msg="logits", **LAYER_TOL)
    np.testing.assert_allclose(probs.cpu().numpy(), g50["probs32"], err_msg="probs", **LAYER_TOL)


def test_resnet50_fp32_at_64_and_launches(g50, m50_fp32):
    from edge_yolo_amd import profiling
    m = m50_fp32
    x = synth.synth_images(*rs.RESNET_SHAPE).cuda()
    with profiling.trace() as t:
        probs, logits = m(x)
    labels = [r[0] for r in t.records]
    assert len(labels) == 56 and labels[0] == "stem7_kernel" and labels[1] == "maxpool3x3s2_kernel" and "resnet_tail_kernel" not in labels, labels  # fp32: composed tails
    assert labels[-2:] == ["classify_pool_kernel", "classify_linear_softmax_kernel"]
    gp, gl = probs.cpu().numpy(), logits.cpu().numpy()
    print(f"resnet50 64x64: max abs err probs {float(np.abs(gp - g50['probs']).max()):.3e} logits {float(np.abs(gl - g50['logits']).max()):.3e}")
    np.testing.assert_allclose(gl, g50["logits"], err_msg="logits", **LAYER_TOL)
    np.testing.assert_allclose(gp, g50["probs"], err_msg="probs", **LAYER_TOL)
    np.testing.assert_array_equal(m.model[-1].top5[0].cpu().numpy(), g50["top5"])


def test_resnet101_fp32_logits(g101):
    m = _build(R101, torch.float32)
    probs, logits = m(synth.synth_images(*rs.RESNET_SHAPE).cuda())
    gl = logits.cpu().numpy()
    print(f"resnet101 64x64: max abs err logits {float(np.abs(gl - g101['logits']).max()):.3e}")
    np.testing.assert_allclose(gl, g101["logits"], err_msg="logits", **LAYER_TOL)
    np.testing.assert_allclose(probs.cpu().numpy(), g101["probs"], err_msg="probs", **LAYER_TOL)


@pytest.mark.parametrize("name,tag", [(R50, "resnet50_cls"), (R101, "resnet101_cls")], ids=["resnet50", "resnet101"])
def test_f16_top1_equal_top5_as_a_set(golden_dir, name, tag):
    g = np.load(os.path.join(golden_dir, tag + ".npz"))
    from edge_yolo_amd import profiling
    m = _build(name, torch.float16)
    with profiling.trace() as t:
        probs, logits = m(synth.synth_images(*rs.RESNET_SHAPE).cuda().half())
    labels = [r[0] for r in t.records]
    assert labels[0] == "stem7_mfma_kernel" and labels.count("resnet_tail_kernel") == 1 and len(labels) == (55 if name == R50 else 106), labels
    assert probs.dtype == torch.float32 and logits.dtype == torch.float32 and bool(torch.isfinite(logits).all())
    topi = m.model[-1].top5[0].cpu().numpy()
    print(f"{tag} f16: max abs err probs {float(np.abs(probs.cpu().numpy() - g['probs']).max()):.3e} top5 {topi.tolist()} reference {g['top5'].tolist()}")
    assert topi[:, 0].tolist() == g["top5"][:, 0].tolist()
    assert [set(r) for r in topi.tolist()] == [set(r) for r in g["top5"].tolist()]


def _facade(nc):
    import edge_yolo_amd
    model = edge_yolo_amd.YOLO(R50, nc=nc)
    model.model.load_state_dict(rs.state_dict(model.model.state_dict(), seed=rs.RESNET_SEED[R50]))
    return model


def test_predict_and_val_reproduce_the_reference_validator(case):
    nc = int(case["nc"])
    model = _facade(nc)
    assert model.task == "classify"
    B = rs.VAL_SHAPE[0]
    for i in range(rs.VAL_BATCHES):
        res = model.predict(rs.val_images(i).cuda())
        assert len(res) == B and all(r.probs is not None and r.boxes is None for r in res)
        for j, r in enumerate(res):
            assert r.probs.top5 == case["top5"][i * B + j].tolist() and r.probs.top1 == int(case["top5"][i * B + j][0])
            np.testing.assert_allclose(r.probs.data.cpu().numpy(), case["probs"][i * B + j], **LAYER_TOL)
    batches = [{"img": rs.val_images(i), "cls": torch.tensor(case["cls"][i * B:(i + 1) * B])} for i in range(rs.VAL_BATCHES)]
    res = model.val(batches)
    print("val", res, "reference", dict(zip(case["keys"].tolist(), case["values"].tolist())))
    assert list(res) == case["keys"].tolist()
    np.testing.assert_array_equal(np.concatenate(model.validator.pred), case["pred"])
    assert list(res.values()) == case["values"].tolist()


def test_graph_replay_equals_the_eager_route():
    model = _facade(rs.RESNET_NC)
    x = synth.synth_images(*rs.RESNET_SHAPE).cuda()
    for half in (False, True):
        first = model.predict(x, half=half)   # warm-up, capture, first replay
        again = model.predict(x, half=half)   # replay
        eager = model.predict(x, half=half, graph=False)
        for a, b, c in zip(first, again, eager):
            assert torch.equal(a.probs.data, b.probs.data) and torch.equal(a.probs.data, c.probs.data) and a.probs.top5 == c.probs.top5
