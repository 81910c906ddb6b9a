"""-m gpu: the classify task end to end.  yolo11n-cls (2x3x64x64, synthetic weights) against the reference's forward (tests/golden/
yolo11n_cls_64.npz, the fp32 parity bars of tests/test_gpu_obb_model.py / test_gpu_pose_model.py for class scores), an f16 run (top-1 equal,
top-5 as a set), YOLO(...).predict() on a tensor, on ndarrays and on a uint8 batch (Results with `probs` and nothing else; graph on and off
bit for bit), and YOLO(...).val() on the images and labels of tests/golden/clsval_case.npz against the reference's own validator."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import cls_synth  # noqa: E402
import synthdata as synth  # noqa: E402

LAYER_TOL = dict(rtol=1e-4, atol=2e-4)  # tests/test_gpu_obb_model.py, fp32 layers
SHAPE = (2, 64, 64)


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "yolo11n_cls_64.npz"))


@pytest.fixture(scope="module")
def case(golden_dir):
    return np.load(os.path.join(golden_dir, "clsval_case.npz"))


def _build(dtype, nc=80):
    from edge_yolo_amd.nn.tasks import ClassificationModel
    m = ClassificationModel("yolo11n-cls.yaml", nc=nc)
    m.load_state_dict(cls_synth.state_dict(m.state_dict()))
    m = m.to("cuda")
    m.fuse()
    return (m.half() if dtype == torch.float16 else m.float()).eval()


def _facade(nc=80):
    import edge_yolo_amd
    model = edge_yolo_amd.YOLO("yolo11n-cls.yaml", nc=nc)
    model.model.load_state_dict(cls_synth.state_dict(model.model.state_dict()))
    return model


def test_fp32_vs_reference_golden_and_launches(golden):
    from edge_yolo_amd import profiling
    g = golden
    m = _build(torch.float32)
    x = synth.synth_images(*SHAPE).cuda()
    probs, logits = m(x)
    assert probs.dtype == logits.dtype == torch.float32 and tuple(probs.shape) == tuple(logits.shape) == g["probs"].shape == (2, 80)
    gp, gl = probs.cpu().numpy(), logits.cpu().numpy()
    print(f"yolo11n_cls_64: max abs err probs {float(np.abs(gp - g['probs']).max()):.3e} logits {float(np.abs(gl - g['logits']).max()):.3e}")
    np.testing.assert_allclose(gl, g["logits"], err_msg="logits", **LAYER_TOL)
    np.testing.assert_allclose(gp, g["probs"], err_msg="probs", **LAYER_TOL)
    topi, topp = m.model[-1].top5
    np.testing.assert_array_equal(topi.cpu().numpy(), g["top5"])
    np.testing.assert_array_equal(topp.cpu().numpy(), np.take_along_axis(gp, g["top5"].astype(np.int64), 1))
    # the head's eval forward is two launches
    head = m.model[-1]
    feat = torch.randn(2, head.conv.conv.in_channels, 2, 2, device="cuda").contiguous(memory_format=torch.channels_last)
    with profiling.trace() as t:
        head(feat)
    assert [r[0] for r in t.records] == ["classify_pool_kernel", "classify_linear_softmax_kernel"], [r[0] for r in t.records]
    a, b = head([feat[:, :128], feat[:, 128:]]), head(feat)  # a list input is concatenated on channels first
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_f16_top1_equal_top5_as_a_set(golden):
    m = _build(torch.float16)
    probs, logits = m(synth.synth_images(*SHAPE).cuda().half())
    assert probs.dtype == torch.float32 and logits.dtype == torch.float32
    topi = m.model[-1].top5[0].cpu().numpy()
    print(f"f16: max abs err probs {float(np.abs(probs.cpu().numpy() - golden['probs']).max()):.3e} top5 {topi.tolist()}")
    assert topi[:, 0].tolist() == golden["top5"][:, 0].tolist()
    assert [set(r) for r in topi.tolist()] == [set(r) for r in golden["top5"].tolist()]


def _only_probs(results, n, nc=80):
    assert len(results) == n
    for r in results:
        assert r.probs is not None and r.boxes is None and r.masks is None and r.obb is None and r.keypoints is None
        assert tuple(r.probs.data.shape) == (nc,) and len(r.probs.top5) == 5 and r.probs.top1 == r.probs.top5[0]
        assert float(r.probs.top1conf) == float(r.probs.data.max()) and r.probs.data.dtype == torch.float32


def test_predict_tensor_ndarray_and_uint8_batch(golden):
    from edge_yolo_amd.data.augment import ClassifyTransform
    model = _facade()
    x = synth.synth_images(*SHAPE)
    res = model.predict(x.cuda(), conf=0.9, iou=0.1, max_det=3, classes=[1], agnostic_nms=True)  # accepted and ignored
    _only_probs(res, 2)
    for i, r in enumerate(res):
        assert r.probs.top5 == golden[f"p{i}_top5"].tolist() and r.probs.top1 == int(golden[f"p{i}_top1"]) and r.orig_shape == (64, 64)
        np.testing.assert_allclose(r.probs.data.cpu().numpy(), golden["probs"][i], **LAYER_TOL)
        np.testing.assert_allclose(r.probs.top5conf.cpu().numpy(), golden[f"p{i}_top5conf"], **LAYER_TOL)
        assert r.probs.numpy().top5 == r.probs.top5
    eager = model.predict(x.cuda(), graph=False)
    for a, b in zip(res, eager):  # graph and non-graph outputs are equal bit for bit
        assert torch.equal(a.probs.data, b.probs.data) and a.probs.top5 == b.probs.top5
    # ndarrays of different shapes: one transform launch per image, then the same forward
    r = np.random.default_rng(5)
    ims = [r.integers(0, 256, (40, 56, 3), dtype=np.uint8), r.integers(0, 256, (70, 64, 3), dtype=np.uint8)]
    res = model.predict(ims, imgsz=64)
    _only_probs(res, 2)
    assert res[0].orig_shape == (40, 56) and res[1].orig_shape == (70, 64)
    xt = ClassifyTransform(64).batch(ims, "cuda", torch.float32)
    want = model.predict(xt)
    for a, b in zip(res, want):
        assert torch.equal(a.probs.data, b.probs.data)
    assert torch.equal(model.predict(ims[0], imgsz=64)[0].probs.data, res[0].probs.data)
    # a decoded uint8 batch: transform + forward as one captured graph, equal to the eager route
    u8 = torch.tensor(np.stack([ims[0], ims[0][::-1].copy()]))
    got = model.predict(u8, imgsz=64)
    _only_probs(got, 2)
    want = model.predict(ClassifyTransform(64).batch_tensor(u8.cuda(), torch.float32), graph=False)
    for a, b in zip(got, want):
        assert torch.equal(a.probs.data, b.probs.data) and a.probs.top5 == b.probs.top5
    with pytest.raises(NotImplementedError, match="augment"):
        model.predict(x.cuda(), augment=True)


def test_val_reproduces_the_reference_validator(case):
    nc = int(case["nc"])
    model = _facade(nc)
    B = cls_synth.VAL_SHAPE[0]
    batches = [{"img": cls_synth.val_images(i), "cls": torch.tensor(case["cls"][i * B:(i + 1) * B])} for i in range(cls_synth.VAL_BATCHES)]
    res = model.val(batches)
    print("val", res, "reference", dict(zip(case["keys"].tolist(), case["values"].tolist())))
    assert list(res) == case["keys"].tolist()
    np.testing.assert_array_equal(np.concatenate(model.validator.pred), case["pred"])
    assert list(res.values()) == case["values"].tolist()
