"""-m gpu: the pose task end to end.  yolo11n-pose (64x96, synthetic weights) against the reference's forward (tests/golden, the parity
bars of tests/test_gpu_obb_model.py), the keypoint rows of the eval-mode return against ey_kpts_decode_rows at the kept anchors,
YOLO(...).predict() against the reference's post-processed rows (graph on and off, tensor and ndarray sources), an f16 run, and
YOLO(...).val() on the images and labels of tests/golden/poseval_case.npz against the reference's own validator."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import pose_synth  # noqa: E402
import synthdata as synth  # noqa: E402
from test_pose_cpu import KEYS10  # noqa: E402

LAYER_TOL = dict(rtol=1e-4, atol=2e-4)  # tests/test_gpu_obb_model.py, fp32 layers
TAG, SHAPE = "yolo11n_pose_64x96", (2, 64, 96)
STRIDES, SIZES = (8.0, 16.0, 32.0), (96, 24, 6)  # anchors per level at 64x96


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, TAG + ".npz"))


@pytest.fixture(scope="module")
def case(golden_dir):
    return np.load(os.path.join(golden_dir, "poseval_case.npz"))


def _build(cfg, dtype):
    from edge_yolo_amd.nn.tasks import PoseModel
    m = PoseModel(cfg)
    m.load_state_dict(pose_synth.state_dict(m.state_dict()))
    m = m.to("cuda")
    m.fuse()
    return (m.half() if dtype == torch.float16 else m.float()).eval()


def _facade():
    import edge_yolo_amd
    model = edge_yolo_amd.YOLO("yolo11n-pose.yaml")
    model.model.load_state_dict(pose_synth.state_dict(model.model.state_dict()))
    return model


def test_fp32_vs_reference_golden_and_kept_rows(golden):
    from edge_yolo_amd.nn import _ops
    from edge_yolo_amd.utils import ops as uops
    g = golden
    m = _build("yolo11n-pose.yaml", torch.float32)
    x = synth.synth_images(*SHAPE).cuda()
    y, (raw, kpt) = m(x)
    assert y.dtype == torch.float32 and tuple(y.shape) == g["y"].shape == (2, 135, 126) and tuple(kpt.shape) == g["kpt"].shape == (2, 51, 126)
    got = y.cpu().numpy()
    print(f"{TAG} y: max abs err boxes/classes {float(np.abs(got[:, :84] - g['y'][:, :84]).max()):.3e} keypoint rows {float(np.abs(got[:, 84:] - g['y'][:, 84:]).max()):.3e}"
          f" logits {float(np.abs(kpt.float().cpu().numpy() - g['kpt']).max()):.3e}")
    np.testing.assert_allclose(kpt.float().cpu().numpy(), g["kpt"], err_msg="kpt", **LAYER_TOL)
    np.testing.assert_allclose(got, g["y"], err_msg="y", **LAYER_TOL)
    # the validator's switch: boxes and classes without the (B, nk, A) decode, the same bits
    head = m.model[-1]
    head.decode_kpts = False
    try:
        y2, (_, maps) = m(x)
    finally:
        head.decode_kpts = True
    assert tuple(y2.shape) == (2, 84, 126) and torch.equal(y2, y[:, :84]) and len(maps) == 3 and tuple(maps[0].shape) == (2, 51, 8, 12)
    # the keypoint rows of the full decode equal ey_kpts_decode_rows at the anchors NMS keeps
    conf = float(g["conf"])
    cand, (_, maps) = m(x, head_nms={"conf": conf, "classes": None, "keep_pred": False})
    boxes, count, index = uops.nms_device(cand, conf, 0.7, None, False, 300)
    rows = _ops.kpts_decode_rows(head.kpt_levels(maps), head.kpt_shape, index, count).cpu().numpy()
    n, idx = count.cpu().numpy(), index.cpu().numpy()
    assert (n >= 5).all()
    for b in range(2):
        np.testing.assert_array_equal(rows[b, :n[b]], got[b][84:][:, idx[b, :n[b]]].T.reshape(n[b], 17, 3))
        assert (rows[b, n[b]:] == 0).all()


def test_fp16_is_finite_and_within_the_f16_bar(golden):
    """The f16 rule of tests/test_gpu_model.py: scores within 2e-2, boxes within 1.5 % of the image size.  Keypoints: the score bar sits on a
    sigmoid, whose slope is at most 1/4, so it admits logit errors of 8e-2; the decode multiplies a logit error by 2 * stride, hence x / y
    within 0.16 * stride of the level; the keypoint confidences are sigmoid outputs under the score bar."""
    g = golden
    m = _build("yolo11n-pose.yaml", torch.float16)
    y, _ = m(synth.synth_images(*SHAPE).cuda().half())
    y = y.cpu().numpy()
    assert y.dtype == np.float32 and y.shape == g["y"].shape and np.isfinite(y).all()
    assert float(np.abs(y[:, 4:84] - g["y"][:, 4:84]).max()) < 2e-2
    assert float(np.abs(y[:, :4] - g["y"][:, :4]).max()) < 0.015 * max(SHAPE[2:])
    k, kr = y[:, 84:].reshape(2, 17, 3, 126), g["y"][:, 84:].reshape(2, 17, 3, 126)
    assert float(np.abs(k[:, :, 2] - kr[:, :, 2]).max()) < 2e-2
    per_anchor = np.repeat(np.array(STRIDES), SIZES) * 0.16
    err = np.abs(k[:, :, :2] - kr[:, :, :2])
    print(f"f16 keypoints: worst |xy error| / stride {float((err / (per_anchor / 0.16)).max()):.3e} (bar 0.16)")
    assert (err <= per_anchor).all()


@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
def test_predict_end_to_end(golden, half):
    g = golden
    model = _facade()
    assert model.task == "pose"
    x = synth.synth_images(*SHAPE)
    kw = dict(conf=float(g["conf"]), iou=0.7, half=half, device="cuda:0")
    res = model.predict(x, **kw)
    assert len(res) == 2 and all(r.masks is None and r.obb is None and r.boxes is not None and r.keypoints is not None for r in res)
    for i, r in enumerate(res):
        n = len(r)
        assert r.orig_shape == r.keypoints.orig_shape == (64, 96) and tuple(r.keypoints.data.shape) == (n, 17, 3) and r.keypoints.has_visible and n >= 5
        b = r.boxes.data
        assert torch.equal(b[:, :4], b[:, :4].round()) and bool((b[:, :4] >= 0).all()) and bool((b[:, [0, 2]] <= 96).all()) and bool((b[:, [1, 3]] <= 64).all())
        k = r.keypoints
        assert bool((k.xy[..., 0] >= 0).all()) and bool((k.xy[..., 0] <= 96).all()) and bool((k.xy[..., 1] <= 64).all())
        assert bool((k.xy[k.conf < 0.5] == 0).all())
        if not half:
            # fp32: the reference's post-processed rows.  The forward agrees to ~1e-4, which does not reorder the kept rows of this fixture
            wb, wk = g[f"boxes{i}"], g[f"kp{i}_data"]
            print(f"image {i}: kept {n}/{len(wb)} box gap {float(np.abs(b.cpu().numpy() - wb).max()) if n == len(wb) else -1:.3e}")
            assert b.shape == wb.shape
            np.testing.assert_array_equal(b[:, :4].cpu().numpy(), wb[:, :4])  # rounded
            np.testing.assert_array_equal(b[:, 5].cpu().numpy(), wb[:, 5])
            np.testing.assert_allclose(b[:, 4].cpu().numpy(), wb[:, 4], **LAYER_TOL)
            vis = (k.conf.cpu().numpy() < 0.5) == (g[f"kp{i}_conf"] < 0.5)  # (a confidence within 1e-4 of 0.5 may fall on the other side)
            assert vis.mean() > 0.99
            np.testing.assert_allclose(k.data.cpu().numpy()[vis], wk[vis], **LAYER_TOL)
            np.testing.assert_allclose(k.xyn.cpu().numpy()[vis], g[f"kp{i}_xyn"][vis], rtol=1e-4, atol=1e-5)
    again = model.predict(x, **kw)  # graph replay
    eager = model.predict(x, graph=False, **kw)
    for a, e, r in zip(again, eager, res):
        assert torch.equal(a.boxes.data, r.boxes.data) and torch.equal(a.keypoints.data, r.keypoints.data)
        assert torch.equal(e.boxes.data, r.boxes.data) and torch.equal(e.keypoints.data, r.keypoints.data)
    none = model.predict(synth.synth_images(2, 64, 96), conf=0.9999, device="cuda:0", half=half)
    assert len(none) == 2 and all(len(q) == 0 and tuple(q.keypoints.data.shape) == (0, 17, 3) for q in none)
    with pytest.warns(UserWarning, match="augment"):
        aug = model.predict(x, augment=True, **kw)
    assert torch.equal(aug[0].keypoints.data, res[0].keypoints.data)


def test_predict_ndarray_source_of_another_aspect(golden):
    """uint8 HWC images taller than wide: letterboxed with padding, so scale_boxes / scale_coords run with a gain and a pad.  Graph on and
    off agree exactly; the results are what the reference's post-process makes of the predictor's own device step."""
    from edge_yolo_amd.utils import ops as uops
    model = _facade()
    r = np.random.default_rng(3)
    ims = [r.integers(0, 256, (120, 70, 3), dtype=np.uint8) for _ in range(2)]
    kw = dict(conf=float(golden["conf"]), iou=0.7, device="cuda:0")
    res = model.predict(ims, **kw)
    eager = model.predict(ims, graph=False, **kw)
    p = model.predictor
    im = p.preprocess(ims)
    assert tuple(im.shape[2:]) != (120, 70)
    boxes, count, index, _, kpts = p._device_step(im)
    for i, (a, e) in enumerate(zip(res, eager)):
        n = int(count[i])
        assert len(a) == n >= 1 and a.orig_shape == (120, 70)
        assert torch.equal(a.boxes.data, e.boxes.data) and torch.equal(a.keypoints.data, e.keypoints.data)
        det, kp = boxes[i, :n].clone(), kpts[i, :n].clone()
        det[:, :4] = uops.scale_boxes(im.shape[2:], det[:, :4], (120, 70, 3)).round()
        kp = uops.scale_coords(im.shape[2:], kp, (120, 70, 3))
        kp[..., :2][kp[..., 2] < 0.5] = 0
        assert torch.equal(a.boxes.data, det) and torch.equal(a.keypoints.data, kp)
        # ... and the same arithmetic on the host (true division there; the device multiplies by the reciprocal of a scalar divisor)
        hk = uops.scale_coords(im.shape[2:], kpts[i, :n].cpu().clone(), (120, 70, 3))
        hk[..., :2][hk[..., 2] < 0.5] = 0
        np.testing.assert_allclose(a.keypoints.data.cpu().numpy(), hk.numpy(), rtol=1e-6, atol=1e-5)
        assert bool((a.keypoints.xy[..., 0] <= 70).all()) and bool((a.keypoints.xy[..., 1] <= 120).all()) and bool((a.keypoints.xy >= 0).all())


def _batch(g):
    return pose_synth.poseval_batch(g, img=pose_synth.poseval_images(g))


def test_val_vs_reference(case):
    """YOLO.val on the reference's images and labels: internally consistent exactly (the validator's own rows and keypoints through the numpy
    route give the same statistics), tp / tp_p equal to the reference's, metrics at the end-to-end tolerance of
    tests/test_gpu_segval_model.py (0.02 in fp32)."""
    from edge_yolo_amd.engine.validator import PoseValidator
    g = case
    model = _facade()
    res = dict(model.val([_batch(g)], device="cuda:0"))
    v = PoseValidator(model.model)
    v.keep_outputs = True
    assert dict(v([_batch(g)])) == res and list(res) == KEYS10 + ["fitness"]
    tp, tp_p = np.concatenate(v.stats["tp"]), np.concatenate(v.stats["tp_p"])
    h = PoseValidator(model.model)
    h.device = torch.device("cpu")
    h.update_metrics(([r for r, _ in v.kept], [k for _, k in v.kept]), pose_synth.poseval_batch(g))
    np.testing.assert_array_equal(np.concatenate(h.stats["tp"]), tp)
    np.testing.assert_array_equal(np.concatenate(h.stats["tp_p"]), tp_p)
    assert h.get_stats() == res
    ref = dict(zip(list(g["full_keys"]), g["full_values"]))
    rows_gap = max(float(np.abs(r[:, :4] - g[f"pred{i}"][:, :4]).max()) if r.shape[0] == len(g[f"pred{i}"]) else -1.0 for i, (r, _) in enumerate(v.kept))
    print(f"\n[poseval] ours {[round(res[k], 4) for k in KEYS10]}\n reference {[round(float(ref[k]), 4) for k in KEYS10]}"
          f"\n gaps {[round(abs(res[k] - float(ref[k])), 5) for k in KEYS10]} tp {int(tp.sum())}/{int(g['full_tp'].sum())} tp_p {int(tp_p.sum())}/{int(g['full_tp_p'].sum())}"
          f" rows {[len(r) for r, _ in v.kept]} worst box gap {rows_gap:.3e}"
          f" tp rows differing {int((tp != g['full_tp']).any(1).sum()) if tp.shape == g['full_tp'].shape else -1}"
          f" tp_p rows differing {int((tp_p != g['full_tp_p']).any(1).sum()) if tp_p.shape == g['full_tp_p'].shape else -1}")
    assert v.seen == int(g["full_seen"])
    np.testing.assert_array_equal(v.nt_per_class, g["full_nt_per_class"])
    np.testing.assert_array_equal(tp, g["full_tp"])
    np.testing.assert_array_equal(tp_p, g["full_tp_p"])
    for k in KEYS10:
        assert abs(res[k] - float(ref[k])) <= 0.02, (k, res[k], float(ref[k]))
    assert abs(res["fitness"] - (res[KEYS10[4]] + res[KEYS10[9]])) <= 1e-12
    with pytest.raises(NotImplementedError):
        model.val([_batch(g)], save_json=True)
