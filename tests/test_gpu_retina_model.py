"""-m gpu: masks at the original resolution end to end.  yolo11n-seg with synthetic weights:
  * utils.ops.process_mask_native on the 64x96 golden's own prototypes, NMS rows and scaled boxes gives the reference's retina bits
    (tests/golden/retina_ops.npz) under the derived criterion of tests/fp64_mask_native_ref.py;
  * YOLO(...).predict(..., predictor=RetinaMasksPredictor) on images of two original shapes in one batch, and on a tensor source: mask shapes equal the
    original shapes, the bits meet the criterion against the float64 restatement applied to that run's own prototypes, coefficient maps,
    anchor indices and scaled boxes, the boxes equal the retina_masks=False run's, whose masks are byte for byte what ey_process_mask gives;
  * SegmentationValidator(process_mask_native=True) against the reference validator's numbers under the bar of
    tests/test_gpu_segval_model.py for this fixture (0.02 in fp32: the predictions agree to ~1e-3, a few borderline matches may differ)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import fp64_mask_native_ref as f64  # noqa: E402
import retina_synth as rs  # noqa: E402
import seg_synth  # noqa: E402
import synthdata as synth  # noqa: E402
from test_segval_cpu import KEYS10, segval_batch  # noqa: E402


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "retina_ops.npz"))


def _geo(hw, shape):
    from edge_yolo_amd.nn._ops import mask_geometry
    return mask_geometry(hw, shape)


def test_process_mask_native_on_the_model_golden(gold, golden_dir):
    from edge_yolo_amd.utils import ops as uops
    g = np.load(os.path.join(golden_dir, "yolo11n_seg_64x96.npz"))
    det, p = g["det0"], g["p"][0]
    for h, w in rs.MODEL_SHAPES:
        tag = f"model_{h}x{w}"
        boxes = uops.scale_boxes((64, 96), torch.tensor(det[:, :4]).cuda(), (h, w))
        np.testing.assert_allclose(boxes.cpu().numpy(), gold[tag + "_boxes"], rtol=0, atol=1e-4)
        want = rs.unpack(gold[tag + "_bits"], gold[tag + "_shape"])
        got = uops.process_mask_native(torch.tensor(p).cuda(), torch.tensor(det[:, 6:]).cuda(), torch.tensor(gold[tag + "_boxes"]).cuda(), (h, w)).cpu().numpy()
        assert got.shape == want.shape == (len(det), h, w)
        ref = f64.process_mask_native64(p, det[:, 6:], gold[tag + "_boxes"], _geo(p.shape[1:], (h, w)))
        und, tot = f64.check_bits(got, ref, 32)
        decided = np.abs(ref["v"]) > f64.mask_bound(ref, 32)
        np.testing.assert_array_equal(got[decided], want[decided])
        print(f"{tag}: {len(det)} masks, undecided {und} of {tot}")


def _images():
    r = np.random.default_rng(5)
    return [r.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in rs.MODEL_SHAPES]


def _device_outputs(pred, source):
    """One eager device step's own outputs on the host: p, [B, A, nm] coefficients, index, count, boxes (network-input pixels)."""
    im = pred.preprocess(source)
    boxes, count, index, _, p, *mcs = pred._device_step(im)
    torch.cuda.synchronize()
    flat = torch.cat([m.float().flatten(2) for m in mcs], 2).permute(0, 2, 1).cpu().numpy()
    return im, boxes, count, index, p, mcs, flat


@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("source", ["images", "tensor"])
def test_predict_retina_masks_end_to_end(source, half):
    import edge_yolo_amd
    from edge_yolo_amd.engine.predictor import RetinaMasksPredictor
    from edge_yolo_amd.nn import _ops
    from edge_yolo_amd.utils import ops as uops
    model = edge_yolo_amd.YOLO("yolo11n-seg.yaml")
    model.model.load_state_dict(seg_synth.state_dict(model.model.state_dict()))
    src = _images() if source == "images" else synth.synth_images(2, 64, 96, seed=3)
    shapes = rs.MODEL_SHAPES if source == "images" else [(64, 96)] * 2
    kw = dict(conf=0.02, iou=0.7, half=half, device="cuda:0", imgsz=96)
    plain = model.predict(src, **kw)
    # ---- retina_masks=False: byte for byte what ey_process_mask gives on that run's own outputs
    im, boxes, count, index, p, mcs, flat = _device_outputs(model.predictor, src)
    n = count.tolist()
    keep = uops.kept_rows(count, index.shape[1])
    rows = torch.stack([torch.arange(len(n), dtype=torch.int32, device="cuda")[:, None].expand(*index.shape)[keep], index[keep]], 1).contiguous()
    low = _ops.process_mask(p, mcs, rows, boxes[keep][:, :4].contiguous(), im.shape[2] // p.shape[2])
    assert sum(n) >= 5
    off = np.concatenate([[0], np.cumsum(n)])
    for i, r in enumerate(plain):
        assert len(r) == n[i] and tuple(r.masks.shape) == (n[i], *im.shape[2:])
        assert torch.equal(r.masks.data, low[off[i]:off[i + 1]].view(torch.bool))
    # ---- retina_masks=True
    res = model.predict(src, predictor=RetinaMasksPredictor, **kw)
    assert model.predictor.retina_masks is True and len(res) == len(shapes)
    for i, (r, q, shape) in enumerate(zip(res, plain, shapes)):
        assert r.orig_shape == tuple(shape) and len(r) == n[i]
        assert torch.equal(r.boxes.data, q.boxes.data)
        assert r.masks.data.dtype == torch.bool and tuple(r.masks.shape) == (n[i], *shape) and r.masks.orig_shape == tuple(shape)
        idx = index[i, :n[i]].cpu().numpy()
        ref = f64.process_mask_native64(p[i].float().cpu().numpy(), flat[i, idx], r.boxes.xyxy.float().cpu().numpy(), _geo(p.shape[2:], shape))
        und, tot = f64.check_bits(r.masks.data.cpu().numpy().astype(np.uint8), ref, 32)
        print(f"image {i} {shape}: {n[i]} masks, undecided {und} of {tot}, set {int(r.masks.data.sum())}")
        assert bool(r.masks.data.any())
    none = model.predict(src, predictor=RetinaMasksPredictor, **{**kw, "conf": 0.9999})
    assert all(len(r) == 0 and r.masks is None for r in none)


def test_fastsam_still_refuses():
    import edge_yolo_amd
    with pytest.raises(NotImplementedError, match="FastSAM: retina_masks"):
        edge_yolo_amd.FastSAM("FastSAM-s.yaml").predict(torch.zeros(1, 3, 64, 96), retina_masks=True, device="cuda:0")
    with pytest.raises(NotImplementedError, match="RetinaMasksPredictor"):  # the facade keyword of the segment task: unchanged, names the built path
        edge_yolo_amd.YOLO("yolo11n-seg.yaml").predict(torch.zeros(1, 3, 64, 96), retina_masks=True, device="cuda:0")


@pytest.mark.parametrize("overlap", [True, False], ids=["overlap", "stack"])
def test_validator_process_mask_native_vs_reference(gold, golden_dir, overlap):
    from edge_yolo_amd.engine.validator import SegmentationValidator
    from edge_yolo_amd.nn.tasks import SegmentationModel
    g = np.load(os.path.join(golden_dir, "segval_case.npz"))
    m = SegmentationModel("yolo11n-seg.yaml")
    m.load_state_dict(seg_synth.state_dict(m.state_dict()))
    m = m.to("cuda")
    m.fuse()
    m = m.float().eval()

    def fresh():
        batch = segval_batch(g, overlap)
        batch["img"] = synth.synth_images(len(g["ori_shape"]), 128, 160, seed=9)
        return batch

    v = SegmentationValidator(m, overlap_mask=overlap, process_mask_native=True)
    v.keep_outputs = True
    res = dict(v([fresh()]))
    assert all(k.shape == (len(r), 128, 160) and k.max(initial=0) <= 1 for r, k in v.kept)  # masks at the network input's resolution
    tag = f"val_{'overlap' if overlap else 'stack'}"
    ref = dict(zip(list(gold[tag + "_keys"]), gold[tag + "_values"]))
    tp_m = np.concatenate(v.stats["tp_m"])
    print(f"\n[{tag}] ours {[round(res[k], 4) for k in KEYS10]}\n reference {[round(float(ref[k]), 4) for k in KEYS10]} tp_m {int(tp_m.sum())}/{int(gold[tag + '_tp_m'].sum())}")
    for k in (KEYS10[1], KEYS10[2], KEYS10[3], KEYS10[4], KEYS10[6], KEYS10[7], KEYS10[8], KEYS10[9]):  # (the keys tests/test_gpu_segval_model.py holds)
        assert abs(res[k] - float(ref[k])) <= 0.02, (k, res[k], float(ref[k]))
    assert tp_m.any()
    plain = SegmentationValidator(m, overlap_mask=overlap)([fresh()])
    assert plain[KEYS10[2]] == res[KEYS10[2]] and plain != res  # the same boxes, other masks
    if overlap:  # the facade: YOLO.val puts the model on the device and hands the option to the validator
        import edge_yolo_amd
        y = edge_yolo_amd.YOLO("yolo11n-seg.yaml")
        y.model.load_state_dict(seg_synth.state_dict(y.model.state_dict()))
        assert y.val([fresh()], process_mask_native=True) == res and y.validator.process_mask_native is True
