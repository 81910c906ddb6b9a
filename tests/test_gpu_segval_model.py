"""-m gpu: segment validation end to end.  SegmentationValidator on the HIP yolo11n-seg (synthetic weights) over the images and labels of
tests/golden/segval_case.npz:
  * internally consistent, exactly: the validator's own kept rows and predicted mask bits, taken to the host, give the same tp, tp_m and
    results_dict through the numpy route (host mask_iou, matching, AP) as the device route returned;
  * against the numbers the REFERENCE got with its model, NMS, process_mask and validator on the same images and labels, under the bar
    tests/test_gpu_model.py::test_validator_end_to_end_vs_reference uses for this kind of fixture (0.02 in fp32, 0.06 in f16: the
    predictions agree to ~1e-3, so a few borderline matches may differ); the mask keys get the same bar;
  * YOLO.val is the same computation for both tasks."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import seg_synth  # noqa: E402
import synthdata as synth  # noqa: E402
from test_segval_cpu import KEYS10, bits, segval_batch  # noqa: E402


@pytest.fixture(scope="module")
def case(golden_dir):
    return np.load(os.path.join(golden_dir, "segval_case.npz"))


def _model(dtype):
    from edge_yolo_amd.nn.tasks import SegmentationModel
    m = SegmentationModel("yolo11n-seg.yaml")
    m.load_state_dict(seg_synth.state_dict(m.state_dict()))
    m = m.to("cuda")
    m.fuse()
    return (m.half() if dtype == torch.float16 else m.float()).eval()


def _batch(g, overlap):
    b = segval_batch(g, overlap)
    b["img"] = synth.synth_images(len(g["ori_shape"]), 128, 160, seed=9)
    return b


@pytest.mark.parametrize("overlap", [True, False], ids=["overlap", "stack"])
@pytest.mark.parametrize("half,tol", [(False, 0.02), (True, 0.06)], ids=["fp32", "f16"])
def test_validator_consistent_and_vs_reference(case, half, tol, overlap):
    from edge_yolo_amd.engine.validator import SegmentationValidator
    g = case
    tag = f"{'overlap' if overlap else 'stack'}_full"
    m = _model(torch.float16 if half else torch.float32)
    v = SegmentationValidator(m, half=half, overlap_mask=overlap)
    v.keep_outputs = True
    res = dict(v([_batch(g, overlap)]))
    tp, tp_m = np.concatenate(v.stats["tp"]), np.concatenate(v.stats["tp_m"])
    # ---- the same rows and mask bits through the host route: everything equal, exactly
    h = SegmentationValidator(m, half=half, overlap_mask=overlap)
    h.device = torch.device("cpu")
    rows = [r for r, _ in v.kept]
    mh, mw = (int(t) for t in g["mask_shape"])
    assert all(k.dtype == np.uint8 and k.shape == (len(r), mh, mw) and k.max(initial=0) <= 1 for r, k in v.kept)
    h.update_metrics((rows, None), segval_batch(g, overlap), pred_masks=[k for _, k in v.kept])
    hres = h.get_stats()
    np.testing.assert_array_equal(np.concatenate(h.stats["tp"]), tp)
    np.testing.assert_array_equal(np.concatenate(h.stats["tp_m"]), tp_m)
    assert hres == res
    assert tp_m.any()
    # ---- against the reference's own validation of the same images and labels
    ref = dict(zip(list(g[tag + "_keys"]), g[tag + "_values"]))
    print(f"\n[segval half={half} {tag}] ours {[round(res[k], 4) for k in KEYS10]}\n reference {[round(float(ref[k]), 4) for k in KEYS10]}"
          f"\n gaps {[round(abs(res[k] - float(ref[k])), 4) for k in KEYS10]} tp {int(tp.sum())}/{int(g[tag + '_tp'].sum())} tp_m {int(tp_m.sum())}/{int(g[tag + '_tp_m'].sum())}")
    if not half:  # how many predicted mask pixels differ from the reference's, where the rows line up
        same = [i for i, (r, _) in enumerate(v.kept) if r.shape == g[f"pred{i}"].shape and np.allclose(r[:, :6], g[f"pred{i}"][:, :6], atol=1e-2)]
        diff = sum(int((v.kept[i][1].reshape(len(v.kept[i][0]), -1) != bits(g[f"pmask{i}"], mh * mw)).sum()) for i in same)
        print(f" images with aligned rows {same}: {diff} mask pixels differ from the reference's")
    assert v.seen == int(g[tag + "_seen"])
    np.testing.assert_array_equal(v.nt_per_class, g[tag + "_nt_per_class"])
    for k in (KEYS10[1], KEYS10[2], KEYS10[3], KEYS10[4], KEYS10[6], KEYS10[7], KEYS10[8], KEYS10[9]):
        assert abs(res[k] - float(ref[k])) <= tol, (k, res[k], float(ref[k]))
    assert abs(res["fitness"] - (res[KEYS10[4]] + res[KEYS10[9]])) <= 1e-12


def test_ground_truth_of_another_resolution(case):
    """Masks at the network-input resolution (4x the predicted masks') take the reference's resize (bilinear, > 0.5) on the device first;
    nearest-repeated 4x4 blocks come back as the original low-resolution masks, so the statistics equal the direct run's."""
    from edge_yolo_amd.engine.validator import SegmentationValidator
    g = case
    m = _model(torch.float32)
    for overlap in (True, False):
        a = SegmentationValidator(m, overlap_mask=overlap)
        a([_batch(g, overlap)])
        big = _batch(g, overlap)
        big["masks"] = np.repeat(np.repeat(big["masks"], 4, axis=1), 4, axis=2)
        b = SegmentationValidator(m, overlap_mask=overlap)
        b([big])
        np.testing.assert_array_equal(np.concatenate(b.stats["tp_m"]), np.concatenate(a.stats["tp_m"]))
        assert b.results_dict == a.results_dict


def test_facade_val(case):
    import edge_yolo_amd
    from edge_yolo_amd.engine.validator import DetectionValidator, SegmentationValidator
    g = case
    y = edge_yolo_amd.YOLO("yolo11n-seg.yaml")
    y.model.load_state_dict(seg_synth.state_dict(y.model.state_dict()))
    for overlap in (True, False):
        got = y.val([_batch(g, overlap)], overlap_mask=overlap)
        want = SegmentationValidator(_model(torch.float32), overlap_mask=overlap)([_batch(g, overlap)])
        assert got == want and list(got) == KEYS10 + ["fitness"] and got[KEYS10[7]] > 0
    with pytest.raises(NotImplementedError):
        y.val([_batch(g, True)], save_json=True)
    # the detect task: a thin door to DetectionValidator
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "validator_case.npz"))
    batch = {"img": synth.synth_images(len(d["ori_shape"]), 128, 160, seed=9), "cls": d["cls"], "bboxes": d["bboxes"], "batch_idx": d["batch_idx"],
             "ori_shape": [tuple(s) for s in d["ori_shape"]],
             "ratio_pad": [((float(a), float(a)), (int(p[0]), int(p[1]))) for a, p in zip(d["ratio_gain"], d["ratio_padwh"])]}
    yd = edge_yolo_amd.YOLO("yolo11n-test.yaml")
    yd.model.load_state_dict(synth.synth_state_dict({k: tuple(t.shape) for k, t in yd.model.state_dict().items()}))
    got = yd.val([batch], half=True)
    m = yd.model  # (val left it on the device, fused, in f16)
    want = DetectionValidator(m, half=True)([batch])
    assert got == want and got["metrics/mAP50(B)"] > 0
