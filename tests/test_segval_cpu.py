"""CPU checks of segment validation: the host form of metrics.mask_iou and of the overlap_mask expansion against the reference's own values
(tests/golden/segval_ops.npz, bit for bit), SegmentationValidator / SegmentMetrics on the reference's predictions, mask bits and labels
against the reference's own validator (tests/golden/segval_case.npz), the facade, and the host side of ey_mask_iou."""
import ctypes
import os

import numpy as np
import pytest
import torch

import edge_yolo_amd
from edge_yolo_amd import _lib as L
from edge_yolo_amd.engine.validator import DetectionValidator, SegmentationValidator
from edge_yolo_amd.nn.tasks import SegmentationModel
from edge_yolo_amd.utils import metrics

KEYS10 = ["metrics/precision(B)", "metrics/recall(B)", "metrics/mAP50(B)", "metrics/mAP75(B)", "metrics/mAP50-95(B)",
          "metrics/precision(M)", "metrics/recall(M)", "metrics/mAP50(M)", "metrics/mAP75(M)", "metrics/mAP50-95(M)"]


@pytest.fixture(scope="module")
def seg_ops(golden_dir):
    return np.load(os.path.join(golden_dir, "segval_ops.npz"))


@pytest.fixture(scope="module")
def case(golden_dir):
    return np.load(os.path.join(golden_dir, "segval_case.npz"))


@pytest.fixture(scope="module")
def seg_model():
    return SegmentationModel("yolo11n-seg.yaml")


def bits(packed, n):
    return np.unpackbits(packed, axis=1)[:, :n]


def test_host_mask_iou_equals_the_reference_bits(seg_ops):
    seen = set()
    for tag in seg_ops["iou_tags"]:
        n = int(seg_ops[f"iou_{tag}_n"])
        g, p = bits(seg_ops[f"iou_{tag}_gt"], n), bits(seg_ops[f"iou_{tag}_pred"], n)
        want = seg_ops[f"iou_{tag}"]
        for a, b in ((g, p), (torch.tensor(g, dtype=torch.float32), torch.tensor(p, dtype=torch.float32))):  # host arrays and CPU tensors
            got = metrics.mask_iou(a, b)
            assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.shape == want.shape
            np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32), err_msg=str(tag))
        inter = g.astype(np.int64) @ p.T.astype(np.int64)
        union = g.sum(1)[:, None] + p.sum(1)[None] - inter
        seen |= {int(u) for u in np.unique(union) if u <= 1}
        assert (want[union == 0] == 0).all()  # 0 / 1e-7 is exactly 0
        one = (union == 1) & (inter == 1)
        if one.any():  # the + 1e-7f moves the last bit: 1 / fl(1 + 1e-7f) < 1
            assert (want[one] < 1).all() and (want[one] == np.float32(1) / (np.float32(1) + np.float32(1e-7))).all()
    assert seen == {0, 1}, "the fixture must hold unions of 0 and of 1"


def test_host_index_map_expansion_equals_the_reference(seg_ops):
    for tag in seg_ops["ex_tags"]:
        m, nl = seg_ops[f"ex_{tag}_map"], int(seg_ops[f"ex_{tag}_nl"])
        got = metrics.expand_index_masks(m, nl)
        assert got.shape == (nl,) + m.shape and got.dtype == np.uint8
        np.testing.assert_array_equal(got.reshape(nl, -1), bits(seg_ops[f"ex_{tag}"], m.size))
    assert int(seg_ops["ex_wide_nl"]) > 255 and (metrics.expand_index_masks(seg_ops["ex_small_map"], 6).reshape(6, -1).sum(1) == 0).any()


def segval_batch(g, overlap, masks_as=np.asarray):
    """The fixture's labels in the collate format; masks: the index maps (B,h,w) or the per-label stack (M,h,w)."""
    mh, mw = (int(v) for v in g["mask_shape"])
    B = len(g["ori_shape"])
    masks = g["gt_index"] if overlap else bits(g["gt_stack"], mh * mw).reshape(-1, mh, mw)
    return {"img": torch.zeros(B, 3, 128, 160), "cls": g["cls"], "bboxes": g["bboxes"], "batch_idx": g["batch_idx"], "masks": masks_as(masks),
            "ori_shape": [tuple(s) for s in g["ori_shape"]],
            "ratio_pad": [((float(a), float(a)), (int(p[0]), int(p[1]))) for a, p in zip(g["ratio_gain"], g["ratio_padwh"])]}


@pytest.mark.parametrize("variant", ["full", "nopred"])
@pytest.mark.parametrize("overlap", [True, False], ids=["overlap", "stack"])
def test_validator_on_reference_predictions(case, seg_model, overlap, variant):
    """Rows, predicted mask bits and labels of the reference -> the reference's tp, tp_m, AP and results_dict.  `nopred` drops the
    predictions of one labelled image (npr == 0 bookkeeping); image 1 has no labels in both."""
    g = case
    tag = f"{'overlap' if overlap else 'stack'}_{variant}"
    mh, mw = (int(v) for v in g["mask_shape"])
    B = len(g["ori_shape"])
    drop = int(g["empty_pred_image"]) if variant == "nopred" else -1
    rows = [g[f"pred{i}"] if i != drop else g[f"pred{i}"][:0] for i in range(B)]
    pmasks = [bits(g[f"pmask{i}"], mh * mw).reshape(-1, mh, mw)[:len(rows[i])] for i in range(B)]
    v = SegmentationValidator(seg_model, overlap_mask=overlap)
    assert v.device.type == "cpu"
    v.update_metrics((rows, None), segval_batch(g, overlap), pred_masks=pmasks)
    res = v.get_stats()
    np.testing.assert_array_equal(np.concatenate(v.stats["tp"]), g[tag + "_tp"])
    np.testing.assert_array_equal(np.concatenate(v.stats["tp_m"]), g[tag + "_tp_m"])
    assert g[tag + "_tp_m"].any() and not np.array_equal(g[tag + "_tp"], g[tag + "_tp_m"])
    assert v.seen == int(g[tag + "_seen"]) == B
    np.testing.assert_array_equal(v.nt_per_class, g[tag + "_nt_per_class"])
    np.testing.assert_allclose(v.metrics.box.all_ap, g[tag + "_ap_box"], rtol=0, atol=1e-9)
    np.testing.assert_allclose(v.metrics.seg.all_ap, g[tag + "_ap_mask"], rtol=0, atol=1e-9)
    np.testing.assert_array_equal(v.metrics.box.ap_class_index, g[tag + "_ap_class_index"])
    assert list(res) == list(g[tag + "_keys"]) == KEYS10 + ["fitness"]
    for k, want in zip(g[tag + "_keys"], g[tag + "_values"]):
        assert abs(res[k] - float(want)) <= 1e-9, (k, res[k], float(want))
    assert abs(res["fitness"] - (res[KEYS10[4]] + res[KEYS10[9]])) <= 1e-12


def test_validator_host_masks_as_cpu_tensors_and_single_cls(case, seg_model):
    """CPU tensors take the same route as arrays; single_cls zeroes the predicted classes before matching."""
    g = case
    mh, mw = (int(v) for v in g["mask_shape"])
    B = len(g["ori_shape"])
    rows = [g[f"pred{i}"] for i in range(B)]
    pmasks = [torch.tensor(bits(g[f"pmask{i}"], mh * mw).reshape(-1, mh, mw)) for i in range(B)]
    v = SegmentationValidator(seg_model, overlap_mask=False)
    v.update_metrics((rows, None), segval_batch(g, False, torch.tensor), pred_masks=pmasks)
    np.testing.assert_array_equal(np.concatenate(v.stats["tp_m"]), g["stack_full_tp_m"])
    s = SegmentationValidator(seg_model, overlap_mask=False, single_cls=True)
    s.update_metrics((rows, None), segval_batch(g, False), pred_masks=pmasks)
    assert (np.concatenate(s.stats["pred_cls"]) == 0).all()


def test_facade_and_keys():
    assert metrics.SegmentMetrics().keys == KEYS10
    assert list(metrics.SegmentMetrics().results_dict) == KEYS10 + ["fitness"] and set(metrics.SegmentMetrics().results_dict.values()) == {0.0}
    y = edge_yolo_amd.YOLO("yolo11n-seg.yaml")
    assert set(y.task_map) == {"detect", "segment"}
    assert y.task_map["segment"]["validator"] is SegmentationValidator and y.task_map["detect"]["validator"] is DetectionValidator
    assert issubclass(SegmentationValidator, DetectionValidator) and callable(y.val)
    for kw in ("save_json", "save_txt", "plots", "process_mask_native"):
        with pytest.raises(NotImplementedError):
            SegmentationValidator(y.model, **{kw: True})
    v = SegmentationValidator(y)  # a facade is accepted like DetectionValidator accepts one
    assert v.overlap_mask and v.conf == 0.001 and list(v.results_dict) == KEYS10 + ["fitness"]
    with pytest.raises(TypeError):
        y.val([], nonsense=1)
    with pytest.raises(TypeError):  # overlap_mask belongs to the segment task
        edge_yolo_amd.YOLO("yolo11n-test.yaml").val([], overlap_mask=True)


def test_mask_iou_symbols_and_host_side_refusals():
    """Both entries are exported; the argument checks that run before any launch answer on a host without a GPU."""
    lib = L.lib()
    for name in ("ey_mask_iou", "ey_mask_iou_workspace_bytes"):
        assert hasattr(lib, name)
    # 64-pixel words, four per block of 256 pixels: 8 bytes x 4 ceil(HW / 256) per mask, rounded up to 16 bytes
    assert lib.ey_mask_iou_workspace_bytes(8, 8, 3, 2) == 5 * 4 * 8 and lib.ey_mask_iou_workspace_bytes(17, 16, 1, 0) == 2 * 4 * 8
    assert lib.ey_mask_iou_workspace_bytes(160, 160, 300, 20) == 320 * 400 * 8
    assert lib.ey_mask_iou_workspace_bytes(0, 8, 1, 1) == 0
    IA, LA = ctypes.c_int * 3, ctypes.c_long * 2
    po, go, oo = IA(0, 2, 5), IA(0, 1, 3), LA(0, 2)

    def call(mode=L.MASK_GT_STACK, B=2, H=4, W=4, pred=8, po=po, gt=8, go=go, oo=oo, iou=8, ws=16, nbytes=1 << 20):
        return lib.ey_mask_iou(mode, B, H, W, pred, po, gt, go, oo, iou, None, ws, nbytes, None)

    assert call(mode=2) == -1
    assert call(H=0) == -1 and call(B=-1) == -1
    assert call(B=129) == -2  # more images than the offset tables hold
    assert call(H=4097, W=4097) == -2  # areas would not be exact in fp32
    assert call(po=None) == -1 and call(oo=None) == -1
    assert call(po=IA(1, 2, 5)) == -1 and call(go=IA(0, 2, 1)) == -1  # offsets start at 0 and never decrease
    assert call(oo=LA(0, -4)) == -1
    assert call(pred=None) == -1 and call(gt=None) == -1 and call(iou=None) == -1 and call(ws=None) == -1
    assert call(ws=24) == -1  # workspace alignment
    assert call(nbytes=8 * 4 * 8 - 16) == -1  # workspace too small: (5 + 3) masks x 4 words
    assert call(mode=L.MASK_GT_INDEX, gt=6) == -1  # the index map is int32
    # nothing to do is valid and launches nothing: no images, or no image with both predictions and ground truth
    assert call(B=0, po=None, go=None, oo=None, pred=None, gt=None, iou=None, ws=None) == 0
    assert call(po=IA(0, 0, 3), go=IA(0, 2, 2), pred=None, gt=None, iou=None, ws=None) == 0
