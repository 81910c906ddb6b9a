"""The pieces every task's predictor, validator and the facade share, on CPU tensors (no launch is made): the kept-rows mask, the offset
tables and slicing of a batch's [gt x pred] matrices, the facade's keyword table, the augment policy, and the tensor-source `orig_shape`
through the one result-assembly path."""
import warnings

import numpy as np
import pytest
import torch

import edge_yolo_amd  # noqa: F401
from edge_yolo_amd.engine import predictor as P
from edge_yolo_amd.engine.model import Model
from edge_yolo_amd.engine.validator import batch_offsets, pair_matrices
from edge_yolo_amd.utils import ops

CPU = torch.device("cpu")


class _Stub:
    names = {0: "a", 1: "b", 2: "c"}


def test_kept_rows_mask():
    max_det = 4
    keep = ops.kept_rows(torch.tensor([0, 1, max_det], dtype=torch.int32), max_det)
    assert keep.dtype == torch.bool and keep.tolist() == [[False] * 4, [True, False, False, False], [True] * 4]
    assert tuple(ops.kept_rows(torch.zeros(0, dtype=torch.int32), max_det).shape) == (0, max_det)


def test_pair_matrices_against_slicing_by_hand():
    n, nl = [0, 3, 2], [2, 0, 3]  # an image without predictions, one without labels, one with both
    assert batch_offsets(n).tolist() == [0, 0, 3, 5] and batch_offsets(nl).tolist() == [0, 2, 2, 5]
    flat = torch.arange(100, 106, dtype=torch.float32)  # image 2's row-major (3, 2) matrix; the others hold nothing
    seen = []

    def launch(pred_off, gt_off):
        seen.append((list(pred_off), list(gt_off)))
        return flat, [0, 0, 0]

    out = pair_matrices(launch, n, nl)
    assert seen == [([0, 0, 3, 5], [0, 2, 2, 5])]  # one launch, with both tables
    assert out[0] is None and out[1] is None
    np.testing.assert_array_equal(out[2], np.array([[100, 101], [102, 103], [104, 105]], np.float32))
    # matrices packed one after the other: each image's slice starts at its own offset
    n, nl = [2, 0, 1], [1, 4, 2]
    flat = torch.arange(4, dtype=torch.float32)
    out = pair_matrices(lambda po, go: (flat, [0, 2, 2]), n, nl)
    np.testing.assert_array_equal(out[0], np.array([[0, 1]], np.float32))
    assert out[1] is None
    np.testing.assert_array_equal(out[2], np.array([[2], [3]], np.float32))


def test_keyword_table():
    defaults = {"conf": 0.25, "half": False}
    got = Model._options("predict", defaults, {"conf": 0.5, "verbose": True, "imgsz": 96}, {"imgsz", "verbose"})
    assert got == {"conf": 0.5, "half": False} and defaults == {"conf": 0.25, "half": False}  # ignored names accepted and dropped
    with pytest.raises(TypeError) as e:
        Model._options("val", defaults, {"zeta": 1, "conf": 0.1, "alpha": 2}, {"imgsz"})
    assert str(e.value) == "val() got unsupported arguments ['alpha', 'zeta']"


@pytest.mark.parametrize("cls, name", [(P.SegmentationPredictor, "SegmentationModel"), (P.FastSAMPredictor, "SegmentationModel"), (P.OBBPredictor, "OBBModel"),
                                       (P.PosePredictor, "PoseModel")])
def test_augment_policy_warns_and_reverts(cls, name):
    with pytest.warns(UserWarning) as w:
        p = cls(_Stub(), CPU, graph=False, augment=True)
    assert [str(m.message) for m in w] == [f"{name} does not support 'augment=True', reverting to single-scale prediction."]
    assert p.augment is False
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert cls(_Stub(), CPU, graph=False).augment is False


def test_augment_policy_detect_runs_and_classify_refuses():
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert P.DetectionPredictor(_Stub(), CPU, graph=False, augment=True).augment is True
        assert P.ClassificationPredictor(_Stub(), CPU, graph=False).augment is False
    with pytest.raises(NotImplementedError) as e:
        P.ClassificationPredictor(_Stub(), CPU, graph=False, augment=True)
    assert str(e.value) == "ClassificationPredictor: augment=True (test-time augmentation) is not built for the classify task"


def _rows(B, max_det, width):
    g = torch.Generator().manual_seed(B * 100 + width)
    rows = torch.rand((B, max_det, width), generator=g) * 40
    rows[..., 2:4] += rows[..., :2]
    return rows


@pytest.mark.parametrize("field", ["boxes", "keypoints", "obb", "probs"])
def test_tensor_source_orig_shape_is_the_network_input(field):
    B, max_det, inp = 2, 5, (64, 96)
    img, count = torch.zeros(B, 3, *inp), torch.tensor([3, 0], dtype=torch.int32)
    cls = {"boxes": P.DetectionPredictor, "keypoints": P.PosePredictor, "obb": P.OBBPredictor, "probs": P.ClassificationPredictor}[field]
    p = cls(_Stub(), CPU, graph=False)
    p._orig = None  # a tensor source
    if field == "boxes":
        res = p.postprocess(_rows(B, max_det, 6), count, img, None)
    elif field == "keypoints":
        res = p.postprocess(_rows(B, max_det, 6), count, img, None, kpts=torch.rand(B, max_det, 17, 3))
    elif field == "obb":
        res = p.postprocess(_rows(B, max_det, 7), count, img, None)
    else:
        res = p.postprocess(torch.softmax(torch.rand(B, 3), 1), img, None)
    assert len(res) == B
    for i, r in enumerate(res):
        assert r.orig_img is None and r.path == f"image{i}.jpg" and r.names is _Stub.names
        assert r.orig_shape == inp and getattr(r, field).orig_shape == inp
        assert [k for k in ("boxes", "masks", "keypoints", "obb", "probs") if getattr(r, k) is not None] == (["boxes", "keypoints"] if field == "keypoints" else [field])
        if field != "probs":
            assert len(r) == int(count[i])
