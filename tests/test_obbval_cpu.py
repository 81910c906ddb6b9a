"""obb validation without a GPU: the float64 restatement of multi-label rotated NMS (tests/fp64_obbval_ref.py) against the reference's kept
lists and rows (tests/golden/obbval_ops.npz), OBBValidator on host arrays against the reference's own OBBValidator / OBBMetrics
(obbval_case.npz: the true-positive matrix exactly, the metrics to 1e-12), metrics.probiou_host against the reference's matrices, and the
public surface: OBBMetrics.keys, the refusals that name the new paths, the unchanged task tables."""
import ctypes
import os

import numpy as np
import pytest
import torch

import fp64_obb_ref as f64
import fp64_obbval_ref as f64v
import obbval_synth as S


@pytest.fixture(scope="module")
def ops_g(golden_dir):
    return np.load(os.path.join(golden_dir, "obbval_ops.npz"))


@pytest.fixture(scope="module")
def case_g(golden_dir):
    return np.load(os.path.join(golden_dir, "obbval_case.npz"))


@pytest.mark.parametrize("case", S.NMS_CASES, ids=[c["tag"] for c in S.NMS_CASES])
def test_oracle_against_the_reference(ops_g, case):
    tag = case["tag"]
    pred = S.nms_case(case, int(ops_g[tag + "_seed"])).numpy()
    assert f64v.distinct_scores(pred, case["conf"])
    ora = f64v.nms_rotated_ml64(pred, case["conf"], case["iou"], case["classes"], case["agnostic"], case["max_det"], case["max_nms"], S.MAX_WH)
    worst = min([float(o["margin"].min()) for o in ora if len(o["margin"])] or [1.0])
    assert worst > S.MARGIN and abs(worst - float(ops_g[tag + "_margin"])) < 1e-12
    for b, o in enumerate(ora):
        kept = ops_g[f"{tag}_kept{b}"]
        assert o["total"] == int(ops_g[f"{tag}_total{b}"]) and len(o["anchor"]) == min(o["total"], case["max_nms"])
        np.testing.assert_array_equal(o["anchor"][o["keep"]], kept[:, 0])
        np.testing.assert_array_equal(o["cls"][o["keep"]], kept[:, 1])
        np.testing.assert_array_equal(o["rows"], ops_g[f"{tag}_rows{b}"])
    if tag == "ml_cut":  # the cut falls inside an anchor's classes: the last survivor's anchor has a class beyond it
        beyond = f64v.candidates_ml(pred[0], case["nc"], case["conf"], None, case["A"] * case["nc"])[0][case["max_nms"]:]
        assert ora[0]["anchor"][-1] in beyond


def test_probiou_host_against_the_reference(ops_g):
    from edge_yolo_amd.utils import metrics
    pred, gt, poff, goff = S.pair_case()
    for b, (n, m) in enumerate(S.PAIR_SIZES):
        p, g = pred[poff[b]:poff[b + 1]], gt[goff[b]:goff[b + 1]]
        got = metrics.probiou_host(g, torch.tensor(p))
        assert got.shape == (m, n) and got.dtype == np.float32
        if n * m:
            ref32, ref64 = ops_g[f"pb_{b}"].astype(np.float64), f64.probiou64(g, p)
            E = float(np.abs(ref32 - ref64).max())
            assert (np.abs(got.astype(np.float64) - ref64) <= f64.bound(E, ref64)).all()


def _batch(g):
    B, H, W = (int(v) for v in g["image_shape"])
    return {"img": torch.zeros(B, 3, H, W), "cls": g["cls"], "bboxes": g["bboxes"], "batch_idx": g["batch_idx"],
            "ori_shape": [tuple(int(v) for v in s) for s in g["ori_shape"]],
            "ratio_pad": [((float(gn), float(gn)), (float(p[0]), float(p[1]))) for gn, p in zip(g["ratio_gain"], g["ratio_padwh"])]}


@pytest.fixture(scope="module")
def obb_model():
    from edge_yolo_amd.nn.tasks import OBBModel
    return OBBModel("yolo11n-obb.yaml")


@pytest.mark.parametrize("variant", ["full", "nopred"])
def test_validator_on_host_rows_against_the_reference(case_g, obb_model, variant):
    from edge_yolo_amd.engine.validator import OBBValidator
    g = case_g
    assert float(g["margin"]) > S.IOU_MARGIN
    B = int(g["image_shape"][0])
    labels_per_image = [int((g["batch_idx"] == i).sum()) for i in range(B)]
    assert 0 in labels_per_image and labels_per_image[int(g["empty_pred_image"])] > 0  # an image without labels, and labels without predictions
    v = OBBValidator(obb_model, device="cpu")
    preds = [g[f"pred{i}"] if not (variant == "nopred" and i == int(g["empty_pred_image"])) else g[f"pred{i}"][:0] for i in range(B)]
    before = g["bboxes"].copy()
    v.update_metrics(preds, _batch(g))
    np.testing.assert_array_equal(g["bboxes"], before)  # the labels are not rewritten
    res = v.get_stats()
    np.testing.assert_array_equal(np.concatenate(v.stats["tp"], 0), g[variant + "_tp"])
    np.testing.assert_array_equal(np.concatenate(v.stats["conf"], 0), g[variant + "_conf"])
    assert v.seen == int(g[variant + "_seen"])
    np.testing.assert_array_equal(v.nt_per_class, g[variant + "_nt_per_class"])
    np.testing.assert_allclose(v.box.all_ap, g[variant + "_ap"], rtol=0, atol=1e-12)
    np.testing.assert_array_equal(v.box.ap_class_index, g[variant + "_ap_class_index"])
    ref, means = dict(zip(g[variant + "_keys"], g[variant + "_values"])), g[variant + "_means"]
    assert list(res) == list(g[variant + "_keys"]) == ["metrics/precision(B)", "metrics/recall(B)", "metrics/mAP50(B)", "metrics/mAP50-95(B)", "fitness"]
    np.testing.assert_allclose(v.metrics.mean_results(), means, rtol=0, atol=1e-12)
    for k in ("metrics/precision(B)", "metrics/recall(B)", "metrics/mAP50(B)", "fitness"):
        assert abs(res[k] - ref[k]) < 1e-12, k
    # the reference zips four keys with the fork's five means, which files mAP75 under "mAP50-95"; here the key holds what it names
    assert ref["metrics/mAP50-95(B)"] == means[3] and ref["fitness"] == means[4]
    assert abs(res["metrics/mAP50-95(B)"] - means[4]) < 1e-12


def test_validator_options_and_single_cls(case_g, obb_model):
    from edge_yolo_amd.engine.validator import OBBValidator
    for kw in ("save_json", "save_txt", "plots"):
        with pytest.raises(NotImplementedError, match=kw):
            OBBValidator(obb_model, device="cpu", **{kw: True})
    g = case_g
    v = OBBValidator(obb_model, device="cpu", single_cls=True)
    batch = _batch(g)
    batch["cls"] = np.zeros_like(g["cls"])
    v.update_metrics([g[f"pred{i}"] for i in range(int(g["image_shape"][0]))], batch)
    assert (np.concatenate(v.stats["pred_cls"]) == 0).all() and set(v.get_stats()) == set(v.metrics.keys + ["fitness"])
    empty = OBBValidator(obb_model, device="cpu")
    assert empty.get_stats() == dict.fromkeys(empty.metrics.keys + ["fitness"], 0.0)
    with pytest.raises(NotImplementedError):
        empty.update(torch.zeros(1, 3, 32, 32), [[]])


def test_public_surface():
    import edge_yolo_amd
    from edge_yolo_amd.engine import model as emodel
    from edge_yolo_amd.engine.validator import DetectionValidator, OBBValidator
    from edge_yolo_amd.utils import metrics
    from edge_yolo_amd.utils import ops as uops
    assert metrics.OBBMetrics().keys == ["metrics/precision(B)", "metrics/recall(B)", "metrics/mAP50(B)", "metrics/mAP50-95(B)"]
    assert set(metrics.OBBMetrics().results_dict) == set(metrics.OBBMetrics().keys + ["fitness"])
    assert issubclass(OBBValidator, DetectionValidator) and emodel.OBBValidator is OBBValidator
    y = edge_yolo_amd.YOLO("yolo11n-obb.yaml")
    assert set(y.task_map) == {"detect", "segment"} and "validator" not in y._task_entry()
    with pytest.raises(NotImplementedError, match=r"validator=OBBValidator"):
        y.val([{"img": torch.zeros(1, 3, 64, 64)}])
    for f in (uops.non_max_suppression, uops.nms_device):
        with pytest.raises(NotImplementedError, match="nms_rotated_multi_label"):
            f(torch.zeros(1, 8, 10), nc=3, multi_label=True, rotated=True)
    with pytest.raises(NotImplementedError, match="nc="):
        uops.nms_rotated_multi_label(torch.zeros(1, 8, 10))
    with pytest.raises(ValueError):
        uops.nms_rotated_multi_label(torch.zeros(1, 8, 10), nc=5)


def test_c_abi_argument_checks():
    from edge_yolo_amd import _lib as L
    lib = L.lib()
    assert lib.ey_nms_rotated_ml_workspace_bytes(2, 3, 64, 100) % 256 == 0 and lib.ey_nms_rotated_ml_workspace_bytes(2, 3, 64, 100) > 0
    assert lib.ey_nms_rotated_ml_workspace_bytes(0, 3, 64, 100) == 0 and lib.ey_nms_rotated_ml_workspace_bytes(1, 1 << 16, 1 << 16, 100) == 0
    # more survivors cost more workspace, up to A * nc of them
    assert lib.ey_nms_rotated_ml_workspace_bytes(1, 3, 64, 100) < lib.ey_nms_rotated_ml_workspace_bytes(1, 3, 64, 192) == lib.ey_nms_rotated_ml_workspace_bytes(1, 3, 64, 30000)
    assert lib.ey_nms_rotated_ml(1, 3, 64, None, 0.25, 0.45, 300, 100, 7680.0, 0, None, None, None, None, None, 0, None) != 0  # null pointers
    assert lib.ey_probiou_batch(0, None, None, None, None, None, None, None) == 0  # B == 0 is valid
    off = (ctypes.c_int * 2)(0, 0)
    assert lib.ey_probiou_batch(1, None, off, None, off, None, (ctypes.c_long * 1)(0), None) == 0  # no pair anywhere: nothing to launch
