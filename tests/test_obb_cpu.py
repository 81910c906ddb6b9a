"""CPU checks of the obb task: the float64 restatements (tests/fp64_obb_ref.py) against the reference's own results (tests/golden/obb_ops.npz,
yolo11n_obb_64x96.npz), registry / structure / state_dict keys of yolo11{n,s,m,l,x}-obb.yaml against what the reference builds
(structure_obb.json), guess_model_task, the tensor utilities and the Results.obb container on CPU tensors, and the refusals."""
import json
import os

import numpy as np
import pytest
import torch

import edge_yolo_amd
from edge_yolo_amd.engine.results import OBB, Results
from edge_yolo_amd.nn import modules as M
from edge_yolo_amd.nn.tasks import DetectionModel, OBBModel, guess_model_task, yaml_model_load
from edge_yolo_amd.utils import ops as uops
import fp64_obb_ref as f64
import obb_synth


@pytest.fixture(scope="module")
def structure(golden_dir):
    return json.load(open(os.path.join(golden_dir, "structure_obb.json")))


@pytest.fixture(scope="module")
def obb_ops(golden_dir):
    return np.load(os.path.join(golden_dir, "obb_ops.npz"))


@pytest.fixture(scope="module")
def model_golden(golden_dir):
    return np.load(os.path.join(golden_dir, "yolo11n_obb_64x96.npz"))


# ---- the float64 restatements reproduce the reference
@pytest.mark.parametrize("case", obb_synth.DECODE_CASES, ids=[c[0] for c in obb_synth.DECODE_CASES])
def test_decode64_reproduces_the_reference(obb_ops, case):
    tag, _, strides, nc = case[:4]
    ref = obb_ops[tag + "_y"].astype(np.float64)
    got = f64.decode64([tuple(t.numpy() for t in lv) for lv in obb_synth.decode_case(*case)], strides)
    assert got.shape == ref.shape
    # fp32 rounding of the reference: a few ulp of the largest term (coordinates up to ~16 bins * stride 32)
    np.testing.assert_allclose(got[:, :4], ref[:, :4], rtol=2e-6, atol=2e-4)
    np.testing.assert_allclose(got[:, 4:], ref[:, 4:], rtol=0, atol=1e-6)


@pytest.mark.parametrize("tag", obb_synth.PROBIOU_CASES)
def test_probiou64_reproduces_the_reference(obb_ops, tag):
    o1, o2 = obb_synth.probiou_case(tag)
    ref, got = obb_ops[tag].astype(np.float64), f64.probiou64(o1, o2)
    assert ref.shape == got.shape == (len(o1), len(o2))
    err = np.abs(ref - got)
    # near IoU = 1 the tail sqrt(1 - exp(-bd) + eps) amplifies the fp32 rounding of bd ~ eps to ~2e-5 (up to 2e-4 where the log term cancels
    # against a large t1); elsewhere the reference is within a few 1e-6
    assert err.max() < 5e-4 and np.median(err) < 2e-6, (err.max(), np.median(err))
    if tag == "pi_identical":
        assert np.all(np.diag(got) > 0.999)
    if tag == "pi_rot_pi":  # the same Gaussian: rotation by pi, and by pi/2 with the sides swapped
        assert np.all(got[np.arange(3), np.arange(3)] > 0.99) and np.all(got[np.arange(3), 3 + np.arange(3)] > 0.99)


def _oracle(case, seed):
    pred = obb_synth.nms_case(case, seed).numpy()
    return pred, f64.nms_rotated64(pred, case["conf"], case["iou"], case["classes"], case["agnostic"], case["max_det"], case["max_nms"], obb_synth.MAX_WH)


@pytest.mark.parametrize("case", obb_synth.NMS_CASES, ids=[c["tag"] for c in obb_synth.NMS_CASES])
def test_fast_nms64_reproduces_the_reference(obb_ops, case):
    tag = case["tag"]
    pred, ora = _oracle(case, int(obb_ops[tag + "_seed"]))
    tau = 4.0 * float(obb_ops[tag + "_E"]) + 2.0 * 2.0 ** -24
    for b, o in enumerate(ora):
        assert len(o["order"]) == min(case["counts"][b], case["max_nms"]) or case["classes"] is not None
        np.testing.assert_array_equal(o["margin"], obb_ops[f"{tag}_margin{b}"])
        if case["exact"]:
            assert not len(o["margin"]) or o["margin"].min() > 1e-3
            np.testing.assert_array_equal(o["rows"], obb_ops[f"{tag}_rows{b}"])
        if case["special"] == "ties":  # (the reference's argsort leaves the order of equal scores unspecified: its flags belong to another order)
            continue
        decided = o["margin"] > tau
        ref_keep = np.isin(o["order"], obb_ops[f"{tag}_kept{b}"])
        np.testing.assert_array_equal(ref_keep[decided], o["keep"][decided])


def test_fast_nms64_on_the_model_golden(model_golden):
    g = model_golden
    o = f64.nms_rotated64(g["y"], float(g["conf"]), 0.7)[0]
    np.testing.assert_array_equal(o["rows"], g["det0"])
    np.testing.assert_array_equal(o["margin"], g["margin0"])
    assert len(g["det0"]) >= 5 and g["margin0"].min() > 1e-3


def test_fast_nms64_semantics():
    """the keep rule on hand-made columns: a suppressed box still suppresses (fast-NMS), iou_thres = 0 keeps nothing."""
    box = np.array([[100, 100, 60, 20, 0.2], [101, 100, 60, 20, 0.2], [300, 300, 40, 40, 0.0], [102, 100, 60, 20, 0.2]], np.float32)
    pred = np.zeros((1, 6, 4), np.float32)
    pred[0, :4], pred[0, 4], pred[0, 5] = box[:, :4].T, [0.9, 0.8, 0.7, 0.6], box[:, 4]
    o = f64.nms_rotated64(pred, 0.25, 0.45)[0]
    assert list(o["index"]) == [0, 2] and o["colmax"][0] == 0.0
    assert len(f64.nms_rotated64(pred, 0.25, 0.0)[0]["index"]) == 0
    assert list(f64.nms_rotated64(pred, 0.25, 1.0)[0]["index"]) == [0, 1, 2, 3]
    assert list(f64.nms_rotated64(pred, 0.25, 0.45, max_nms=1)[0]["index"]) == [0]


# ---- structure
@pytest.mark.parametrize("scale", list(obb_synth.SCALES))
def test_registry_builds_the_reference_graph(structure, scale):
    name = obb_synth.NAME.format(scale)
    want = structure[name]
    m = OBBModel(name)
    assert sum(p.numel() for p in m.parameters()) == want["params"]
    assert list(m.save) == want["save"] and [float(s) for s in m.stride] == want["stride"]
    assert [dict(i=l.i, f=l.f, type=l.type, np=int(l.np)) for l in m.model] == want["layers"]
    assert list(m.state_dict()) == want["keys"]
    head = m.model[-1]
    assert isinstance(head, M.OBB) and dict(ne=head.ne) == want["head"] and len(head.cv4) == 3
    assert head.cv4[0][2].out_channels == 1


def test_n_scale_parameter_count(structure):
    assert structure["yolo11n-obb.yaml"]["params"] == 2695747


def test_guess_model_task_and_facade():
    assert guess_model_task("yolo11n-obb.yaml") == "obb" and guess_model_task(yaml_model_load("yolo11s-obb.yaml")) == "obb"
    assert guess_model_task("yolo11n.yaml") == "detect" and guess_model_task("yolo11n-seg.yaml") == "segment"
    y = edge_yolo_amd.YOLO("yolo11n-obb.yaml")
    assert y.task == "obb" and isinstance(y.model, OBBModel) and guess_model_task(y.model) == "obb" and y.model.task == "obb"
    assert y._task_entry()["model"] is OBBModel and y._task_entry()["predictor"].__name__ == "OBBPredictor"
    assert guess_model_task(DetectionModel("yolo11n.yaml")) == "detect"
    with pytest.raises(ValueError):
        edge_yolo_amd.YOLO("yolo11n-obb.yaml", task="detect")


def test_obb_row_on_another_backbone():
    d = obb_synth.edgeline_obb_cfg(yaml_model_load("yolo11n-test.yaml"))
    m = OBBModel(d)
    assert isinstance(m.model[-1], M.OBB) and m.model[-1].ne == 1 and [float(s) for s in m.stride] == [8.0, 16.0, 32.0]
    assert guess_model_task(d) == "obb" and edge_yolo_amd.YOLO(d).task == "obb"


def test_module_keys_match_the_reference(obb_ops):
    tag, kw, _ = obb_synth.HEAD_CASE
    M.OBB.legacy = False
    assert list(M.OBB(**kw).state_dict()) == list(obb_ops[tag + "_keys"])


# ---- tensor utilities and the results container
def test_rbox_utilities_match_the_reference(obb_ops):
    rb = obb_synth.rbox_vectors()
    np.testing.assert_array_equal(uops.regularize_rboxes(rb).numpy(), obb_ops["rboxes_regularized"])
    np.testing.assert_array_equal(uops.xywhr2xyxyxyxy(rb).numpy(), obb_ops["rboxes_corners"])
    reg = uops.regularize_rboxes(rb)
    assert bool((reg[:, 2] >= reg[:, 3]).all()) and bool((reg[:, 4] >= 0).all()) and bool((reg[:, 4] < np.pi).all())
    np.testing.assert_allclose(uops.xywhr2xyxyxyxy(rb.numpy()), obb_ops["rboxes_corners"], rtol=1e-6, atol=1e-4)  # the numpy form
    assert uops.xywhr2xyxyxyxy(rb[None]).shape == (1, 12, 4, 2)


def test_results_obb_matches_the_reference(model_golden):
    g = model_golden
    obb = torch.tensor(g["obb0"])
    r = Results(np.zeros((64, 96, 3), np.uint8), path="image0.jpg", names={i: str(i) for i in range(80)}, obb=obb)
    assert r.boxes is None and r.masks is None and isinstance(r.obb, OBB) and len(r) == len(r.obb) == len(obb) >= 5
    assert r.obb.orig_shape == (64, 96)
    np.testing.assert_array_equal(r.obb.xywhr.numpy(), g["obb0"][:, :5])
    np.testing.assert_array_equal(r.obb.conf.numpy(), g["obb0"][:, 5])
    np.testing.assert_array_equal(r.obb.cls.numpy(), g["obb0"][:, 6])
    np.testing.assert_array_equal(r.obb.xyxyxyxy.numpy(), g["obb0_xyxyxyxy"])
    np.testing.assert_array_equal(r.obb.xyxyxyxyn.numpy(), g["obb0_xyxyxyxyn"])
    np.testing.assert_array_equal(r.obb.xyxy.numpy(), g["obb0_xyxy"])
    n = r.obb.numpy()
    assert isinstance(n.data, np.ndarray) and n.xyxy.shape == (len(obb), 4) and n.xyxyxyxyn.shape == (len(obb), 4, 2) and len(r.obb.cpu()) == len(obb)
    np.testing.assert_allclose(n.xyxy, g["obb0_xyxy"], rtol=1e-6, atol=1e-4)
    assert len(Results(None, "a", {}, obb=torch.zeros(0, 7))) == 0
    with pytest.raises(AssertionError):
        OBB(torch.zeros(2, 6), (4, 4))


def test_postprocess_of_the_golden_rows(model_golden):
    """regularize_rboxes + scale_boxes(xywh=True) on the reference's NMS rows give the reference's final obb rows."""
    g = model_golden
    det = torch.tensor(g["det0"])
    rb = uops.regularize_rboxes(torch.cat([det[:, :4], det[:, -1:]], -1))
    rb[:, :4] = uops.scale_boxes((64, 96), rb[:, :4], (64, 96), xywh=True)
    np.testing.assert_array_equal(torch.cat([rb, det[:, 4:6]], -1).numpy(), g["obb0"])


def test_refusals():
    y = edge_yolo_amd.YOLO("yolo11n-obb.yaml")
    x = torch.zeros(1, 3, 64, 64)
    with pytest.raises(NotImplementedError, match="obb"):
        y.val([{"img": x}])
    with pytest.raises(NotImplementedError, match="obb"):
        next(iter(y.predict_batches([x])))
    with pytest.raises(NotImplementedError, match="multi_label"):
        uops.non_max_suppression(torch.zeros(1, 8, 10), nc=3, multi_label=True, rotated=True)
    with pytest.raises(NotImplementedError, match="nc="):
        uops.nms_device(torch.zeros(1, 8, 10), rotated=True)
    with pytest.raises(ValueError):
        uops.nms_device(torch.zeros(1, 8, 10), nc=5, rotated=True)
    with pytest.raises(NotImplementedError):
        M.OBB(nc=3, ne=2, ch=(16,)).eval()([torch.zeros(1, 16, 2, 2)])
