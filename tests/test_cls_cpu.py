"""CPU checks of the classify task: registry / structure / state_dict keys / parameter counts of yolo11{n,s,m,l,x}-cls.yaml against what the
reference builds (tests/golden/structure_cls.json), guess_model_task, the parse rule, the checkpoint round trip, Probs against the
reference's own fields, ClassifyMetrics and the validator's host bookkeeping against the reference's validator (tests/golden/
clsval_case.npz), the float64 restatements (tests/fp64_cls_ref.py) against the reference's fp32 values and Pillow (tests/golden/cls_ops.npz),
and the refusals."""
import json
import os

import numpy as np
import pytest
import torch

import edge_yolo_amd
from edge_yolo_amd import _lib as L
from edge_yolo_amd.data.augment import ClassifyTransform
from edge_yolo_amd.engine.predictor import ClassificationPredictor
from edge_yolo_amd.engine.results import Probs, Results
from edge_yolo_amd.engine.validator import ClassificationValidator
from edge_yolo_amd.nn import modules as M
from edge_yolo_amd.nn.tasks import ClassificationModel, DetectionModel, guess_model_task, parse_model, yaml_model_load
from edge_yolo_amd.utils import metrics
import cls_synth
import fp64_cls_ref as f64

KEYS = ["metrics/accuracy_top1", "metrics/accuracy_top5", "fitness"]


@pytest.fixture(scope="module")
def structure(golden_dir):
    return json.load(open(os.path.join(golden_dir, "structure_cls.json")))


@pytest.fixture(scope="module")
def cls_ops(golden_dir):
    return np.load(os.path.join(golden_dir, "cls_ops.npz"))


@pytest.fixture(scope="module")
def case(golden_dir):
    return np.load(os.path.join(golden_dir, "clsval_case.npz"))


# ------------------------------------------------------------------------------------------------------------------ registry
@pytest.mark.parametrize("scale", list(cls_synth.SCALES))
def test_registry_builds_the_reference_graph(structure, scale):
    name = cls_synth.NAME.format(scale)
    want = structure[name]
    m = ClassificationModel(name, nc=1000)
    assert sum(p.numel() for p in m.parameters()) == want["params"]
    assert list(m.save) == want["save"] and [float(s) for s in m.stride] == want["stride"] == [1.0]
    assert [dict(i=l.i, f=l.f, type=l.type, np=int(l.np)) for l in m.model] == want["layers"]
    assert list(m.state_dict()) == want["keys"]
    assert m.names == {i: str(i) for i in range(1000)} and not m.training
    # the reference's ClassificationModel never calls initialize_weights: its BatchNorm layers keep torch's eps (detect-family models: 1e-3)
    assert {mod.eps for mod in m.modules() if isinstance(mod, torch.nn.BatchNorm2d)} == {1e-5}
    head = m.model[-1]
    assert isinstance(head, M.Classify) and head.linear.out_features == 1000 and head.conv.conv.out_channels == 1280
    assert sum(p.numel() for p in ClassificationModel(name, nc=3).parameters()) == want["params_nc3"]


def test_head_members_and_keys(cls_ops):
    tag, c1, c2, _ = cls_synth.HEAD_CASE
    head = M.Classify(c1, c2)
    assert list(head.state_dict()) == list(cls_ops[tag + "_keys"])
    assert {"conv.conv.weight", "conv.bn.weight", "conv.bn.running_var", "linear.weight", "linear.bias"} <= set(head.state_dict())
    assert isinstance(head.pool, torch.nn.AdaptiveAvgPool2d) and isinstance(head.drop, torch.nn.Dropout)
    assert not list(head.pool.parameters()) and not list(head.drop.parameters()) and not list(head.pool.buffers())


def test_guess_model_task():
    assert guess_model_task("yolo11n-cls.yaml") == "classify" and guess_model_task(yaml_model_load("yolo11s-cls.yaml")) == "classify"
    assert guess_model_task(ClassificationModel("yolo11n-cls.yaml")) == "classify"
    for name in ("classify", "classifier", "cls", "fc"):
        assert guess_model_task(name) == "classify"
    assert guess_model_task("yolo11n.yaml") == "detect" and guess_model_task("yolo11n-pose.yaml") == "pose"
    assert guess_model_task(DetectionModel("yolo11n.yaml")) == "detect"


@pytest.mark.parametrize("nc", [1000, 3])
def test_parse_rule_keeps_nc_unscaled(nc):
    d = yaml_model_load("yolo11n-cls.yaml")
    d["nc"] = nc
    model, save = parse_model(dict(d), ch=3)
    head = model[-1]
    assert isinstance(head, M.Classify) and head.linear.out_features == nc and head.linear.in_features == 1280 and save == []
    assert head.conv.conv.in_channels == 256  # 1024 x 0.25: the layer before is width-scaled, the class count is not
    assert head.f == -1 and head.i == 10 and head.type == "ultralytics.nn.modules.head.Classify"


def test_model_needs_nc_and_reshape_outputs():
    d = yaml_model_load("yolo11n-cls.yaml")
    d.pop("nc")
    with pytest.raises(ValueError, match="nc not specified"):
        ClassificationModel(dict(d))
    m = ClassificationModel(dict(d), nc=7)
    assert m.model[-1].linear.out_features == 7 and len(m.names) == 7
    ClassificationModel.reshape_outputs(m, 4)
    assert m.model[-1].linear.out_features == 4
    lin = m.model[-1].linear
    ClassificationModel.reshape_outputs(m, 4)
    assert m.model[-1].linear is lin


def test_facade_and_checkpoint_round_trip(tmp_path):
    y = edge_yolo_amd.YOLO("yolo11n-cls.yaml", nc=6)
    assert y.task == "classify" and isinstance(y.model, ClassificationModel) and guess_model_task(y.model) == "classify"
    assert set(y.task_map) == {"detect", "segment"}
    entry = y._task_entry()
    assert entry["model"] is ClassificationModel and entry["predictor"] is ClassificationPredictor and entry["validator"] is ClassificationValidator
    with pytest.raises(ValueError):
        edge_yolo_amd.YOLO("yolo11n-cls.yaml", task="detect")
    with pytest.raises(ValueError, match="iterable of batch dicts"):
        y.val()
    y.model.load_state_dict(cls_synth.state_dict(y.model.state_dict()))
    path = str(tmp_path / "cls.pt")
    y.save(path)
    z = edge_yolo_amd.YOLO(path)
    assert z.task == "classify" and z.model.model[-1].linear.out_features == 6 and len(z.names) == 6
    for (ka, a), (kb, b) in zip(y.model.state_dict().items(), z.model.state_dict().items()):
        assert ka == kb and torch.equal(a, b), ka


# ------------------------------------------------------------------------------------------------------------------ Probs / Results
def test_probs_against_reference(cls_ops):
    for name in ("probs80", "probs2"):
        data = torch.tensor(cls_ops[name + "_data"])
        p = Probs(data)
        assert p.top1 == int(cls_ops[name + "_top1"]) and p.top5 == list(cls_ops[name + "_top5"])
        assert float(p.top1conf) == float(cls_ops[name + "_top1conf"])
        np.testing.assert_array_equal(p.top5conf.numpy(), cls_ops[name + "_top5conf"])
        n = p.numpy()
        assert isinstance(n.data, np.ndarray) and n.top5 == p.top5 and n.top1 == p.top1 and p.cpu().top5 == p.top5
        np.testing.assert_array_equal(n.top5conf, cls_ops[name + "_top5conf"])
        # with the head's own top-k attached the fields come from it
        k = len(p.top5)
        q = Probs(data, top=(torch.tensor(f64.rank(data.numpy()[None])[0]), data[torch.tensor(p.top5)]))
        assert q.top5 == p.top5 and q.top1 == p.top1 and len(q.numpy().top5) == k
    r = Results(None, "a.jpg", {0: "0"}, probs=torch.tensor(cls_ops["probs80_data"]))
    assert r.probs is not None and r.boxes is None and r.masks is None and r.obb is None and r.keypoints is None and len(r) == 80


# ------------------------------------------------------------------------------------------------------------------ metrics / validator
def test_classify_metrics_against_reference(case):
    for tag, nc in (("host10", 10), ("host3", 3)):
        m = metrics.ClassifyMetrics()
        pred, cls = case[tag + "_pred"], case[tag + "_cls"]
        assert pred.shape[1] == min(nc, 5)
        m.process([torch.tensor(cls[:8]).int(), torch.tensor(cls[8:]).int()], [torch.tensor(pred[:8]), torch.tensor(pred[8:])])
        assert m.keys == KEYS[:2] and list(m.results_dict) == KEYS
        assert [m.top1, m.top5, m.fitness] == list(case[tag + "_values"]) and m.fitness == (m.top1 + m.top5) / 2
        assert m.curves == [] and m.curves_results == []


class _Names:
    def __init__(self, nc):
        self.names = {i: str(i) for i in range(nc)}
        self.p = torch.nn.Parameter(torch.zeros(1))

    def parameters(self):
        return iter([self.p])

    forward_layers = None


def test_validator_host_bookkeeping_against_reference(case):
    for tag, nc in (("host10", 10), ("host3", 3)):
        v = ClassificationValidator(_Names(nc), device="cpu")
        p, cls = cls_synth.host_probs(tag, 16, nc), case[tag + "_cls"]
        v.update_metrics(torch.tensor(p[:8]), {"cls": torch.tensor(cls[:8])})
        v.update_metrics((p[8:], None), {"cls": cls[8:]})  # the eval forward's (probs, logits) tuple, numpy
        np.testing.assert_array_equal(np.concatenate(v.pred), case[tag + "_pred"])
        res = v.get_stats()
        assert list(res) == KEYS and list(res.values()) == list(case[tag + "_values"])
    # the model-level case: the reference's probabilities through the host route give the reference's numbers
    v = ClassificationValidator(_Names(int(case["nc"])), device="cpu")
    v.update_metrics(case["probs"], {"cls": case["cls"]})
    np.testing.assert_array_equal(v.pred[0], case["pred"])
    assert list(v.get_stats().values()) == list(case["values"]) and list(case["keys"]) == KEYS
    with pytest.raises(NotImplementedError, match="plots"):
        ClassificationValidator(_Names(3), device="cpu", plots=True)


# ------------------------------------------------------------------------------------------------------------------ float64 restatements
def test_fp64_linear_softmax_against_reference(cls_ops):
    for tag in cls_synth.LINEAR_FULL:
        pooled, w, b = cls_synth.linear_case(tag)
        l64, p64 = f64.linear_softmax64(pooled, w, b)
        assert float(np.abs(l64 - cls_ops[tag + "_logits"]).max()) == float(cls_ops[tag + "_El"])  # E is this very difference
        assert float(np.abs(p64 - cls_ops[tag + "_probs"]).max()) == float(cls_ops[tag + "_Ep"])
        assert float(cls_ops[tag + "_El"]) < 1e-4 and float(cls_ops[tag + "_Ep"]) < 1e-6
    for tag in cls_synth.LINEAR_CASES:
        n = 1 if cls_synth.LINEAR_CASES[tag][3] == "big" else 5
        np.testing.assert_array_equal(f64.rank(f64.linear_softmax64(*cls_synth.linear_case(tag))[1])[:, :n], cls_ops[tag + "_top"][:, :n])
    assert f64.rank(np.full((2, 80), 1 / 80)).tolist() == [[0, 1, 2, 3, 4]] * 2 and f64.rank(np.array([[0.5, 0.5]])).tolist() == [[0, 1]]


def test_fp64_head_against_reference(cls_ops):
    tag, c1, c2, shape = cls_synth.HEAD_CASE
    head = M.Classify(c1, c2)
    head.load_state_dict(cls_synth.state_dict(head.state_dict(), prefix=tag + "."))
    w, b = head.conv.folded()
    mean, _, _ = f64.pool64(cls_synth.case_input(tag, shape).numpy(), w.reshape(1280, c1).numpy(), b.numpy(), True)
    l64, p64 = f64.linear_softmax64(mean, head.linear.weight.detach().numpy(), head.linear.bias.detach().numpy())
    np.testing.assert_allclose(l64, cls_ops[tag + "_logits"], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(p64, cls_ops[tag + "_probs"], rtol=1e-5, atol=1e-6)


def test_fp64_transform_against_pillow(cls_ops):
    assert len(cls_synth.TRANSFORM_CASES) >= 9
    origins = set()
    for tag, h, w, S in cls_synth.TRANSFORM_CASES:
        nh, nw = f64.resized(h, w, S)
        t, l = f64.crop_origin(nh, S), f64.crop_origin(nw, S)
        assert [nh, nw, t, l] == list(cls_ops[tag + "_geom"]) and (nh, nw) == ClassifyTransform.resized(h, w, S)
        assert (t, l) == (ClassifyTransform.crop_origin(nh, S), ClassifyTransform.crop_origin(nw, S))
        origins.add((max(nh, nw) - S, max(t, l)))
        got = f64.transform(cls_synth.transform_image(tag, h, w), S)
        assert float(np.abs(got - cls_ops[tag + "_pil"]).max()) <= 1.0 + 2.0 ** -8, tag
    assert {(1, 0), (3, 2), (5, 2), (17, 8)} <= origins  # round-half-to-even


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_refusals():
    with pytest.raises(NotImplementedError):
        M.Classify(64, 10, k=3)
    with pytest.raises(NotImplementedError):
        M.Classify(64, 10, s=2)
    with pytest.raises(NotImplementedError):
        M.Classify(64, 10, g=2)
    y = edge_yolo_amd.YOLO("yolo11n-cls.yaml")
    with pytest.raises(NotImplementedError, match="classify"):
        next(y.predict_batches([torch.zeros(1, 3, 64, 64)]))
    with pytest.raises(NotImplementedError, match="augment"):
        ClassificationPredictor(y.model, torch.device("cpu"), augment=True)
    with pytest.raises(NotImplementedError, match="8192"):
        M.Classify(64, 8193).eval()(torch.zeros(1, 64, 2, 2))
    # the library refuses before it looks at a pointer
    lib = L.lib()
    assert lib.ey_classify_linear_softmax(L.F32, 1, 1280, 8193, None, None, None, None, None, None, None, None) == -2
    assert b"8192" in lib.ey_last_error()
    assert lib.ey_classify_linear_softmax(L.F32, 1, 1280, 0, None, None, None, None, None, None, None, None) == -1
    assert lib.ey_classify_pool(L.F16, 1, 49, 12, 1280, L.ACT_SILU, None, 12, None, None, None, None) == -1  # (null pointers come first)
    assert lib.ey_classify_transform(L.F32, None, 1, 8, 8, 24, 192, None, 8, 1, None) == -1
    with pytest.raises(NotImplementedError):
        ClassifyTransform((224, 200))
