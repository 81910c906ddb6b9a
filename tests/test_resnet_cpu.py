"""CPU checks of the ResNet classifiers and the YOLOv8 task models: every scale of the eight YAMLs under cfg/models/v8 builds the graph the
reference builds from its own files (tests/golden/structure_v8tasks.json: parameter counts, layer types, save list, strides, state_dict
keys), ResNetLayer's parse rule and module layout, a state_dict written the reference's way loads, task guessing and the facade's classes,
and the refusals that stay: (5, 2, 2) stems, 3x3 max-pools outside ResNetLayer, OBB validation, predict_batches of seg / obb / cls."""
import hashlib
import json
import os

import pytest
import torch

import edge_yolo_amd
from edge_yolo_amd.engine import predictor as P
from edge_yolo_amd.engine import validator as V
from edge_yolo_amd.nn import _ops as ops
from edge_yolo_amd.nn import modules as M
from edge_yolo_amd.nn.tasks import ClassificationModel, DetectionModel, OBBModel, PoseModel, SegmentationModel, guess_model_task, parse_model, yaml_model_load
import resnet_synth as rs

MODEL = {"classify": ClassificationModel, "segment": SegmentationModel, "pose": PoseModel, "obb": OBBModel}
NAMES = [rs.scaled(base, sc) for base in rs.V8_TASK_YAMLS for sc in rs.SCALES]


@pytest.fixture(scope="module")
def structure(golden_dir):
    return json.load(open(os.path.join(golden_dir, "structure_v8tasks.json")))


def _build(name):
    task = rs.task_of(name)
    return MODEL[task](name, nc=1000) if task == "classify" else MODEL[task](name)


@pytest.mark.parametrize("name", NAMES)
def test_registry_builds_the_reference_graph(structure, name):
    want = structure[name]
    assert guess_model_task(name) == want["task"] == rs.task_of(name)
    m = _build(name)
    assert sum(p.numel() for p in m.parameters()) == want["params"]
    assert list(m.save) == want["save"] and [float(s) for s in m.stride] == want["stride"]
    assert [dict(i=l.i, f=l.f, type=l.type, np=int(l.np)) for l in m.model] == want["layers"]
    keys = list(m.state_dict())
    assert len(keys) == want["nkeys"] and hashlib.sha1("\n".join(keys).encode()).hexdigest() == want["keys_sha1"]
    if "keys" in want:
        assert keys == want["keys"]
    if want["task"] == "classify":  # the reference's ClassificationModel keeps torch's BatchNorm eps
        assert {mod.eps for mod in m.modules() if isinstance(mod, torch.nn.BatchNorm2d)} == {1e-5}


@pytest.mark.parametrize("base,params,nkeys", [("yolov8-cls-resnet50.yaml", 27413032, 326), ("yolov8-cls-resnet101.yaml", 46405160, 632)])
def test_resnet_is_the_same_at_every_scale(structure, base, params, nkeys):
    n, x = structure[rs.scaled(base, "n")], structure[rs.scaled(base, "x")]
    assert n["params"] == x["params"] == params and n["nkeys"] == x["nkeys"] == nkeys and n["keys_sha1"] == x["keys_sha1"] and n["layers"] == x["layers"]
    assert n["stride"] == [1.0] and n["save"] == []
    assert [l["type"] for l in n["layers"]] == ["ultralytics.nn.modules.block.ResNetLayer"] * 5 + ["ultralytics.nn.modules.head.Classify"]


def test_strides_and_parameter_counts_of_the_issue():
    want = {"yolov8n-cls.yaml": (2719288, [1.0]), "yolov8n-seg.yaml": (3409968, [8.0, 16.0, 32.0]), "yolov8n-pose.yaml": (3295470, [8.0, 16.0, 32.0]),
            "yolov8n-obb.yaml": (3228867, [8.0, 16.0, 32.0]), "yolov8n-seg-p6.yaml": (5302816, [8.0, 16.0, 32.0, 64.0]),
            "yolov8n-pose-p6.yaml": (5182152, [8.0, 16.0, 32.0, 64.0])}
    for name, (params, stride) in want.items():
        m = _build(name)
        assert sum(p.numel() for p in m.parameters()) == params and [float(s) for s in m.stride] == stride, name


def test_resnet_layer_parse_rule_and_layout():
    d = yaml_model_load("yolov8s-cls-resnet50.yaml")
    assert d["scale"] == "s"
    model, save = parse_model(dict(d), ch=3)
    assert save == [] and [type(l) for l in model] == [M.ResNetLayer] * 5 + [M.Classify]
    head = model[-1]
    assert head.conv.conv.in_channels == 2048 and head.linear.out_features == 1000  # c2 = 4 x 512: not scaled by the width factor 0.5
    stem = model[0]
    assert stem.is_first and isinstance(stem.layer[0], M.Conv) and isinstance(stem.layer[1], torch.nn.MaxPool2d)
    c = stem.layer[0].conv
    assert (c.in_channels, c.out_channels, c.kernel_size, c.stride, c.padding) == (3, 64, (7, 7), (2, 2), (3, 3)) and isinstance(stem.layer[0].act, torch.nn.SiLU)
    p = stem.layer[1]
    assert (p.kernel_size, p.stride, p.padding) == (3, 2, 1) and not list(p.parameters())
    assert [len(l.layer) for l in model[1:5]] == [3, 4, 6, 3]
    for l, (c1, c2, s) in zip(model[1:5], [(64, 64, 1), (256, 128, 2), (512, 256, 2), (1024, 512, 2)]):
        b0, b1 = l.layer[0], l.layer[1]
        assert isinstance(b0, M.ResNetBlock) and isinstance(b0.shortcut, torch.nn.Sequential) and isinstance(b1.shortcut, torch.nn.Identity)
        assert b0.cv1.conv.in_channels == c1 and b0.cv2.conv.stride == (s, s) and b0.cv3.conv.out_channels == 4 * c2 and b0.shortcut[0].conv.stride == (s, s)
        assert b1.cv1.conv.in_channels == 4 * c2 and b1.cv2.conv.stride == (1, 1)
        assert isinstance(b0.cv1.act, torch.nn.SiLU) and isinstance(b0.cv2.act, torch.nn.SiLU)
        assert isinstance(b0.cv3.act, torch.nn.Identity) and isinstance(b0.shortcut[0].act, torch.nn.Identity)
    keys = set(model.state_dict())
    assert {"0.layer.0.conv.weight", "0.layer.0.bn.running_var", "1.layer.0.cv1.conv.weight", "1.layer.0.shortcut.0.conv.weight", "1.layer.2.cv3.bn.bias"} <= keys
    assert not any(k.startswith("0.layer.1") for k in keys)


def test_resnet_constructor_signature():
    l = M.ResNetLayer(64, 32, 2, False, 2, 2)  # (c1, c2, s, is_first, n, e)
    assert len(l.layer) == 2 and l.layer[0].cv3.conv.out_channels == 64 and l.layer[1].cv1.conv.in_channels == 64
    assert isinstance(l.layer[0].shortcut, torch.nn.Sequential)  # stride 2
    assert isinstance(M.ResNetLayer(128, 32, 1, n=1).layer[0].shortcut, torch.nn.Identity)  # c1 == e c2 at stride 1
    b = M.ResNetBlock(16, 8)
    assert b.cv3.conv.out_channels == 32 and b.cv2.conv.padding == (1, 1)


def test_reference_style_state_dict_loads_and_round_trips(structure, tmp_path):
    """keys exactly as the reference names them (structure_v8tasks.json), values from the seeded generator: strict loading."""
    y = edge_yolo_amd.YOLO("yolov8n-cls-resnet50.yaml", nc=6)
    shapes = {k: tuple(v.shape) for k, v in y.model.state_dict().items()}
    ref_keys = [k for k in structure["yolov8n-cls-resnet50.yaml"]["keys"]]
    assert list(shapes) == ref_keys
    sd = rs.state_dict({k: torch.empty(shapes[k]) for k in ref_keys})
    y.model.load_state_dict(sd, strict=True)
    assert torch.equal(y.model.model[1].layer[0].shortcut[0].conv.weight, sd["model.1.layer.0.shortcut.0.conv.weight"])
    path = str(tmp_path / "r50.pt")
    y.save(path)
    z = edge_yolo_amd.YOLO(path)
    assert z.task == "classify" and z.model.model[-1].linear.out_features == 6
    for (ka, a), (kb, b) in zip(y.model.state_dict().items(), z.model.state_dict().items()):
        assert ka == kb and torch.equal(a, b), ka


def test_task_guessing_and_facade_classes():
    want = {"yolov8n-cls-resnet50.yaml": ("classify", ClassificationModel, P.ClassificationPredictor, V.ClassificationValidator),
            "yolov8x-cls-resnet101.yaml": ("classify", ClassificationModel, P.ClassificationPredictor, V.ClassificationValidator),
            "yolov8n-cls.yaml": ("classify", ClassificationModel, P.ClassificationPredictor, V.ClassificationValidator),
            "yolov8s-seg-p6.yaml": ("segment", SegmentationModel, P.SegmentationPredictor, V.SegmentationValidator),
            "yolov8n-seg.yaml": ("segment", SegmentationModel, P.SegmentationPredictor, V.SegmentationValidator),
            "yolov8n-pose.yaml": ("pose", PoseModel, P.PosePredictor, V.PoseValidator),
            "yolov8m-pose-p6.yaml": ("pose", PoseModel, P.PosePredictor, V.PoseValidator)}
    for name, (task, model, pred, val) in want.items():
        assert guess_model_task(name) == task and guess_model_task(yaml_model_load(name)) == task
        y = edge_yolo_amd.YOLO(name)
        assert y.task == task and type(y.model) is model, name
        e = y._task_entry()
        assert e["model"] is model and e["predictor"] is pred and e["validator"] is val, name
    y = edge_yolo_amd.YOLO("yolov8n-obb.yaml")
    assert y.task == "obb" and type(y.model) is OBBModel and y._task_entry()["predictor"] is P.OBBPredictor
    assert guess_model_task(ClassificationModel("yolov8n-cls-resnet50.yaml", nc=3)) == "classify"
    with pytest.raises(FileNotFoundError):
        yaml_model_load("yolov8n-cls-resnet18.yaml")


def test_refusals_that_stay():
    with pytest.raises(NotImplementedError):  # OBB validation is not built
        edge_yolo_amd.YOLO("yolov8n-obb.yaml").val([])
    for name in ("yolov8n-seg.yaml", "yolov8n-obb.yaml", "yolov8n-cls-resnet50.yaml"):
        with pytest.raises(NotImplementedError):
            next(iter(edge_yolo_amd.YOLO(name).predict_batches([torch.zeros(1, 3, 64, 64)])))
    # a bare 3x3 stride-2 max-pool row is still no YAML row: the pool is reachable from ResNetLayer only
    d = yaml_model_load("yolov8n-cls.yaml")
    d["backbone"] = list(d["backbone"]) + [[-1, 1, "nn.MaxPool2d", [3, 2, 1]]]
    with pytest.raises(NotImplementedError):
        parse_model(dict(d), ch=3)
    with pytest.raises(NotImplementedError):
        M.MaxPool2d(3, 2, 1)
    assert (5, 2, 2) not in ops.STEM_KS and (7, 2, 3) in ops.STEM_KS and {(6, 2, 2), (3, 1, 1)} <= set(ops.STEM_KS)


def test_resnet_layer_is_not_block_recordable():
    from edge_yolo_amd.nn._block import BlockUnsupported
    layer = M.ResNetLayer(64, 16, 1, False, 1)
    ops.RECORD = object()
    try:
        with pytest.raises(BlockUnsupported):
            layer(torch.zeros(1, 64, 4, 4))
    finally:
        ops.RECORD = None
