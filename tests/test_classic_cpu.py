"""YOLOv3, YOLOv5 and YOLOv6 without a GPU: structure, state_dict keys and parameter counts against the reference
(tests/golden/structure_classic.json), every scale name of the three families, the strides from the graph alone (two levels for yolov3-tiny),
the YAML `activation:` confined to the model that names it, the task guess, the refusals of what has no kernel, the module keys against
tests/golden/classic_ops.npz, and the row condition of the model goldens re-checked on the recorded rows."""
import copy
import json
import os

import numpy as np
import pytest
import torch.nn as nn

import classic_synth as cs


@pytest.fixture(scope="module")
def structure(golden_dir):
    with open(os.path.join(golden_dir, "structure_classic.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def ops_golden(golden_dir):
    return np.load(os.path.join(golden_dir, "classic_ops.npz"))


@pytest.mark.parametrize("name", cs.STRUCT_FILES)
def test_structure_matches_reference(structure, name):
    from edge_yolo_amd.nn.tasks import DetectionModel, guess_model_task
    want = structure[name]
    m = DetectionModel(name)
    assert sum(p.numel() for p in m.parameters()) == want["params"] == cs.PARAMS[name]
    assert list(m.save) == want["save"]
    assert [float(s) for s in m.stride] == want["stride"] == cs.STRIDES[name]
    assert [dict(i=l.i, f=l.f, type=l.type, np=int(l.np)) for l in m.model] == want["layers"]
    assert list(m.state_dict()) == cs.unpack_keys(want["keys"])
    assert guess_model_task(name) == "detect" and guess_model_task(m) == "detect"
    head = m.model[-1]
    assert type(head).__name__ == "Detect" and head.legacy is True is want["legacy"] and head.nl == len(want["stride"])


@pytest.mark.parametrize("name,file,scale", cs.NAMES, ids=[n[0] for n in cs.NAMES])
def test_every_scale_name_resolves(name, file, scale):
    """'yolov5s.yaml' -> v5/yolov5.yaml + scale 's'; the v3 names are files of their own.  The small scales are built as well."""
    from edge_yolo_amd.nn.tasks import CFG_DIR, DetectionModel, guess_model_task, yaml_model_load
    import yaml
    d = yaml_model_load(name)
    on_disk = yaml.safe_load(open(CFG_DIR / file, encoding="utf-8"))
    assert d["scale"] == scale and d["backbone"] == on_disk["backbone"] and d["head"] == on_disk["head"]
    assert ("scales" in d) == bool(scale) and (not scale or scale in d["scales"])
    assert guess_model_task(d) == "detect"
    if scale in ("n", "s"):
        m = DetectionModel(name)
        width = d["scales"][scale][1]
        assert m.model[0].conv.out_channels == int(64 * width) and type(m.model[-1]).__name__ == "Detect"


def test_strides_come_from_the_graph_without_a_forward():
    from edge_yolo_amd.nn.tasks import DetectionModel
    tiny = DetectionModel("yolov3-tiny.yaml")
    assert [float(s) for s in tiny.stride] == [16.0, 32.0] and tiny.model[-1].nl == 2
    assert tiny._down[:13] == [1.0, 2.0, 2.0, 4.0, 4.0, 8.0, 8.0, 16.0, 16.0, 32.0, 32.0, 32.0, 32.0]  # MaxPool2d: x stride; ZeroPad2d: x 1
    v6 = DetectionModel("yolov6n.yaml")
    assert [float(s) for s in v6.stride] == [8.0, 16.0, 32.0]
    assert (v6._down[10], v6._down[11], v6._down[16]) == (32.0, 16.0, 8.0)  # ConvTranspose2d: / 2
    assert [float(s) for s in DetectionModel("yolov5n-p6.yaml").stride] == [8.0, 16.0, 32.0, 64.0]


def test_zeropad_in_front_of_its_only_reader_is_lazy():
    from edge_yolo_amd.nn.modules import MaxPool2d, ZeroPad2d
    from edge_yolo_amd.nn.tasks import DetectionModel, yaml_model_load
    m = DetectionModel("yolov3-tiny.yaml")
    assert isinstance(m.model[11], ZeroPad2d) and isinstance(m.model[12], MaxPool2d) and m.model[11].lazy is True
    d = yaml_model_load("yolov3-tiny.yaml")
    d["head"][0][0] = 11  # the first head Conv reads the padded map itself (33 channels wide maps are fine on the CPU: nothing runs)
    assert DetectionModel(d).model[11].lazy is False  # a second reader: the padded map has to exist


def test_activation_key_applies_to_its_own_model_only():
    from edge_yolo_amd.nn.modules import Conv
    from edge_yolo_amd.nn.tasks import DetectionModel, yaml_model_load
    assert isinstance(Conv.default_act, nn.SiLU)
    v6 = DetectionModel("yolov6n.yaml")
    convs = [c for c in v6.modules() if isinstance(c, Conv)]
    assert convs and all(isinstance(c.act, nn.ReLU) for c in convs)
    assert isinstance(Conv.default_act, nn.SiLU)
    v5 = DetectionModel("yolov5n.yaml")  # built after a YOLOv6: still a SiLU model
    assert all(isinstance(c.act, nn.SiLU) for c in v5.modules() if isinstance(c, Conv))
    d = yaml_model_load("yolov6n.yaml")
    d["head"][5] = [-1, 1, "NoSuchModule", [128]]  # the build raises half-way, behind ReLU Convs
    with pytest.raises(NotImplementedError):
        DetectionModel(d)
    assert isinstance(Conv.default_act, nn.SiLU)
    assert isinstance(Conv(8, 8).act, nn.SiLU)


def test_task_guess():
    from edge_yolo_amd import YOLO
    from edge_yolo_amd.nn.tasks import guess_model_task
    for name in ("yolov5n.yaml", "yolov5s-p6.yaml", "yolov3.yaml", "yolov3-spp.yaml", "yolov3-tiny.yaml", "yolov6s.yaml"):
        assert guess_model_task(name) == "detect"
    for name in ("yolov5n.yaml", "yolov3-tiny.yaml", "yolov6n.yaml"):
        y = YOLO(name)
        assert y.task == "detect" and type(y.model).__name__ == "DetectionModel"


def _row_model(row, ch=16):
    from edge_yolo_amd.nn.tasks import parse_model
    return parse_model({"nc": 80, "backbone": [row], "head": []}, ch)


def test_refusals():
    from edge_yolo_amd.nn import modules as M
    with pytest.raises(NotImplementedError):
        M.SPP(32, 32, k=(3, 5, 7))
    with pytest.raises(NotImplementedError):
        _row_model([-1, 1, "SPP", [32, [3, 5, 7]]])
    with pytest.raises(NotImplementedError):
        _row_model([-1, 1, "nn.MaxPool2d", [3, 2, 1]])
    with pytest.raises(NotImplementedError):
        _row_model([-1, 1, "nn.ConvTranspose2d", [16, 3, 2]])
    with pytest.raises(NotImplementedError, match="nn.AvgPool2d"):
        _row_model([-1, 1, "nn.AvgPool2d", [2]])
    for bad in (dict(kernel_size=2, stride=2, padding=1), dict(kernel_size=2, stride=2, dilation=2), dict(kernel_size=2, stride=2, ceil_mode=True),
                dict(kernel_size=2, stride=2, return_indices=True), dict(kernel_size=2, stride=3)):
        with pytest.raises(NotImplementedError):
            M.MaxPool2d(**bad)
    assert _row_model([-1, 1, "nn.MaxPool2d", [2, 2, 0]])[0][0].type == "torch.nn.modules.pooling.MaxPool2d"
    assert _row_model([-1, 1, "nn.ZeroPad2d", [[0, 1, 0, 1]]])[0][0].type == "torch.nn.modules.padding.ZeroPad2d"
    up = _row_model([-1, 1, "nn.ConvTranspose2d", [32, 2, 2, 0]])[0][0]
    assert up.type == "torch.nn.modules.conv.ConvTranspose2d" and (up.in_channels, up.out_channels) == (16, 32) and list(up.state_dict()) == ["weight", "bias"]


def test_torch_rows_are_subclasses_with_torch_keys():
    from edge_yolo_amd.nn import modules as M
    assert issubclass(M.MaxPool2d, nn.MaxPool2d) and issubclass(M.ZeroPad2d, nn.ZeroPad2d) and issubclass(M.ConvTranspose2d, nn.ConvTranspose2d)
    a, b = M.ConvTranspose2d(16, 24, 2, 2, 0), nn.ConvTranspose2d(16, 24, 2, 2, 0)
    assert {k: tuple(v.shape) for k, v in a.state_dict().items()} == {k: tuple(v.shape) for k, v in b.state_dict().items()}
    copy.deepcopy(a)  # (models are deep-copied by the facade)


OWN_NS = None


def _own_ns():
    from edge_yolo_amd.nn import modules as M
    from edge_yolo_amd.nn.tasks import parse_model
    return {"Conv": M.Conv, "SPP": M.SPP, "MaxPool2d": M.MaxPool2d, "ZeroPad2d": M.ZeroPad2d, "ConvTranspose2d": M.ConvTranspose2d, "parse": parse_model}


def test_module_keys_match_reference(ops_golden):
    for tag in cs.OPS_CASES:
        m = cs.make_module(tag, _own_ns())
        assert list(m.state_dict()) == [str(k) for k in ops_golden[tag + "_keys"]], tag
    row = cs.make_module("bottleneck_row_n2", _own_ns())
    assert isinstance(row[0], nn.Sequential) and len(row[0]) == 2 and row[0].type == "ultralytics.nn.modules.block.Bottleneck"


def test_golden_rows_are_separated(golden_dir):
    """What the generator asserted on the reference alone, re-checked on the recorded rows: per image at least 5 kept rows, their scores more
    than 1e-3 apart, and no candidate's best score within 1e-3 of conf."""
    for tag, (name, shape, *_) in cs.MODEL_CASES.items():
        g = np.load(os.path.join(golden_dir, tag + ".npz"))
        assert g["y"].shape[0] == shape[0] and sum(f"raw{i}" in g for i in range(5)) == cs.NL[tag]
        assert g["y"].shape[2] == sum(g[f"raw{i}"].shape[2] * g[f"raw{i}"].shape[3] for i in range(cs.NL[tag]))
        for i in range(shape[0]):
            n, gap, margin = cs.kept_rows_separated(g["y"][i], g[f"det{i}"], float(g["conf"]))
            assert n == len(g[f"det{i}"]) >= cs.MIN_ROWS and gap > cs.ROW_GAP and margin > cs.ROW_GAP
    g = np.load(os.path.join(golden_dir, "yolov5n-p6_64x128.npz"))
    assert g["raw3"].shape[2:] == (1, 2)  # the 1x2 map at stride 64
