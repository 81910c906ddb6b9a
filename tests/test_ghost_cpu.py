"""YOLOv8 and YOLOv8-ghost without a GPU: structure, state_dict keys and parameter counts of the six model files at all five scales against
the reference (tests/golden/structure_ghost.json), the pyramid levels of the P2 / P6 files, the hidden widths of the 1x1 GhostConvs (the
4-channel path of ey_ghost_conv cannot be dropped silently), the module keys against tests/golden/ghost_ops.npz, and the row condition of the
model goldens re-checked on the recorded rows."""
import json
import os

import numpy as np
import pytest

import ghost_synth as gs


@pytest.fixture(scope="module")
def structure(golden_dir):
    with open(os.path.join(golden_dir, "structure_ghost.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def ops_golden(golden_dir):
    return np.load(os.path.join(golden_dir, "ghost_ops.npz"))


@pytest.mark.parametrize("name", gs.FILES)
def test_structure_matches_reference(structure, name):
    from edge_yolo_amd.nn.tasks import DetectionModel, guess_model_task
    want = structure[name]
    m = DetectionModel(name)
    assert sum(p.numel() for p in m.parameters()) == want["params"]
    if name in gs.PARAMS:
        assert want["params"] == gs.PARAMS[name]
    assert list(m.save) == want["save"]
    assert [float(s) for s in m.stride] == want["stride"]
    assert [dict(i=l.i, f=l.f, type=l.type, np=int(l.np)) for l in m.model] == want["layers"]
    assert list(m.state_dict()) == gs.unpack_keys(want["keys"])
    assert guess_model_task(name) == "detect" and guess_model_task(m) == "detect"
    head = m.model[-1]
    suffix = name[len("yolov8") + 1:-len(".yaml")]
    assert type(head).__name__ == "Detect" and head.legacy is want["legacy"] and head.nl == gs.NL[suffix] == len(want["stride"])
    first = {"-p2": 4.0, "-ghost-p2": 4.0}.get(suffix, 8.0)
    assert want["stride"] == [first * 2 ** i for i in range(head.nl)]


def test_every_file_resolves_through_the_facade():
    from edge_yolo_amd import YOLO
    for name in ("yolov8n.yaml", "yolov8s-ghost-p6.yaml", "yolov8m-p2.yaml", "yolov8n-ghost.yaml", "yolov8n-ghost-p2.yaml", "yolov8n-p6.yaml"):
        y = YOLO(name)
        assert y.task == "detect" and type(y.model).__name__ == "DetectionModel"


@pytest.mark.parametrize("scale", list(gs.HIDDEN))
def test_hidden_widths_of_the_pointwise_ghostconvs(scale):
    """Hidden widths that are multiples of 4 and no multiples of 8 exist at the n, m and x scales; every input width is a multiple of 8."""
    from edge_yolo_amd.nn.modules import GhostConv
    from edge_yolo_amd.nn.tasks import DetectionModel
    for suffix in ("-ghost", "-ghost-p2"):
        m = DetectionModel(f"yolov8{scale}{suffix}.yaml")
        pw = [g for g in m.modules() if isinstance(g, GhostConv) and g.cv1.conv.kernel_size == (1, 1)]
        assert pw and all(g.cv1.conv.stride == (1, 1) and g.cv1.conv.groups == 1 and g.cv2.conv.kernel_size == (5, 5) for g in pw)
        assert sorted({g.cv1.conv.out_channels for g in pw}) == gs.HIDDEN[scale]
        assert all(g.cv1.conv.in_channels % 8 == 0 for g in pw)
        assert any(g.cv1.conv.out_channels % 8 == 4 for g in pw)
    if scale == "n":
        m = DetectionModel("yolov8n-ghost-p6.yaml")
        assert sorted({g.cv1.conv.out_channels for g in m.modules() if isinstance(g, GhostConv) and g.cv1.conv.kernel_size == (1, 1)}) == gs.HIDDEN_P6_N


def test_the_graph_knows_that_a_strided_ghostconv_halves_the_map():
    from edge_yolo_amd.nn.tasks import DetectionModel
    m = DetectionModel("yolov8n-ghost-p6.yaml")
    assert [m._down[i] for i in (0, 1, 3, 5, 7, 9, 11)] == [2.0, 4.0, 8.0, 16.0, 32.0, 64.0, 64.0]


def test_module_keys_match_reference(ops_golden):
    from edge_yolo_amd.nn import modules as M
    for tag, cls, args, kw, _ in gs.MODULE_CASES:
        assert list(getattr(M, cls)(*args, **kw).state_dict()) == list(ops_golden[tag + "_keys"]), tag


def test_golden_rows_are_separated(golden_dir):
    """What the generator asserted on the reference alone, re-checked on the recorded rows: per image at least 5 kept rows, their scores more
    than 1e-3 apart, and no candidate's best score within 1e-3 of conf."""
    for tag, (name, shape, *_) in gs.MODEL_CASES.items():
        g = np.load(os.path.join(golden_dir, tag + ".npz"))
        suffix = name[len("yolov8") + 1:-len(".yaml")]
        assert g["y"].shape[0] == shape[0] and sum(f"raw{i}" in g for i in range(5)) == gs.NL[suffix]
        for i in range(shape[0]):
            n, gap, margin = gs.kept_rows_separated(g["y"][i], g[f"det{i}"], float(g["conf"]))
            assert n == len(g[f"det{i}"]) >= gs.MIN_ROWS and gap > gs.ROW_GAP and margin > gs.ROW_GAP
