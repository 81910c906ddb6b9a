"""YOLOv12 (A2C2f / ABlock / AAttn) without a GPU: YAML resolution, the layer table, parameter counts and state_dict keys of all
five scales against the reference (tests/golden/structure_v12.json, make_golden_v12.py), the l/x layer scale, and refusals."""
import json
import os

import numpy as np
import pytest
import torch


@pytest.fixture(scope="module")
def E():
    import edge_yolo_amd
    return edge_yolo_amd


@pytest.fixture(scope="module")
def structure(golden_dir):
    return json.load(open(os.path.join(golden_dir, "structure_v12.json")))


@pytest.mark.parametrize("scale", "nl")
def test_yolo_builds(E, scale):
    model = E.YOLO(f"yolov12{scale}.yaml")
    assert type(model.model.model[6]).__name__ == "A2C2f"


@pytest.mark.parametrize("scale", "nslmx")
def test_structure_matches_reference(E, structure, scale):
    from edge_yolo_amd.nn.tasks import DetectionModel
    name = f"yolov12{scale}.yaml"
    want = structure[name]
    m = DetectionModel(name)
    got = [dict(i=l.i, f=l.f, type=l.type, np=int(l.np)) for l in m.model]
    assert got == want["layers"]
    assert sum(p.numel() for p in m.parameters()) == want["params"]
    assert list(m.save) == want["save"]
    assert list(m.state_dict()) == want["keys"]


@pytest.mark.parametrize("scale,has_gamma", [("n", False), ("s", False), ("m", False), ("l", True), ("x", True)])
def test_layer_scale_on_l_and_x(E, scale, has_gamma):
    from edge_yolo_amd.nn.modules import A2C2f
    from edge_yolo_amd.nn.tasks import DetectionModel
    m = DetectionModel(f"yolov12{scale}.yaml")
    blocks = {l.i: l for l in m.model if isinstance(l, A2C2f)}
    assert sorted(blocks) == [6, 8, 11, 14, 17]
    for i, b in blocks.items():
        a2 = i in (6, 8)
        assert (b.gamma is not None) == (a2 and has_gamma), i
        if b.gamma is not None:
            assert tuple(b.gamma.shape) == (b.cv2.conv.out_channels,)
    mlp = blocks[6].m[0][0].mlp[0].conv.out_channels
    assert mlp == int(blocks[6].cv1.conv.out_channels * (1.5 if has_gamma else 2.0))
    assert blocks[6].m[0][0].attn.area == 4 and blocks[8].m[0][0].attn.area == 1


def test_module_keys_match_reference(E, golden_dir):
    from edge_yolo_amd.nn.modules import A2C2f, AAttn, ABlock
    g = np.load(os.path.join(golden_dir, "v12_ops.npz"))
    for tag, mod in (("aattn_a4", AAttn(64, 2, 4)), ("ablock_a4", ABlock(64, 2, 1.2, 4)), ("a2c2f_a2", A2C2f(64, 64, 1, True, 4)),
                     ("a2c2f_c3k", A2C2f(64, 64, 2, False, -1)), ("a2c2f_res", A2C2f(64, 64, 1, True, 1, True, 1.5))):
        assert sorted(mod.state_dict()) == list(g[tag + "_keys"]), tag


def test_area_split_refused(E):
    """H*W % area != 0: the reference's reshape fails; here the module raises before anything runs."""
    from edge_yolo_amd.nn.modules import AAttn
    with pytest.raises(ValueError, match="equal areas"):
        AAttn(64, 2, 4)(torch.zeros(1, 64, 5, 5))


def test_grouped_conv_layers(E):
    from edge_yolo_amd.nn.tasks import DetectionModel
    m = DetectionModel("yolov12n.yaml")
    assert m.model[1].conv.groups == 2 and m.model[3].conv.groups == 4
