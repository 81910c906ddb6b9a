"""YOLOv13 (HyperACE / FullPAD / DSC3K2 / stride-2 DSConv) without a GPU: YAML resolution, the layer table, parameter counts and
state_dict keys of all four scales against the reference (tests/golden/structure_v13.json, make_golden_v13.py), the parse rules
(hyperedges, channel_adjust, DownsampleConv widths), graph strides, and refusals."""
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
    return json.load(open(os.path.join(golden_dir, "structure_v13.json")))


@pytest.mark.parametrize("scale", "nslx")
def test_yolo_builds(E, scale):
    model = E.YOLO(f"yolov13{scale}.yaml")
    assert type(model.model.model[9]).__name__ == "HyperACE"
    assert [float(s) for s in model.model.stride] == [8.0, 16.0, 32.0]


def test_no_m_scale(E):
    from edge_yolo_amd.nn.tasks import DetectionModel
    with pytest.raises(KeyError, match="scale 'm' is not defined"):
        DetectionModel("yolov13m.yaml")


@pytest.mark.parametrize("scale", "nslx")
def test_structure_matches_reference(E, structure, scale):
    from edge_yolo_amd.nn.tasks import DetectionModel
    name = f"yolov13{scale}.yaml"
    want = structure[name]
    m = DetectionModel(name)
    got = [dict(i=l.i, f=l.f, type=l.type, np=int(l.np)) for l in m.model]
    assert got == want["layers"]
    assert sum(p.numel() for p in m.parameters()) == want["params"]
    assert list(m.save) == want["save"]
    assert list(m.state_dict()) == want["keys"]


@pytest.mark.parametrize("scale,params", [("n", 2494151), ("s", 9055527), ("l", 27627783), ("x", 64057511)])
def test_parameter_counts(E, scale, params):
    from edge_yolo_amd.nn.tasks import DetectionModel
    assert sum(p.numel() for p in DetectionModel(f"yolov13{scale}.yaml").parameters()) == params


@pytest.mark.parametrize("scale,he,adjust,D,ds_c", [("n", 4, True, 64, (128, 256)), ("s", 8, True, 128, (256, 512)), ("l", 8, False, 256, (512, 512)),
                                                   ("x", 12, False, 384, (768, 768))])
def test_parse_rules(E, scale, he, adjust, D, ds_c):
    """Hyperedges int(8 * 0.5) for n and int(8 * 1.5) for x; channel_adjust=False for l/x (FuseModule 3c -> c, DownsampleConv keeps c);
    the C3AH width D = c2 / 2 with 16-channel heads; DSC3K2 forced to dsc3k for l/x."""
    from edge_yolo_amd.nn.modules import DSBottleneck, DSC3K2, DSC3k
    from edge_yolo_amd.nn.tasks import DetectionModel
    m = DetectionModel(f"yolov13{scale}.yaml")
    h = m.model[9]
    for br in (h.branch1, h.branch2):
        g = br.m.hgnn.edge_generator
        assert g.num_hyperedges == he and g.num_heads == D // 16 and g.head_dim == 16
        assert tuple(g.prototype_base.shape) == (he, D)
    c_in = h.fuse.conv_out.conv.out_channels
    assert h.fuse.conv_out.conv.in_channels == (4 if adjust else 3) * c_in
    ds = m.model[11]
    assert isinstance(ds.channel_adjust, torch.nn.Identity) != adjust
    assert (m.model[9].cv2.conv.out_channels, m.model[14].gate.shape) == (ds_c[0], torch.Size([]))
    if adjust:
        assert ds.channel_adjust.conv.out_channels == ds_c[1]
    for i in (2, 4):
        assert isinstance(m.model[i], DSC3K2)
        assert all(isinstance(b, DSC3k if scale in "lx" else DSBottleneck) for b in m.model[i].m)


def test_module_keys_match_reference(E, golden_dir):
    from edge_yolo_amd.nn import modules as M
    from edge_yolo_amd.nn.modules.conv import DSConv
    g = np.load(os.path.join(golden_dir, "v13_ops.npz"))
    for tag, mod in (("hgc_d64_e4", M.AdaHGComputation(64, 4, 4)), ("hgc_d128_e12_mean", M.AdaHGComputation(128, 12, 8, 0.1, "mean")),
                     ("c3ah", M.C3AH(64, 64, 1.0, 8)), ("fuse_adj", M.FuseModule(32, True)), ("fuse_noadj", M.FuseModule(32, False)),
                     ("hyperace_n1", M.HyperACE(32, 64, 1, 4, True, True, 0.5, 1, "both", True)),
                     ("hyperace_n2", M.HyperACE(32, 64, 2, 8, True, True, 0.5, 1, "both", False)),
                     ("hyperace_dsb", M.HyperACE(32, 64, 1, 4, False, False, 0.5, 1, "both", False)),
                     ("down_adj", M.DownsampleConv(32, True)), ("down_noadj", M.DownsampleConv(32, False)), ("fullpad", M.FullPAD_Tunnel()),
                     ("dsconv_s2_odd", DSConv(32, 48, 3, 2)), ("dsc3k2_dsb", M.DSC3K2(64, 64, 1, False)), ("dsc3k2_dsc3k", M.DSC3K2(64, 64, 1, True)),
                     ("hgconv_tokens", M.AdaHGConv(64, 8, 4))):
        assert sorted(mod.state_dict()) == list(g[tag + "_keys"]), tag


def test_reference_state_dict_loads(E, golden_dir):
    """A state_dict with exactly the reference's keys and shapes loads strictly (no missing / unexpected keys)."""
    from edge_yolo_amd.nn.tasks import DetectionModel
    want = json.load(open(os.path.join(golden_dir, "structure_v13.json")))["yolov13n.yaml"]["keys"]
    m = DetectionModel("yolov13n.yaml")
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    assert list(sd) == want
    m2 = DetectionModel("yolov13n.yaml")
    m2.load_state_dict(sd, strict=True)


def test_refusals(E):
    from edge_yolo_amd.nn.modules import AdaHyperedgeGen, C3AH
    from edge_yolo_amd.nn.modules.conv import DSConv
    with pytest.raises(ValueError, match="Unsupported context"):
        AdaHyperedgeGen(64, 4, 4, context="sum")
    with pytest.raises(AssertionError, match="multiple of 16"):
        C3AH(40, 40)
    with pytest.raises(NotImplementedError, match="inside AdaHGConv"):
        AdaHyperedgeGen(64, 4, 4)(torch.zeros(1, 5, 64))
    with pytest.raises(NotImplementedError, match="stride other than 1 and 2"):
        DSConv(16, 16, 3, 3)(torch.zeros(1, 16, 8, 8))
