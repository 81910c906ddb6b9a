"""YOLOv13-LGL (DSC3K2_LGL: a Local-Global-Local transformer block behind every DS unit) without a GPU: YAML resolution, the layer
table, parameter counts, `save` and ordered state_dict keys of all four scales against the reference
(tests/golden/structure_v13_lgl.json, make_golden_v13_lgl.py), module-level keys, strides, the head-count rule, and refusals."""
import json
import os

import numpy as np
import pytest
import torch

import lgl_synth

NAME = "yolov13{}-DSC3K2_LGL.yaml"
LGL_LAYERS = (2, 4, 17, 21, 26, 30)


@pytest.fixture(scope="module")
def E():
    import edge_yolo_amd
    return edge_yolo_amd


@pytest.fixture(scope="module")
def structure(golden_dir):
    return json.load(open(os.path.join(golden_dir, "structure_v13_lgl.json")))


@pytest.mark.parametrize("scale", "nslx")
def test_yolo_builds(E, scale):
    model = E.YOLO(NAME.format(scale))
    for i in LGL_LAYERS:
        assert type(model.model.model[i]).__name__ == "DSC3K2_LGL"
    assert type(model.model.model[9]).__name__ == "HyperACE"
    assert [float(s) for s in model.model.stride] == [8.0, 16.0, 32.0]


def test_no_m_scale(E):
    from edge_yolo_amd.nn.tasks import DetectionModel
    with pytest.raises(KeyError, match="scale 'm' is not defined"):
        DetectionModel(NAME.format("m"))


@pytest.mark.parametrize("scale", "nslx")
def test_structure_matches_reference(E, structure, scale):
    from edge_yolo_amd.nn.tasks import DetectionModel
    want = structure[NAME.format(scale)]
    m = DetectionModel(NAME.format(scale))
    got = [dict(i=l.i, f=l.f, type=l.type, np=int(l.np)) for l in m.model]
    assert got == want["layers"]
    assert sum(p.numel() for p in m.parameters()) == want["params"]
    assert list(m.save) == want["save"]
    assert list(m.state_dict()) == want["keys"]


@pytest.mark.parametrize("scale,params,keys", [("n", 2790029, 1010), ("l", 31815955, 1664)])
def test_parameter_counts(E, scale, params, keys):
    from edge_yolo_amd.nn.tasks import DetectionModel
    m = DetectionModel(NAME.format(scale))
    assert sum(p.numel() for p in m.parameters()) == params
    assert len(m.state_dict()) == keys


@pytest.mark.parametrize("scale", "nslx")
def test_head_rule(E, structure, scale):
    """heads = max(1, c // 64), or the divisor of c nearest to it; sr_ratio 2, mlp_ratio 4, qkv bias; units per block = the repeats."""
    from edge_yolo_amd.nn.tasks import DetectionModel
    m = DetectionModel(NAME.format(scale))
    want = structure[NAME.format(scale)]["heads"]
    for i in LGL_LAYERS:
        blk = m.model[i]
        assert len(blk.m) == (1 if scale in "ns" else 2)
        heads = []
        for u in blk.m:
            sa = u.lgl.lgl.SelfAttn
            c = sa.norm1.normalized_shape[0]
            assert c == blk.c and c % sa.attn.num_heads == 0
            cand = max(1, c // 64)
            if c % cand:
                cand = min((d for d in range(1, c + 1) if c % d == 0), key=lambda d: abs(d - cand))
            assert sa.attn.num_heads == cand
            assert sa.attn.sr == 2 and sa.attn.qkv.bias is not None and sa.mlp.fc1.out_features == 4 * c
            assert u.lgl.lgl.LocalAgg.mlp.fc1.out_channels == 4 * c
            assert tuple(u.lgl.gamma.shape) == (1,) and float(u.lgl.gamma.detach()) == 0.0
            heads.append(sa.attn.num_heads)
        assert heads == want[str(i)]
    if scale == "n":
        assert [m.model[i].c for i in LGL_LAYERS] == [16, 32, 64, 32, 64, 128]
        assert [m.model[i].m[0].lgl.lgl.SelfAttn.attn.num_heads for i in LGL_LAYERS] == [1, 1, 1, 1, 1, 2]


def test_module_keys_match_reference(E, golden_dir):
    from edge_yolo_amd.nn.modules import block
    g = np.load(os.path.join(golden_dir, "v13_lgl_ops.npz"))
    seen = set()
    for tag, prefix, cls, args, kw, shape, lgl in lgl_synth.CASES:
        if prefix in seen:
            continue
        seen.add(prefix)
        mod = getattr(block, cls)(*args, **kw)
        assert sorted(mod.state_dict()) == list(g[prefix + "_keys"]), prefix
    keys = list(block.DSC3K2_LGL(32, 64, 1, False, 0.25).state_dict())
    for want in ("cv1.conv.weight", "cv2.bn.running_var", "m.0.core.ds1.dw.weight", "m.0.core.ds2.pw.weight", "m.0.core.ds2.bn.bias", "m.0.lgl.gamma",
                 "m.0.lgl.lgl.LocalAgg.pos_embed.bias", "m.0.lgl.lgl.LocalAgg.norm1.running_mean", "m.0.lgl.lgl.LocalAgg.mlp.fc2.weight",
                 "m.0.lgl.lgl.SelfAttn.attn.qkv.bias", "m.0.lgl.lgl.SelfAttn.attn.LocalProp.weight", "m.0.lgl.lgl.SelfAttn.attn.norm.weight",
                 "m.0.lgl.lgl.SelfAttn.mlp.fc1.weight"):
        assert want in keys, want


def test_reference_state_dict_loads(E, structure):
    """A state_dict with exactly the reference's keys and shapes loads strictly, and the synthetic LGL statistics are usable: every
    running_var and norm weight of an LGL block is positive (plain synthdata would draw them from N(0, 0.1))."""
    from edge_yolo_amd.nn.tasks import DetectionModel
    m = DetectionModel(NAME.format("n"))
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert list(shapes) == structure[NAME.format("n")]["keys"]
    sd = lgl_synth.state_dict(shapes)
    m.load_state_dict(sd, strict=True)
    for k, v in sd.items():
        if ".lgl." in k and (k.endswith("running_var") or k.rsplit(".", 2)[-2] in ("norm", "norm1", "norm2") and k.endswith(".weight")):
            assert float(v.min()) >= 0.5, k


def test_refusals(E):
    from edge_yolo_amd.nn.modules import block
    with pytest.raises(NotImplementedError, match="sr_ratio 1 and 2"):
        block.GlobalSparseAttn(32, 1, sr_ratio=4)
    with pytest.raises(NotImplementedError, match="exact GELU"):
        block.Mlp(16, 64, act_layer=torch.nn.ReLU)
    with pytest.raises(NotImplementedError, match="nn.LayerNorm"):
        block.SelfAttn(32, 1, norm_layer=torch.nn.BatchNorm1d)
    sa = block.SelfAttn(128, 2, sr_ratio=1)  # sr_ratio 1: no pool, no un-pool, no LocalAgg
    assert isinstance(sa.attn.LocalProp, torch.nn.Identity) and isinstance(block.LGLBlock(32, 1).LocalAgg, torch.nn.Identity)
    assert block._LGLAdapter(48, num_heads=5).lgl.SelfAttn.attn.num_heads in (4, 6)  # nearest divisor
