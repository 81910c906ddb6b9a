"""YOLOv10 without a GPU: structure, state_dict keys and parameter counts of the six model files against the reference
(tests/golden/structure_v10.json), guess_model_task, the head's legacy / end2end flags, scale resolution (the `b` file, an unknown scale),
RepVGGDW's fuse() and its folded 7x7 kernel in float64 against the reference's unfused output (tests/golden/v10_ops.npz) at the fp32 layer
bar of tests/test_gpu_v10_model.py (rtol 1e-4, atol 2e-4)."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import v10_synth as vs

LAYER_TOL = dict(rtol=1e-4, atol=2e-4)


@pytest.fixture(scope="module")
def structure(golden_dir):
    with open(os.path.join(golden_dir, "structure_v10.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def ops_golden(golden_dir):
    return np.load(os.path.join(golden_dir, "v10_ops.npz"))


@pytest.mark.parametrize("name", vs.FILES)
def test_structure_matches_reference(structure, name):
    from edge_yolo_amd import YOLO
    from edge_yolo_amd.nn.tasks import DetectionModel, guess_model_task
    want = structure[name]
    m = DetectionModel(name)
    assert sum(p.numel() for p in m.parameters()) == want["params"]
    if name in vs.PARAMS:
        assert want["params"] == vs.PARAMS[name]
    assert list(m.save) == want["save"]
    assert [float(s) for s in m.stride] == want["stride"]
    assert [dict(i=l.i, f=l.f, type=l.type, np=int(l.np)) for l in m.model] == want["layers"]
    assert list(m.state_dict()) == vs.unpack_keys(want["keys"])
    assert guess_model_task(name) == "detect" and guess_model_task(m) == "detect"
    head = m.model[-1]
    assert type(head).__name__ == "v10Detect" and head.legacy is False and want["legacy"] is False
    assert head.end2end is True and want["end2end"] is True and m.end2end is True
    y = YOLO(name)
    assert y.task == "detect" and type(y.model).__name__ == "DetectionModel"


def test_scdown_layers_and_their_widths():
    """The (C1, C2) pairs the SCDown layers see, per scale: what the fused kernel's gate has to admit."""
    from edge_yolo_amd.nn.tasks import DetectionModel
    want = {"n": [(64, 128), (128, 256), (128, 128)], "s": [(128, 256), (256, 512), (256, 256)], "m": [(192, 384), (384, 576), (384, 384)],
            "b": [(256, 512), (512, 512), (512, 512)], "l": [(256, 512), (512, 512), (512, 512)], "x": [(320, 640), (640, 640), (640, 640)]}
    for s, pairs in want.items():
        m = DetectionModel(f"yolov10{s}.yaml")
        got = [(l.i, l.cv1.conv.in_channels, l.cv1.conv.out_channels) for l in m.model if type(l).__name__ == "SCDown"]
        assert got == [(i, a, b) for i, (a, b) in zip((5, 7, 20), pairs)]
        assert all(b % 64 == 0 and a % 8 == 0 for a, b in pairs)
        assert [m._down[i] for i in (4, 5, 7, 20)] == [8.0, 16.0, 32.0, 32.0]  # the graph knows that SCDown halves the map


def test_b_file_resolves_its_scale_and_an_unknown_scale_raises():
    from edge_yolo_amd.nn.tasks import DetectionModel, guess_model_scale, yaml_model_load
    assert guess_model_scale("yolov10b.yaml") == ""  # no letter of [nslmx]: the empty scale falls to the file's only entry
    d = yaml_model_load("yolov10b.yaml")
    assert d["scale"] == "" and list(d["scales"]) == ["b"]
    m = DetectionModel(d)
    assert m.model[0].conv.out_channels == 64 and m.model[7].cv1.conv.out_channels == 512  # width 1.0, max 512
    d = yaml_model_load("yolov10n.yaml")
    d["scale"] = "q"
    with pytest.raises(KeyError, match="scale 'q'"):
        DetectionModel(d)


def test_psa_head_counts():
    from edge_yolo_amd.nn.tasks import DetectionModel
    for s, (c, heads, hd, kd) in {"n": (128, 2, 64, 32), "m": (288, 4, 72, 36), "x": (320, 5, 64, 32)}.items():
        a = DetectionModel(f"yolov10{s}.yaml").model[10].attn
        assert (a.qkv.conv.in_channels, a.num_heads, a.head_dim, a.key_dim) == (c, heads, hd, kd)


def test_fuse_leaves_repvggdw_with_one_conv(structure):
    from edge_yolo_amd.nn.modules import RepVGGDW
    from edge_yolo_amd.nn.tasks import DetectionModel
    m = DetectionModel("yolov10n.yaml")
    m.load_state_dict(vs.model_weights("yolov10n_64x96", m.state_dict()))
    reps = [mod for mod in m.modules() if isinstance(mod, RepVGGDW)]
    assert len(reps) == 1 and [k for k in reps[0].state_dict() if k.startswith("conv1.")]
    before = [r.folded() for r in reps]
    m.fuse()
    for r, (w, b) in zip(reps, before):
        assert list(r.state_dict()) == ["conv.weight", "conv.bias"] and not hasattr(r, "conv1") and isinstance(r.conv, torch.nn.Conv2d)
        assert tuple(r.conv.weight.shape) == (r.dim, 1, 7, 7) and r.conv.groups == r.dim and r.conv.padding == (3, 3)
        # fuse() visited it while its inner Convs still carried their BatchNorm: the single conv is the fold of both branches
        assert torch.equal(r.conv.weight, w) and torch.equal(r.conv.bias, b)
        w2, b2 = r.folded()
        assert torch.equal(w2, w) and torch.equal(b2, b)
    assert m.convs_folded()
    m.fuse()  # idempotent


def test_repvggdw_folded_kernel_fp64_vs_reference(ops_golden):
    from edge_yolo_amd.nn.modules import RepVGGDW
    tag, _, args, kw, shape = next(c for c in vs.MODULE_CASES if c[0] == "repvggdw")
    m = RepVGGDW(*args, **kw).eval()
    for mod in m.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.eps = 1e-3
    m.load_state_dict(vs.state_dict(m.state_dict(), prefix=tag + "."))
    assert list(m.state_dict()) == list(ops_golden[tag + "_keys"])
    x = vs.case_input(tag, shape).double()

    def run(mod):
        w, b = mod.folded()
        assert tuple(w.shape) == (args[0], 1, 7, 7)
        return F.silu(F.conv2d(x, w.double(), b.double(), stride=1, padding=3, groups=args[0])).numpy()

    got = run(m)
    print(f"repvggdw folded 7x7 in fp64 vs the reference's two branches: max abs err {float(np.abs(got - ops_golden[tag + '_y']).max()):.3e}")
    np.testing.assert_allclose(got, ops_golden[tag + "_y"], **LAYER_TOL)
    m.fuse()
    assert list(m.state_dict()) == list(ops_golden[tag + "_fused_keys"]) == ["conv.weight", "conv.bias"]
    np.testing.assert_allclose(run(m), ops_golden[tag + "_y"], **LAYER_TOL)
    np.testing.assert_allclose(run(m), ops_golden[tag + "_fused_y"], **LAYER_TOL)


def test_module_keys_match_reference(ops_golden):
    from edge_yolo_amd.nn import modules as M
    for tag, cls, args, kw, _ in vs.MODULE_CASES:
        assert list(getattr(M, cls)(*args, **kw).state_dict()) == list(ops_golden[tag + "_keys"]), tag


def test_golden_rows_are_separated(golden_dir):
    """What the generator asserted on the reference alone, re-checked on the recorded rows: per image the scores at or above conf, and the
    one after them, are more than 1e-3 apart, and at least 5 rows pass."""
    for tag in vs.MODEL_CASES:
        g = np.load(os.path.join(golden_dir, tag + ".npz"))
        for i in range(g["y"].shape[0]):
            n, gap = vs.separated_rows(g["y"][i, :, 4], float(g["conf"]))
            assert n >= vs.MIN_ROWS and gap > vs.ROW_GAP and len(g[f"det{i}"]) == n


def test_other_end2end_heads_still_raise():
    from edge_yolo_amd.nn import modules as M
    for cls, args in ((M.Segment, (80, 32, 64, (32, 64))), (M.OBB, (80, 1, (32, 64))), (M.Pose, (80, (17, 3), (32, 64)))):
        head = cls(*args).eval()
        head.end2end = True
        head.stride = torch.tensor([8.0, 16.0])
        with pytest.raises(NotImplementedError, match="end2end"):
            head([torch.zeros(1, 32, 4, 4), torch.zeros(1, 64, 2, 2)])
