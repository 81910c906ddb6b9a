"""DySample and yolov13*-DySample.yaml without a GPU: YAML resolution, the layer table, parameter counts, `save` and ordered state_dict
keys of all four scales against the reference (tests/golden/structure_dysample.json, make_golden_dysample.py), init_pos, the 'pl' ->
dense weight expansion (the float64 pixel-space restatement of tests/fp64_dysample_ref.py fed the module's dense weights reproduces the
reference's 'lp' and 'pl' outputs), strides, and refusals."""
import json
import os

import numpy as np
import pytest
import torch

import dysample_synth
import fp64_dysample_ref as ref

NAME = dysample_synth.NAME


@pytest.fixture(scope="module")
def E():
    import edge_yolo_amd
    return edge_yolo_amd


@pytest.fixture(scope="module")
def structure(golden_dir):
    return json.load(open(os.path.join(golden_dir, "structure_dysample.json")))


@pytest.fixture(scope="module")
def ops_golden(golden_dir):
    return np.load(os.path.join(golden_dir, "dysample_ops.npz"))


@pytest.mark.parametrize("scale", "nslx")
def test_yolo_builds(E, scale):
    model = E.YOLO(NAME.format(scale))
    for i in dysample_synth.DYSAMPLE_LAYERS:
        m = model.model.model[i]
        assert type(m).__name__ == "DySample" and (m.scale, m.style, m.groups) == (2, "lp", 4) and not hasattr(m, "scope")
    assert not any(type(m).__name__ == "Upsample" for m in model.model.model)
    assert [float(s) for s in model.model.stride] == [8.0, 16.0, 32.0]


def test_layer_down_strides(E):
    """_layer_down divides by the DySample scale: 8 / 16 / 32 at the head, and the three DySample outputs sit at 8, 16, 8."""
    from edge_yolo_amd.nn.tasks import DetectionModel
    m = DetectionModel(NAME.format("n"))
    assert [m._down[j] for j in m.model[-1].f] == [8, 16, 32]
    assert [m._down[i] for i in dysample_synth.DYSAMPLE_LAYERS] == [8, 16, 8]
    assert not any(i in m._block_of for i in dysample_synth.DYSAMPLE_LAYERS)  # never part of a block program
    assert not any(m._block_single_ok(i) for i in dysample_synth.DYSAMPLE_LAYERS)


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
    for i in dysample_synth.DYSAMPLE_LAYERS:
        assert m.model[i].init_pos.flatten().tolist() == want["init_pos"][str(i)]


@pytest.mark.parametrize("scale,params,channels", [("n", 2510631, (128, 256, 128)), ("s", 9088391, (256, 512, 256)), ("l", 27677031, (512, 512, 512)),
                                                   ("x", 64131335, (768, 768, 768))])
def test_parameter_counts(E, scale, params, channels):
    """yolov13's count plus the three offset convs (C -> 32 with bias)."""
    from edge_yolo_amd.nn.tasks import DetectionModel
    m = DetectionModel(NAME.format(scale))
    assert sum(p.numel() for p in m.parameters()) == params
    assert tuple(m.model[i].in_channels for i in dysample_synth.DYSAMPLE_LAYERS) == channels
    base = DetectionModel(f"yolov13{scale}.yaml")
    assert params - sum(p.numel() for p in base.parameters()) == sum(32 * c + 32 for c in channels)


def test_module_keys_and_init_pos_match_reference(E, ops_golden):
    from edge_yolo_amd.nn.modules import DySample
    for tag, args, shape in dysample_synth.CASES:
        mod = DySample(*args)
        assert sorted(mod.state_dict()) == list(ops_golden[tag + "_keys"]), tag
        assert list(mod.state_dict()) == ["init_pos", "offset.weight", "offset.bias"] + (["scope.weight"] if args[4] else []), tag
        assert np.array_equal(mod.init_pos.numpy(), ops_golden[tag + "_init_pos"]), tag
        assert set(mod.init_pos.flatten().tolist()) == {-0.25, 0.25}
        want = dysample_synth.fill(mod, tag).init_pos  # the synthetic fill leaves the buffer alone
        assert np.array_equal(want.numpy(), ops_golden[tag + "_init_pos"]), tag


def test_reference_state_dict_loads(E, structure):
    from edge_yolo_amd.nn.tasks import DetectionModel
    m = DetectionModel(NAME.format("n"))
    assert list(m.state_dict()) == structure[NAME.format("n")]["keys"]
    sd = dysample_synth.state_dict(m.state_dict())
    m.load_state_dict(sd, strict=True)
    for i in dysample_synth.DYSAMPLE_LAYERS:
        assert torch.equal(m.model[i].init_pos, sd[f"model.{i}.init_pos"]) and m.model[i].init_pos.abs().eq(0.25).all()


def test_pl_to_dense_is_the_shuffled_conv(E):
    """W'[r 4 + q, c] = W[r, c // 4] [c % 4 == q]: the dense conv on x equals pixel_unshuffle(conv(pixel_shuffle(x))), in exact arithmetic
    on integer data."""
    from edge_yolo_amd.nn.modules.dysample import pl_to_dense
    g = torch.Generator().manual_seed(3)
    w = torch.randint(-4, 5, (8, 6), generator=g).double()
    b = torch.randint(-4, 5, (8,), generator=g).double()
    x = torch.randint(-4, 5, (2, 24, 3, 5), generator=g).double()
    wd, bd = pl_to_dense(w, b)
    assert tuple(wd.shape) == (32, 24) and tuple(bd.shape) == (32,)
    for r in range(8):
        for q in range(4):
            for c in range(24):
                assert wd[r * 4 + q, c] == (w[r, c // 4] if c % 4 == q else 0)
    F = torch.nn.functional
    want = F.pixel_unshuffle(F.conv2d(F.pixel_shuffle(x, 2), w.view(8, 6, 1, 1), b), 2)
    got = F.conv2d(x, wd.view(32, 24, 1, 1), bd)
    assert torch.equal(got, want)


@pytest.mark.parametrize("case", dysample_synth.CASES, ids=[c[0] for c in dysample_synth.CASES])
def test_fp64_restatement_reproduces_reference(E, ops_golden, case):
    """The module's dense weights ('pl': expanded) through the float64 pixel-space formula against the reference module's fp32 output:
    1e-5 (the reference's own fp32 rounding is 2.5e-6)."""
    from edge_yolo_amd.nn.modules import DySample
    tag, args, shape = case
    mod = dysample_synth.fill(DySample(*args), tag)
    x = torch.from_numpy(ops_golden[tag + "_x"])
    assert torch.equal(x, dysample_synth.case_input(shape))
    w, b, s = mod.dense_weights()
    assert tuple(w.shape) == (8 * args[3], args[0]) and (s is None) == (not args[4])
    y = ref.dysample(x, w, b, s, mod.init_pos, args[3])
    err = float((y - torch.from_numpy(ops_golden[tag]).double()).abs().max())
    print(f"{tag}: max |fp64 restatement - reference fp32| = {err:.2e}")
    assert err < 1e-5


def test_refusals(E):
    from edge_yolo_amd.nn.modules import DySample
    from edge_yolo_amd.nn.tasks import DetectionModel
    with pytest.raises(NotImplementedError, match="scale=3"):
        DySample(32, 3)
    with pytest.raises(NotImplementedError, match="groups=3"):
        DySample(36, 2, "lp", 3)
    with pytest.raises(AssertionError):
        DySample(32, 2, "xx")
    with pytest.raises(AssertionError):
        DySample(30, 2, "pl", 2)  # 'pl' needs C % 4 == 0
    with pytest.raises(AssertionError):
        DySample(36, 2, "lp", 8)  # C % groups
    with pytest.raises(KeyError, match="scale 'm' is not defined"):
        DetectionModel(NAME.format("m"))
