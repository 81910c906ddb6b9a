"""CPU checks of the segment task: registry / structure / state_dict keys of yolo11{n,s,m,l,x}-seg.yaml against what the reference builds
(tests/golden/structure_seg.json), the swapped-head dict config, guess_model_task, the refusals, the host side of the weight packer, and the
float64 restatement (tests/fp64_mask_ref.py) against the reference's own process_mask results (tests/golden/seg_ops.npz)."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import edge_yolo_amd
from edge_yolo_amd import _lib as L
from edge_yolo_amd.engine.results import Masks, Results
from edge_yolo_amd.nn import modules as M
from edge_yolo_amd.nn.tasks import DetectionModel, SegmentationModel, guess_model_task, yaml_model_load
from edge_yolo_amd.utils import ops as uops
import fp64_mask_ref as f64
import seg_synth


@pytest.fixture(scope="module")
def structure(golden_dir):
    return json.load(open(os.path.join(golden_dir, "structure_seg.json")))


@pytest.fixture(scope="module")
def seg_ops(golden_dir):
    return np.load(os.path.join(golden_dir, "seg_ops.npz"))


@pytest.mark.parametrize("scale", list(seg_synth.SCALES))
def test_registry_builds_the_reference_graph(structure, scale):
    name = seg_synth.NAME.format(scale)
    want = structure[name]
    m = SegmentationModel(name)
    assert sum(p.numel() for p in m.parameters()) == want["params"]
    assert list(m.save) == want["save"] and [float(s) for s in m.stride] == want["stride"]
    got = [dict(i=l.i, f=l.f, type=l.type, np=int(l.np)) for l in m.model]
    assert got == want["layers"]
    assert list(m.state_dict()) == want["keys"]
    head = m.model[-1]
    assert isinstance(head, M.Segment) and isinstance(head.proto, M.Proto) and dict(nm=head.nm, npr=head.npr) == want["head"]
    assert isinstance(head.proto.upsample, torch.nn.ConvTranspose2d) and len(head.cv4) == 3


def test_n_scale_parameter_count(structure):
    assert structure["yolo11n-seg.yaml"]["params"] == 2876848


def test_guess_model_task_and_facade():
    assert guess_model_task("yolo11n-seg.yaml") == "segment" and guess_model_task(yaml_model_load("yolo11s-seg.yaml")) == "segment"
    assert guess_model_task("yolo11n.yaml") == "detect" and guess_model_task("yolo11n-test.yaml") == "detect"
    y = edge_yolo_amd.YOLO("yolo11n-seg.yaml")
    assert y.task == "segment" and isinstance(y.model, SegmentationModel) and guess_model_task(y.model) == "segment"
    assert set(y.task_map) == {"detect", "segment"} and y.task_map["segment"]["model"] is SegmentationModel
    assert y.task_map["segment"]["predictor"].__name__ == "SegmentationPredictor"
    assert guess_model_task(DetectionModel("yolo11n.yaml")) == "detect"
    with pytest.raises(ValueError):
        edge_yolo_amd.YOLO("yolo11n-seg.yaml", task="detect")


def test_segment_row_on_another_backbone(golden_dir):
    """A Segment row on the EdgeLine graph (dict config): builds, and its keys are the detect model's minus the GFL head's plus Segment's."""
    d = seg_synth.edgeline_seg_cfg(yaml_model_load("yolo11n-test.yaml"))
    m = SegmentationModel(d)
    head = m.model[-1]
    assert isinstance(head, M.Segment) and head.nm == 32 and head.npr == 64 and [float(s) for s in m.stride] == [8.0, 16.0, 32.0]
    g = np.load(os.path.join(golden_dir, "edgeline_n_seg_64.npz"))
    assert g["mc"].shape == (2, 32, 84) and g["p"].shape == (2, 32, 16, 16)
    assert edge_yolo_amd.YOLO(d).task == "segment"


def test_module_keys_match_the_reference(seg_ops):
    for tag, args, _ in seg_synth.PROTO_CASES:
        assert list(M.Proto(*args).state_dict()) == list(seg_ops[tag + "_keys"])
    tag, kw, _ = seg_synth.SEGMENT_CASE
    M.Segment.legacy = False
    assert list(M.Segment(**kw).state_dict()) == list(seg_ops[tag + "_keys"])


def test_refusals():
    y = edge_yolo_amd.YOLO("yolo11n-seg.yaml")
    x = torch.zeros(1, 3, 64, 64)
    with pytest.raises(NotImplementedError, match="retina_masks"):
        y.predict(x, retina_masks=True)
    with pytest.raises(NotImplementedError, match="predict_batches"):
        next(iter(y.predict_batches([x])))
    with pytest.raises(TypeError):  # (the detect task does not know the argument at all: unchanged)
        edge_yolo_amd.YOLO("yolo11n.yaml").predict(x, retina_masks=True)
    mk = Masks(torch.zeros(2, 8, 12, dtype=torch.uint8), (8, 12))
    assert mk.data.dtype == torch.bool and tuple(mk.shape) == (2, 8, 12) and len(mk) == 2 and mk.orig_shape == (8, 12)
    assert mk.cpu().data.dtype == torch.bool and mk.numpy().data.dtype == np.bool_
    for prop in ("xy", "xyn"):
        with pytest.raises(NotImplementedError):
            getattr(mk, prop)
    r = Results(None, path="a.jpg", names={0: "0"}, boxes=torch.zeros(2, 6), masks=torch.ones(2, 4, 4, dtype=torch.uint8))
    assert len(r.masks) == 2 and bool(r.masks.data.all())
    assert Results(None, path="a.jpg", names={0: "0"}, boxes=torch.zeros(0, 6)).masks is None


def test_process_mask_symbols_and_host_side_refusals():
    """Every new entry is exported; the argument checks that run before any launch answer on a host without a GPU."""
    lib = L.lib()
    for name in ("ey_process_mask", "ey_deconv2x2", "ey_deconv2x2_pack_weight", "ey_deconv2x2_packed_bytes"):
        assert hasattr(lib, name)
    one = (ctypes.c_void_p * 1)(8)
    ia = (ctypes.c_int * 1)(8)
    for kw in (dict(s=3), dict(nm=12), dict(nl=5)):
        s, nm, nl = kw.get("s", 4), kw.get("nm", 8), kw.get("nl", 1)
        code = lib.ey_process_mask(L.F32, 1, 2, 2, nm, 8, nm, nl, one, L.F32, ia, ia, ia, 1, 8, 8, s, 8, None)
        assert code == -2, kw
    assert lib.ey_process_mask(L.F32, 1, 2, 2, 8, 8, 8, 1, one, L.F32, ia, ia, ia, 0, None, None, 4, None, None) == 0  # N = 0


def test_deconv_pack_layout():
    """ey_deconv2x2_pack_weight: row order of the packed [4 Cout][Cin] matrix as csrc/segment.hip documents it."""
    cin, cout = 16, 24
    w = torch.arange(cin * cout * 4, dtype=torch.float32).view(cin, cout, 2, 2).contiguous()
    nb = L.lib().ey_deconv2x2_packed_bytes(L.F32, cin, cout)
    assert nb == 4 * cout * cin * 4
    buf = torch.empty(nb, dtype=torch.uint8)
    L.check(L.lib().ey_deconv2x2_pack_weight(L.F32, cin, cout, w.data_ptr(), buf.data_ptr(), nb), "pack")
    got = buf.view(torch.float32).view(4 * cout, cin)
    for row in range(4 * cout):
        p, t, i = row // 32, (row % 32) // 16, row % 16
        q = 32 * p + 8 * (i // 4) + 4 * t + i % 4
        d, co = q // cout, q % cout
        assert torch.equal(got[row], w[:, co, d // 2, d % 2]), row
    assert L.lib().ey_deconv2x2_pack_weight(L.F32, 12, cout, w.data_ptr(), buf.data_ptr(), nb) == -1


@pytest.mark.parametrize("case", seg_synth.PM_GOLDEN, ids=[c[0] for c in seg_synth.PM_GOLDEN])
def test_fp64_restatement_equals_the_reference_bits(seg_ops, case):
    """The reference's fp32 process_mask decides every pixel of these cases as the float64 restatement does, outside the derived bound,
    and at most one of their in-box pixels lies inside it.  Its pre-threshold values stay within the bound of the float64 values."""
    tag, s, half, nm = case[0], case[1], case[2], case[3]
    protos, coef, boxes, shape = seg_synth.pm_golden_case(*case)
    ref = f64.process_mask64(protos, coef, boxes, s)
    assert ref["bits"].shape == seg_ops[tag + "_bits"].shape
    und, tot = f64.check_bits(seg_ops[tag + "_bits"], ref, nm)
    assert tot > 0 and und <= 1  # (one pixel of pm_s4_f32 has |v| inside the bound; check_bits holds the 1e-3 cap)
    assert (np.abs(seg_ops[tag + "_pre"].astype(np.float64) - ref["v"]) <= f64.mask_bound(ref, nm)).all()
    if s > 1:  # upsample=False is the s = 1 form on boxes scaled by 1/s
        low = f64.process_mask64(protos, coef, boxes * np.float32(1.0 / s), 1)
        np.testing.assert_array_equal(seg_ops[tag + "_bits_lowres"], low["bits"])


def test_crop_mask_is_the_reference_rule():
    m = torch.ones(2, 4, 6)
    b = torch.tensor([[1.0, 0.0, 3.0, 2.0], [0.5, 1.5, 2.5, 4.0]])
    got = uops.crop_mask(m, b)
    want = torch.zeros(2, 4, 6)
    want[0, 0:2, 1:3] = 1
    want[1, 2:4, 1:3] = 1
    assert torch.equal(got, want)


def test_deconv64_is_conv_transpose():
    r = np.random.default_rng(3)
    x, w, b = r.normal(size=(2, 8, 3, 5)), r.normal(size=(8, 16, 2, 2)), r.normal(size=16)
    y, mag = f64.deconv64(x, w, b)
    want = torch.nn.functional.conv_transpose2d(torch.tensor(x), torch.tensor(w), torch.tensor(b), stride=2)
    np.testing.assert_allclose(y, want.numpy(), rtol=1e-12, atol=1e-12)
    assert (mag >= np.abs(y) - 1e-12).all()
