"""Masks at the original resolution without a GPU: the reference's process_mask_native bits (tests/golden/retina_ops.npz) meet the derived
criterion of tests/fp64_mask_native_ref.py -- which guards the float64 restatement and the bound that
tests/test_gpu_process_mask_native.py holds ey_process_mask_native to --, the crop records of the op cases, and the option plumbing."""
import os

import numpy as np
import pytest
import torch

import edge_yolo_amd
import fp64_mask_native_ref as f64
import retina_synth as rs
from edge_yolo_amd.engine.predictor import DetectionPredictor, FastSAMPredictor, RetinaMasksPredictor, SegmentationPredictor
from edge_yolo_amd.engine.validator import SegmentationValidator
from edge_yolo_amd.nn._ops import mask_geometry

GOLDEN = [c for c in rs.OP_CASES if c[5] > 0]


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "retina_ops.npz"))


def test_mask_geometry_of_the_cases():
    for c in rs.OP_CASES:
        assert mask_geometry(c[:2], c[2:4]) == (*rs.GEOMETRY[c[:4]], c[2], c[3]), c
    assert mask_geometry((1, 1), (5, 3))[:4] == (0, 1, 0, 0)  # an empty crop: the kernel refuses it, the reference's F.interpolate fails on it


@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("case", GOLDEN, ids=rs.case_id)
def test_reference_bits_meet_the_criterion(gold, case, half):
    protos, coef, boxes, shape = rs.golden_case(case, half)
    tag = rs.golden_tag(case, half)
    bits = rs.unpack(gold[tag + "_bits"], gold[tag + "_shape"])
    assert bits.shape == (len(coef), *shape)
    ref = f64.process_mask_native64(protos, coef, boxes, mask_geometry(protos.shape[1:], shape))
    und, tot = f64.check_bits(bits, ref, case[4])
    print(f"{tag}: undecided {und} of {tot} in-box pixels; set bits {int(bits.sum())}")
    assert tot > 0


def test_model_golden_meets_the_criterion(gold, golden_dir):
    g = np.load(os.path.join(golden_dir, "yolo11n_seg_64x96.npz"))
    det, p = g["det0"], g["p"][0]
    for h, w in rs.MODEL_SHAPES:
        tag = f"model_{h}x{w}"
        bits = rs.unpack(gold[tag + "_bits"], gold[tag + "_shape"])
        assert bits.shape == (len(det), h, w) and bits.any()
        ref = f64.process_mask_native64(p, det[:, 6:], gold[tag + "_boxes"], mask_geometry(p.shape[1:], (h, w)))
        f64.check_bits(bits, ref, 32)


def test_option_plumbing():
    """retina_masks is a constructor argument of SegmentationPredictor and the default of RetinaMasksPredictor, the class the facade is
    handed; the facade's own keyword keeps raising (tests/test_seg_cpu.py pins it) and its message names the built path."""
    assert issubclass(RetinaMasksPredictor, SegmentationPredictor) and RetinaMasksPredictor.refused_options == {}
    assert "RetinaMasksPredictor" in SegmentationPredictor.refused_options["retina_masks"]
    assert "retina_masks" in FastSAMPredictor.refused_options and DetectionPredictor.refused_options == {}
    y = edge_yolo_amd.YOLO("yolo11n-seg.yaml")
    for on in (False, True):
        p = SegmentationPredictor(y.model, torch.device("cpu"), graph=False, retina_masks=on)
        assert p.retina_masks is on
    assert SegmentationPredictor(y.model, torch.device("cpu"), graph=False).retina_masks is False
    assert RetinaMasksPredictor(y.model, torch.device("cpu"), graph=False).retina_masks is True
    with pytest.raises(NotImplementedError, match="RetinaMasksPredictor"):
        y.predict(torch.zeros(1, 3, 64, 64), retina_masks=True)
    with pytest.raises(NotImplementedError, match="FastSAM: retina_masks"):
        FastSAMPredictor(y.model, torch.device("cpu"), graph=False, retina_masks=True)
    with pytest.raises(NotImplementedError, match="FastSAM: retina_masks"):
        edge_yolo_amd.FastSAM("FastSAM-s.yaml").predict(torch.zeros(1, 3, 64, 96), retina_masks=True)  # (refused before a device is looked for)
    with pytest.raises(TypeError):  # the detect task does not know the argument
        edge_yolo_amd.YOLO("yolo11n.yaml").predict(torch.zeros(1, 3, 64, 64), retina_masks=True)
    v = SegmentationValidator(y.model, device="cuda", process_mask_native=True)  # (accepted for a validator on the device; nothing is launched here)
    assert v.process_mask_native is True and SegmentationValidator(y.model).process_mask_native is False
    assert SegmentationValidator.val_options["process_mask_native"] is False
    with pytest.raises(NotImplementedError, match="no CPU path"):  # the native assembly is the kernel alone
        SegmentationValidator(y.model, process_mask_native=True)
    for kw in ("save_json", "save_txt", "plots"):
        with pytest.raises(NotImplementedError):
            SegmentationValidator(y.model, device="cuda", process_mask_native=True, **{kw: True})
    mk = edge_yolo_amd.engine.results.Masks(torch.zeros(2, 7, 9, dtype=torch.uint8), (7, 9))
    for prop in ("xy", "xyn"):
        with pytest.raises(NotImplementedError):
            getattr(mk, prop)
    from edge_yolo_amd.utils import ops
    assert callable(ops.process_mask_native)
    assert tuple(ops.process_mask_native(torch.zeros(8, 4, 4), torch.zeros(0, 8), torch.zeros(0, 4), (9, 5)).shape) == (0, 9, 5)
