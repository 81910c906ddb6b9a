"""CPU checks of the pose task: registry / structure / state_dict keys of yolo11{n,s,m,l,x}-pose.yaml against what the reference builds
(tests/golden/structure_pose.json), a Pose row on another backbone, guess_model_task, the data_kpt_shape override, the facade, scale_coords /
clip_coords / Keypoints against the reference's own vectors bit for bit (tests/golden/pose_ops.npz), the float64 restatements
(tests/fp64_pose_ref.py) against the reference's fp32 values, and the numpy kpt_iou route with PoseValidator / PoseMetrics on the reference's
predictions and labels against the reference's own validator (tests/golden/poseval_case.npz)."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import edge_yolo_amd
from edge_yolo_amd import _lib as L
from edge_yolo_amd.engine.results import Keypoints, Results
from edge_yolo_amd.engine.validator import PoseValidator
from edge_yolo_amd.nn import modules as M
from edge_yolo_amd.nn.tasks import DetectionModel, PoseModel, guess_model_task, yaml_model_load
from edge_yolo_amd.utils import metrics
from edge_yolo_amd.utils import ops as uops
import fp64_pose_ref as f64
import pose_synth

KEYS10 = ["metrics/precision(B)", "metrics/recall(B)", "metrics/mAP50(B)", "metrics/mAP75(B)", "metrics/mAP50-95(B)",
          "metrics/precision(P)", "metrics/recall(P)", "metrics/mAP50(P)", "metrics/mAP75(P)", "metrics/mAP50-95(P)"]


@pytest.fixture(scope="module")
def structure(golden_dir):
    return json.load(open(os.path.join(golden_dir, "structure_pose.json")))


@pytest.fixture(scope="module")
def pose_ops(golden_dir):
    return np.load(os.path.join(golden_dir, "pose_ops.npz"))


@pytest.fixture(scope="module")
def case(golden_dir):
    return np.load(os.path.join(golden_dir, "poseval_case.npz"))


@pytest.fixture(scope="module")
def pose_model():
    return PoseModel("yolo11n-pose.yaml")


# ------------------------------------------------------------------------------------------------------------------ registry
@pytest.mark.parametrize("scale", list(pose_synth.SCALES))
def test_registry_builds_the_reference_graph(structure, scale):
    name = pose_synth.NAME.format(scale)
    want = structure[name]
    m = PoseModel(name)
    assert sum(p.numel() for p in m.parameters()) == want["params"]
    assert list(m.save) == want["save"] and [float(s) for s in m.stride] == want["stride"]
    assert [dict(i=l.i, f=l.f, type=l.type, np=int(l.np)) for l in m.model] == want["layers"]
    assert list(m.state_dict()) == want["keys"]
    head = m.model[-1]
    assert isinstance(head, M.Pose) and list(head.kpt_shape) == want["kpt_shape"] == [17, 3] and head.nk == 51 and len(head.cv4) == 3
    assert list(m.kpt_shape) == [17, 3]


def test_n_scale_parameter_counts(structure):
    assert structure["yolo11n-pose.yaml"]["params"] == 2908507
    assert sum(p.numel() for p in PoseModel("yolo11n-pose.yaml", nc=1).parameters()) == 2874462


def test_guess_model_task_and_facade():
    assert guess_model_task("yolo11n-pose.yaml") == "pose" and guess_model_task(yaml_model_load("yolo11s-pose.yaml")) == "pose"
    assert guess_model_task("yolo11n.yaml") == "detect" and guess_model_task("yolo11n-obb.yaml") == "obb"
    y = edge_yolo_amd.YOLO("yolo11n-pose.yaml")
    assert y.task == "pose" and isinstance(y.model, PoseModel) and guess_model_task(y.model) == "pose"
    assert set(y.task_map) == {"detect", "segment"}
    entry = y._task_entry()
    assert entry["model"] is PoseModel and entry["predictor"].__name__ == "PosePredictor" and entry["validator"] is PoseValidator
    with pytest.raises(ValueError):
        edge_yolo_amd.YOLO("yolo11n-pose.yaml", task="detect")
    with pytest.raises(ValueError, match="iterable of batch dicts"):  # val() gets past the task check (obb does not)
        y.val()
    with pytest.raises(NotImplementedError):
        edge_yolo_amd.YOLO("yolo11n-obb.yaml").val(dataloader=[])
    with pytest.raises(NotImplementedError, match="detect task only"):
        next(y.predict_batches([torch.zeros(1, 3, 64, 64)]))


def test_pose_row_on_another_backbone_and_kpt_shape_override():
    d = pose_synth.edgeline_pose_cfg(yaml_model_load("yolo11n-test.yaml"), kpt_shape=(5, 2))
    m = PoseModel(d)
    head = m.model[-1]
    assert isinstance(head, M.Pose) and list(head.kpt_shape) == [5, 2] and head.nk == 10 and [float(s) for s in m.stride] == [8.0, 16.0, 32.0]
    assert head.cv4[0][2].out_channels == 10 and guess_model_task(d) == "pose" and edge_yolo_amd.YOLO(d).task == "pose"
    o = PoseModel("yolo11n-pose.yaml", data_kpt_shape=(5, 2))
    assert list(o.model[-1].kpt_shape) == [5, 2] and o.model[-1].nk == 10 and list(o.yaml["kpt_shape"]) == [5, 2]
    same = PoseModel("yolo11n-pose.yaml", data_kpt_shape=(17, 3))
    assert same.model[-1].nk == 51
    assert guess_model_task(DetectionModel("yolo11n.yaml")) == "detect"


def test_head_keys_and_refusals(pose_ops):
    tag, kw, _ = pose_synth.HEAD_CASE
    M.Pose.legacy = False
    head = M.Pose(**kw)
    assert list(head.state_dict()) == list(pose_ops[tag + "_keys"]) and head.nk == 51
    x = [torch.zeros(1, c, 2, 2) for c in kw["ch"]]
    with pytest.raises(RuntimeError):
        head.train()(x)
    head.eval()
    head.end2end = True
    with pytest.raises(NotImplementedError):
        head(x)
    head.end2end = False
    head.defer_decode = True
    with pytest.raises(NotImplementedError, match="deferred"):
        head(x)
    with pytest.raises(NotImplementedError, match="ndim"):
        M.Pose(nc=2, kpt_shape=(4, 4), ch=(16, 16)).eval()([torch.zeros(1, 16, 2, 2)] * 2)
    with pytest.warns(UserWarning, match="augment"):
        edge_yolo_amd.engine.predictor.PosePredictor(PoseModel("yolo11n-pose.yaml"), torch.device("cpu"), graph=False, augment=True)


# ------------------------------------------------------------------------------------------------------------------ tensor utilities
@pytest.mark.parametrize("case_", pose_synth.COORDS_CASES, ids=[c[0] for c in pose_synth.COORDS_CASES])
def test_scale_coords_equals_the_reference_bits(pose_ops, case_):
    tag, img0, ratio_pad, normalize, padding = case_
    c = pose_synth.coords_vectors()
    out = uops.scale_coords(pose_synth.COORDS_IMG1, c, img0, ratio_pad=ratio_pad, normalize=normalize, padding=padding)
    assert out.data_ptr() == c.data_ptr()  # in place, and the same tensor comes back
    np.testing.assert_array_equal(out.numpy(), pose_ops[tag])
    np.testing.assert_array_equal(out.numpy()[..., 2], pose_synth.coords_vectors().numpy()[..., 2])  # the confidences are not touched


def test_clip_coords_equals_the_reference_bits(pose_ops):
    c = pose_synth.coords_vectors()
    assert uops.clip_coords(c, (60, 100)) is c
    np.testing.assert_array_equal(c.numpy(), pose_ops["clip_coords"])
    a = pose_synth.coords_vectors().numpy()
    assert uops.clip_coords(a, (60, 100)) is a
    np.testing.assert_array_equal(a, pose_ops["clip_coords_np"])


def test_keypoints_container(pose_ops):
    c = pose_synth.coords_vectors()
    k = Keypoints(c, (96, 128))
    assert k.has_visible and len(k) == 6 and tuple(k.shape) == (6, 5, 3)
    for name, got in (("data", k.data), ("xy", k.xy), ("xyn", k.xyn), ("conf", k.conf), ("input_after", c)):
        np.testing.assert_array_equal(got.numpy(), pose_ops["kp3_" + name])
    low = pose_synth.coords_vectors()[..., 2] < 0.5
    assert low.any() and (k.xy[low] == 0).all() and (k.xy[~low] != 0).any() and k.xy[0, 0].abs().sum() > 0  # 0.5 itself is visible
    k2 = Keypoints(pose_synth.coords_vectors()[..., :2].contiguous(), (96, 128))
    assert k2.conf is None and not k2.has_visible
    np.testing.assert_array_equal(k2.data.numpy(), pose_ops["kp2_data"])
    np.testing.assert_array_equal(k2.xyn.numpy(), pose_ops["kp2_xyn"])
    k1 = Keypoints(pose_synth.coords_vectors()[0], (96, 128))
    np.testing.assert_array_equal(k1.data.numpy(), pose_ops["kp1_data"])
    n = k.numpy()
    assert isinstance(n.data, np.ndarray) and n.cpu() is n and isinstance(n.xyn, np.ndarray)
    r = Results(np.zeros((96, 128, 3), np.uint8), "a.jpg", {0: "0"}, boxes=torch.zeros(6, 6), keypoints=pose_synth.coords_vectors())
    assert len(r) == 6 and r.keypoints.orig_shape == (96, 128) and r.masks is None and r.obb is None
    assert Results(None, "a.jpg", {}, boxes=torch.zeros(0, 6)).keypoints is None


# ------------------------------------------------------------------------------------------------------------------ float64 restatements
@pytest.mark.parametrize("case_", pose_synth.DECODE_CASES, ids=[c[0] for c in pose_synth.DECODE_CASES])
def test_decode_restatements_against_the_reference(pose_ops, case_):
    tag, maps, strides, kpt_shape = case_[:4]
    levels = [t.numpy() for t in pose_synth.decode_case(*case_)]
    ref32 = pose_ops[tag + "_y"]
    got32, got64 = f64.decode(levels, strides, kpt_shape, np.float32), f64.decode(levels, strides, kpt_shape)
    ndim = kpt_shape[1]
    xy = np.arange(ref32.shape[1]) % ndim < 2
    np.testing.assert_array_equal(got32[:, xy], ref32[:, xy])  # one rounding: the fp32 restatement IS the reference
    assert (np.abs(got64[:, xy] - ref32[:, xy]) <= f64.ulp32(got64[:, xy])).all()
    if ndim == 3:
        E = float(np.abs(ref32[:, ~xy] - got64[:, ~xy]).max())
        assert E < 2.0 ** -22, E  # the reference's fp32 sigmoid: a few ulp of values below 1


def test_head_case_decode_is_the_restatement(pose_ops):
    tag = pose_synth.HEAD_CASE[0]
    y, kpt = pose_ops[tag + "_y"], pose_ops[tag + "_kpt"]
    off, levels = 0, []
    for _, _, h, w in pose_synth.HEAD_CASE[2]:
        levels.append(kpt[:, :, off:off + h * w].reshape(1, 51, h, w))
        off += h * w
    got = f64.decode(levels, [8.0, 16.0, 32.0], (17, 3), np.float32)
    xy = np.arange(51) % 3 < 2
    np.testing.assert_array_equal(got[:, xy], y[:, 84:][:, xy])


@pytest.mark.parametrize("tag", pose_synth.OKS_CASES)
def test_kpt_iou_host_route_and_restatement(pose_ops, tag):
    g, p, a, sg = pose_synth.oks_case(tag)
    ref32, E = pose_ops[tag], float(pose_ops[tag + "_E"])
    ref64 = f64.kpt_iou64(g, p, a, sg)
    assert ref32.shape == ref64.shape == (len(g), len(p))
    assert abs(float(np.abs(ref32 - ref64).max()) - E) <= 1e-12 and E < 2e-7
    got = metrics.kpt_iou(g, p, a, sg)
    assert isinstance(got, np.ndarray) and got.dtype == np.float32
    err = np.abs(got.astype(np.float64) - ref64)
    print(f"{tag}: E {E:.3e} host route {float(err.max()):.3e}")
    assert (err <= f64.bound(E, ref64)).all()
    np.testing.assert_array_equal(metrics.kpt_iou(torch.tensor(g), torch.tensor(p), torch.tensor(a), sg), got)  # CPU tensors take the same route
    novis = ~(g[..., 2] != 0).any(1)
    assert (got[novis] == 0).all() and (ref32[novis] == 0).all()
    if tag == "oks_novis":
        assert novis.sum() == 2
    if tag == "oks_identical":
        assert (np.abs(np.diag(got) - 1) < 1e-6).all()
    if tag == "oks_area0":
        assert a[0] == 0 and abs(got[0, 0] - 1) < 1e-6 and (got[0, 1:] == 0).all()


def test_oks_sigma_and_metrics_keys():
    np.testing.assert_array_equal(metrics.OKS_SIGMA, pose_synth.OKS_SIGMA)
    assert metrics.OKS_SIGMA.shape == (17,) and metrics.OKS_SIGMA.dtype == np.float64
    pm = metrics.PoseMetrics()
    assert pm.keys == KEYS10 and list(pm.results_dict) == KEYS10 + ["fitness"] and set(pm.results_dict.values()) == {0.0}
    assert pm.pose is pm.seg and isinstance(pm, metrics.SegmentMetrics)


# ------------------------------------------------------------------------------------------------------------------ validator
def _host_preds(g, drop):
    B = len(g["ori_shape"])
    rows = [g[f"pred{i}"] if i != drop else g[f"pred{i}"][:0] for i in range(B)]
    return [r[:, :6] for r in rows], [r[:, 6:].reshape(len(r), 17, 3) for r in rows]


@pytest.mark.parametrize("variant", ["full", "nopred"])
def test_validator_on_reference_predictions(case, pose_model, variant):
    """Rows, keypoints and labels of the reference -> the reference's tp, tp_p, AP and results_dict.  `nopred` drops the predictions of one
    labelled image (npr == 0 bookkeeping); image 1 has no labels in both."""
    g = case
    assert float(g["margin"]) > pose_synth.MARGIN
    B = len(g["ori_shape"])
    v = PoseValidator(pose_model)
    assert v.device.type == "cpu" and v.kpt_shape == [17, 3] and v.sigma is metrics.OKS_SIGMA
    v.update_metrics(_host_preds(g, int(g["empty_pred_image"]) if variant == "nopred" else -1), pose_synth.poseval_batch(g))
    res = v.get_stats()
    assert list(v.stats) == ["tp_p", "tp", "conf", "pred_cls", "target_cls", "target_img"]
    np.testing.assert_array_equal(np.concatenate(v.stats["tp"]), g[variant + "_tp"])
    np.testing.assert_array_equal(np.concatenate(v.stats["tp_p"]), g[variant + "_tp_p"])
    assert g[variant + "_tp_p"].any() and not np.array_equal(g[variant + "_tp"], g[variant + "_tp_p"])
    assert v.seen == int(g[variant + "_seen"]) == B
    np.testing.assert_array_equal(v.nt_per_class, g[variant + "_nt_per_class"])
    np.testing.assert_allclose(v.metrics.box.all_ap, g[variant + "_ap_box"], rtol=0, atol=1e-9)
    np.testing.assert_allclose(v.metrics.pose.all_ap, g[variant + "_ap_pose"], rtol=0, atol=1e-9)
    np.testing.assert_array_equal(v.metrics.box.ap_class_index, g[variant + "_ap_class_index"])
    assert list(res) == list(g[variant + "_keys"]) == KEYS10 + ["fitness"]
    for k, want in zip(g[variant + "_keys"], g[variant + "_values"]):
        assert abs(res[k] - float(want)) <= 1e-9, (k, res[k], float(want))
    assert abs(res["fitness"] - (res[KEYS10[4]] + res[KEYS10[9]])) <= 1e-12


def test_validator_cpu_tensors_single_cls_and_other_kpt_shapes(case, pose_model):
    g = case
    v = PoseValidator(pose_model)
    rows, kpts = _host_preds(g, -1)
    v.update_metrics(([torch.tensor(r) for r in rows], [torch.tensor(k) for k in kpts]), pose_synth.poseval_batch(g, wrap=torch.tensor))
    np.testing.assert_array_equal(np.concatenate(v.stats["tp_p"]), g["full_tp_p"])
    s = PoseValidator(pose_model, single_cls=True)
    s.update_metrics(_host_preds(g, -1), pose_synth.poseval_batch(g))
    assert (np.concatenate(s.stats["pred_cls"]) == 0).all()
    five = PoseValidator(PoseModel("yolo11n-pose.yaml", data_kpt_shape=(5, 2)))
    np.testing.assert_array_equal(five.sigma, np.ones(5) / 5)
    for kw in ("save_json", "save_txt", "plots"):
        with pytest.raises(NotImplementedError, match=kw):
            PoseValidator(pose_model, **{kw: True})
    with pytest.raises(NotImplementedError):
        v.update(None, None)
    fv = PoseValidator(edge_yolo_amd.YOLO("yolo11n-pose.yaml"))  # a facade is accepted like DetectionValidator accepts one
    assert fv.conf == 0.001 and list(fv.results_dict) == KEYS10 + ["fitness"]


# ------------------------------------------------------------------------------------------------------------------ library
def test_pose_symbols_and_host_side_refusals():
    """The three entries are exported; the argument checks that run before any launch answer on a host without a GPU."""
    lib = L.lib()
    for name in ("ey_kpts_decode_levels", "ey_kpts_decode_rows", "ey_kpt_iou"):
        assert hasattr(lib, name) and name in L.SIGNATURES
    IA1, FA1, PA1 = ctypes.c_int * 1, ctypes.c_float * 1, ctypes.c_void_p * 1
    one = dict(H=IA1(1), W=IA1(1), st=FA1(8.0), ptr=PA1(64), cs=IA1(512), off=IA1(0))

    def levels(nl, nkpt, ndim):
        return lib.ey_kpts_decode_levels(L.F32, 1, nl, one["H"], one["W"], one["st"], one["ptr"], one["cs"], nkpt, ndim, 64, 1024, 1, one["off"], None)

    def rows(nl, nkpt, ndim):
        return lib.ey_kpts_decode_rows(L.F32, 1, nl, one["H"], one["W"], one["st"], one["ptr"], one["cs"], nkpt, ndim, 1, one["off"], 1, 64, 64, 64, None)

    for fn in (levels, rows):
        assert fn(5, 17, 3) == -2 and fn(0, 17, 3) == -2  # EY_EUNSUPPORTED: 1 to 4 levels
        assert fn(1, 17, 4) == -2 and fn(1, 17, 1) == -2  # ndim 2 or 3
        assert fn(1, 86, 3) == -2 and fn(1, 129, 2) == -2  # nkpt * ndim <= 256
    off2 = (ctypes.c_int * 2)(0, 0)
    out_off = (ctypes.c_long * 1)(0)
    assert lib.ey_kpt_iou(1, 65, 3, 64, off2, 64, off2, 64, 64, out_off, 64, None) == -2  # K <= 64
    assert lib.ey_kpt_iou(129, 17, 3, 64, off2, 64, off2, 64, 64, out_off, 64, None) == -2  # B <= 128
    assert lib.ey_kpt_iou(1, 17, 4, 64, off2, 64, off2, 64, 64, out_off, 64, None) == -2
    assert lib.ey_kpt_iou(0, 17, 3, None, None, None, None, None, None, None, None, None) == 0  # B == 0 is valid
    assert lib.ey_kpt_iou(1, 17, 3, None, off2, None, off2, None, None, out_off, None, None) == 0  # no pair anywhere: nothing to launch
