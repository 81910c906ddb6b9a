"""YOLOv9 (GELAN) without a GPU: structure, state_dict keys and parameter counts of the seven model files against the reference
(tests/golden/structure_v9.json), guess_model_task and the legacy head flag; the float64 restatements of the ADown / AConv pooling front end,
CBFuse and the RepConv fold against the reference's own outputs (tests/golden/v9_ops.npz); the nearest-resize index rule against
torch.nn.functional.interpolate; fuse_convs; and the refusals.

The bounds are counted operation by operation with u = 2^-24 (the reference computes in fp32), not fitted (the achieved error is printed):
  avg pool   three sums and one exact scaling by 0.25:               |A_ref - A_64| <= 3 u * 0.25 * sum|x|  (any order of the three sums)
  max pool   a maximum of values each within e of its float64 twin lies within e of the float64 maximum
  CBFuse     n - 1 sums in any order:                                 |y_ref - y_64| <= (n - 1) u * sum|terms|
  RepConv    the reference adds three fp32 results: conv1 (9 c1 products and sums, then BatchNorm: 4 more roundings), conv2 (c1 of them, then
             BatchNorm), the identity BatchNorm (4 roundings), two sums, then SiLU.  With T the sum over the three branches of sum|k||x| + |b|
             (each branch's BatchNorm-folded float64 kernel, absolute values), the pre-activation differs from the float64 fold by at most
             (9 c1 + c1 + 3 * 4 + 2 + 2) u T; SiLU has slope <= 1.1 and adds 4 u |y| of its own (exp, sum, division, product)."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fp64_v9_ref as f64
import v9_synth as vs

U = 2.0 ** -24


@pytest.fixture(scope="module")
def structure(golden_dir):
    with open(os.path.join(golden_dir, "structure_v9.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def ops_golden(golden_dir):
    return np.load(os.path.join(golden_dir, "v9_ops.npz"))


def _model(name):
    from edge_yolo_amd.nn.tasks import DetectionModel, SegmentationModel
    return (SegmentationModel if vs.TASK[name] == "segment" else DetectionModel)(name)


@pytest.mark.parametrize("name", vs.FILES)
def test_structure_matches_reference(structure, name):
    from edge_yolo_amd.nn.tasks import guess_model_task
    from edge_yolo_amd import YOLO
    want = structure[name]
    m = _model(name)
    assert sum(p.numel() for p in m.parameters()) == want["params"]
    if name in vs.PARAMS:
        assert want["params"] == vs.PARAMS[name]
    assert list(m.save) == want["save"]
    assert [float(s) for s in m.stride] == want["stride"]
    assert [dict(i=l.i, f=l.f, type=l.type, np=int(l.np)) for l in m.model] == want["layers"]
    assert list(m.state_dict()) == vs.unpack_keys(want["keys"])
    assert guess_model_task(name) == vs.TASK[name] and guess_model_task(m) == vs.TASK[name]
    assert m.model[-1].legacy is True and want["legacy"] is True
    y = YOLO(name)
    assert y.task == vs.TASK[name] and type(y.model).__name__ == ("SegmentationModel" if vs.TASK[name] == "segment" else "DetectionModel")


def test_silence_row_is_renamed_and_identity_only_as_layer_0():
    from edge_yolo_amd.nn.tasks import DetectionModel, yaml_model_load
    d = yaml_model_load("yolov9e.yaml")
    d["backbone"][0][2] = "Silence"
    m = DetectionModel(d)
    assert type(m.model[0]) is torch.nn.Identity and m.yaml["backbone"][0][2] == "nn.Identity"
    d = yaml_model_load("yolov9t.yaml")
    d["backbone"].insert(2, [-1, 1, "nn.Identity", []])
    with pytest.raises(NotImplementedError, match="nn.Identity"):
        DetectionModel(d)


def test_repncspelan4_n_is_an_argument_not_a_repeat():
    m = _model("yolov9t.yaml")
    blk = m.model[4]
    assert type(blk).__name__ == "RepNCSPELAN4" and len(blk.cv2[0].m) == 3 and len(blk.cv3[0].m) == 3
    assert type(blk.cv2[0].m[0].cv1).__name__ == "RepConv"


# ---------------------------------------------------------------------------------------------------------------- float64 restatements
@pytest.mark.parametrize("tag", ["aconv", "adown"])
def test_adown_pool64_vs_reference(ops_golden, tag):
    case = next(c for c in vs.MODULE_CASES if c[0] == tag)
    x = vs.case_input(tag, case[4]).numpy()
    C = x.shape[1]
    c_avg = C if tag == "aconv" else C // 2
    a64, m64 = f64.adown_pool64(x, c_avg)
    x64 = np.abs(x.astype(np.float64))
    T = 0.25 * (x64[:, :, :-1, :-1] + x64[:, :, :-1, 1:] + x64[:, :, 1:, :-1] + x64[:, :, 1:, 1:])
    bnd = 3 * U * T
    err = np.abs(ops_golden[tag + "_a"].astype(np.float64) - a64)
    print(f"{tag} a: max err {err.max():.3e}, bound {bnd[:, :c_avg].max():.3e}")
    assert (err <= bnd[:, :c_avg]).all()
    if m64 is None:
        assert tag + "_m" not in ops_golden.files
        return
    # every pooled value lies within the largest bound of its window of the float64 maximum
    bm = f64._maxpool3s2p1(bnd[:, c_avg:])
    err = np.abs(ops_golden[tag + "_m"].astype(np.float64) - m64)
    print(f"{tag} m: max err {err.max():.3e}, bound {bm.max():.3e}")
    assert m64.shape == ops_golden[tag + "_m"].shape and (err <= bm).all()
    # the stated fp32 order reproduces the reference bit for bit (torch's CPU avg_pool2d sums in that order)
    a32, m32 = f64.adown_pool_stated(x, c_avg, np.float32)
    assert np.array_equal(a32, ops_golden[tag + "_a"]) and np.array_equal(m32, ops_golden[tag + "_m"])


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
@pytest.mark.parametrize("shape", [(2, 16, 3, 5), (1, 8, 9, 7), (2, 8, 2, 2), (1, 8, 17, 33)], ids=str)
def test_stated_avg_order_is_torchs_cpu_avg_pool(shape, dtype):
    """Both memory formats, fp32 and f16: the numpy restatement of the stated order equals torch's CPU avg_pool2d / chunk / max_pool2d bits."""
    x = torch.tensor(vs.exact_input(f"avg{shape}", shape, dtype == torch.float16)).to(dtype)
    npdt = np.float16 if dtype == torch.float16 else np.float32
    c_avg = shape[1] // 2 if shape[1] >= 16 else shape[1]
    a, m = f64.adown_pool_stated(x.float().numpy(), c_avg, npdt)
    for xx in (x, x.contiguous(memory_format=torch.channels_last)):
        A = F.avg_pool2d(xx, 2, 1, 0, False, True)
        assert np.array_equal(A[:, :c_avg].float().numpy(), a.astype(np.float32))
        if m is not None:
            assert np.array_equal(F.max_pool2d(A[:, c_avg:].float(), 3, 2, 1).numpy(), m.astype(np.float32))


def test_cbfuse64_vs_reference(ops_golden):
    tag, idx, _, _ = vs.CBFUSE_CASE
    xs = vs.cbfuse_inputs()
    srcs = [x[idx[i]].numpy() for i, x in enumerate(xs[:-1])] + [xs[-1].numpy()]
    y64, T = f64.cbfuse64(srcs)
    err = np.abs(ops_golden[tag + "_y"].astype(np.float64) - y64)
    bnd = (len(srcs) - 1) * U * T
    print(f"cbfuse: max err {err.max():.3e}, bound {bnd.max():.3e}")
    assert (err <= bnd).all()
    got = f64.cbfuse_stated(srcs, np.float32)  # list order: within the same bound of float64
    assert (np.abs(got.astype(np.float64) - y64) <= bnd).all()


@pytest.mark.parametrize("n_in,n_out", vs.NEAREST_PAIRS)
def test_nearest_index_rule_is_torchs(n_in, n_out):
    src = torch.arange(n_in, dtype=torch.float32)
    want_h = F.interpolate(src.view(1, 1, n_in, 1).expand(1, 1, n_in, 2), size=(n_out, 2), mode="nearest")[0, 0, :, 0].long().numpy()
    want_w = F.interpolate(src.view(1, 1, 1, n_in).expand(1, 1, 2, n_in), size=(2, n_out), mode="nearest")[0, 0, 0].long().numpy()
    got = f64.nearest_index(n_out, n_in)
    assert np.array_equal(got, want_h) and np.array_equal(got, want_w)


@pytest.mark.parametrize("tag", ["repconv", "repconv_bn"])
def test_repconv_fold64_reproduces_the_unfused_reference(ops_golden, tag):
    from edge_yolo_amd.nn.modules import RepConv
    _, _, args, kw, shape = next(c for c in vs.MODULE_CASES if c[0] == tag)
    m = RepConv(*args, **kw).eval()
    sd = vs.state_dict(m.state_dict(), prefix=tag + ".")
    m.load_state_dict(sd)
    assert list(m.state_dict()) == list(ops_golden[tag + "_keys"])
    x = vs.case_input(tag, shape).numpy()
    eps = m.conv1.bn.eps
    k, b = f64.repconv_fold64({kk: v.numpy() for kk, v in sd.items()}, eps)
    pre = f64.conv3x3_64(x, k, b)
    y64 = f64.silu64(pre)
    # scale: the branches' absolute terms
    c1 = args[0]
    T = np.zeros_like(pre)
    for kk, bb in f64.repconv_branches64({key: v.numpy() for key, v in sd.items()}, eps):
        T += f64.conv3x3_64(np.abs(x), np.abs(kk), np.abs(bb))
    bnd = 1.1 * (10 * c1 + 16) * U * T + 4 * U * np.abs(y64)
    err = np.abs(ops_golden[tag + "_y"].astype(np.float64) - y64)
    print(f"{tag}: max err {err.max():.3e}, bound {bnd.max():.3e} (ratio {float((err / bnd).max()):.3f})")
    assert (err <= bnd).all()
    # the module's own fp32 fold is the float64 fold rounded (a few ulp of the branch terms)
    kf, bf = m.get_equivalent_kernel_bias()
    assert np.abs(kf.numpy() - k).max() <= 8 * U * np.abs(k).max() and np.abs(bf.numpy() - b).max() <= 16 * U * max(np.abs(b).max(), 1.0)
    # fuse_convs leaves exactly the reference's keys, and the same fold
    m.fuse_convs()
    assert list(m.state_dict()) == list(ops_golden[tag + "_fused_keys"]) == ["conv.weight", "conv.bias"]
    assert not hasattr(m, "conv1") and not hasattr(m, "conv2") and not hasattr(m, "bn")
    kf2, bf2 = m.folded()
    assert torch.equal(kf2, kf) and torch.equal(bf2, bf)
    m.fuse_convs()  # idempotent


def test_model_fuse_calls_fuse_convs(structure):
    m = _model("yolov9t.yaml")
    m.load_state_dict(vs.state_dict(m.state_dict()))
    m.fuse()
    reps = [mod for mod in m.modules() if type(mod).__name__ == "RepConv"]
    assert reps and all(hasattr(r, "conv") and not hasattr(r, "conv1") for r in reps)
    assert m.convs_folded() and not any(k.endswith("running_mean") for k in m.state_dict())


def test_module_keys_match_reference(ops_golden):
    from edge_yolo_amd.nn import modules as M
    for tag, cls, args, kw, _ in vs.MODULE_CASES:
        assert list(getattr(M, cls)(*args, **kw).state_dict()) == list(ops_golden[tag + "_keys"]), tag
    tag, args, _ = vs.CBLINEAR_CASE
    assert list(M.CBLinear(*args).state_dict()) == list(ops_golden[tag + "_keys"])


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals():
    from edge_yolo_amd.nn import _ops as ops, modules as M
    with pytest.raises(NotImplementedError, match="k=5"):
        M.SPPELAN(32, 32, 16, k=3)
    with pytest.raises(NotImplementedError, match="CBLinear"):
        M.CBLinear(32, [8, 8], k=3)
    with pytest.raises(NotImplementedError, match="CBLinear"):
        M.CBLinear(32, [8, 8], g=2)
    with pytest.raises(ValueError, match="multiples of 8"):
        ops.adown_pool(torch.zeros(1, 12, 4, 4))
    with pytest.raises(ValueError, match="multiples of 8"):
        ops.adown_pool(torch.zeros(1, 16, 4, 4), 4)
    with pytest.raises(ValueError, match="c_avg"):
        ops.adown_pool(torch.zeros(1, 16, 4, 4), 0)
    with pytest.raises(ValueError, match="2x2 window"):
        ops.adown_pool(torch.zeros(1, 16, 1, 4))
    with pytest.raises(ValueError, match="multiple of 8"):
        ops.cbfuse([torch.zeros(1, 12, 2, 2), torch.zeros(1, 12, 4, 4)])
    with pytest.raises(ValueError, match="1 to 6"):
        ops.cbfuse([torch.zeros(1, 8, 2, 2)] * 7)
    with pytest.raises(NotImplementedError, match="at most 6"):
        M.CBFuse([0] * 6)([(torch.zeros(1, 8, 2, 2),)] * 6 + [torch.zeros(1, 8, 4, 4)])


def test_predict_batches_refuses_yolov9e():
    from edge_yolo_amd import YOLO
    with pytest.raises(NotImplementedError, match="nn.Identity"):
        next(iter(YOLO("yolov9e.yaml").predict_batches([torch.zeros(1, 3, 64, 64)])))
