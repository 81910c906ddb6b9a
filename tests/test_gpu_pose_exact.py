"""-m gpu: the three pose kernels (csrc/pose.hip) against the reference's golden values and the float64 restatements of tests/fp64_pose_ref.py.

x / y keypoint values have one rounding: they equal the reference's fp32 result (golden) and the fp32 restatement bit for bit.  Every
other float output (the sigmoid rows, OKS) follows the project's rule: per case E = max |reference fp32 (golden) - float64| on the case's own
inputs; the kernel must satisfy |gpu - float64| <= 4 E + 2 ulp(fp32) of the value.  E and the achieved error are printed per case.
ey_kpts_decode_rows equals ey_kpts_decode_levels at the kept anchors bit for bit and writes zeros everywhere else.  Indices >= A_total are not
fed on the GPU: that guard is checked by reading csrc/pose.hip (kpts_decode_rows_kernel forms the address only behind `l >= 0`)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import fp64_pose_ref as f64  # noqa: E402
import pose_synth  # noqa: E402

NAN = float("nan")


@pytest.fixture(scope="module")
def pose_ops(golden_dir):
    return np.load(os.path.join(golden_dir, "pose_ops.npz"))


def _check(tag, got, ref32, ref64):
    """the tolerance rule; returns (E, achieved)."""
    got, ref32 = np.asarray(got, np.float64), np.asarray(ref32, np.float64)
    assert got.shape == ref64.shape == ref32.shape, (tag, got.shape, ref64.shape)
    E = float(np.abs(ref32 - ref64).max()) if ref64.size else 0.0
    err = np.abs(got - ref64)
    ach = float(err.max()) if err.size else 0.0
    print(f"{tag}: E {E:.3e} achieved {ach:.3e} bound(min) {4 * E:.3e}")
    bad = err > f64.bound(E, ref64)
    assert not bad.any(), f"{tag}: {int(bad.sum())} values beyond 4E + 2ulp (E {E:.3e}, worst {ach:.3e})"
    return E, ach


def _device_levels(case):
    """the case's logits as NHWC device views (channel-sliced out of wider NaN-filled buffers when the case says so) -> (levels, A)."""
    from edge_yolo_amd import _lib as L
    tag, maps, strides, kpt_shape, B, half, sliced = case
    dt = torch.float16 if half else torch.float32
    lead = (8 if half else 3) if sliced else 0  # f16: a 16-byte aligned window (vector loads); f32: a misaligned one (scalar loads)
    levels, a_off = [], 0
    for t, (H, W), s in zip(pose_synth.decode_case(*case), maps, strides):
        c = t.shape[1]
        buf = L.empty_nhwc(B, lead + (c + 7) // 8 * 8 + (8 if sliced else 0), H, W, dt, "cuda")
        buf.fill_(NAN)  # whatever lies beside the window must not matter
        v = buf[:, lead:lead + c]
        v.copy_(t.to(dt))
        levels.append((v, s, a_off))
        a_off += H * W
    return levels, a_off


@pytest.fixture(scope="module")
def decoded():
    """ey_kpts_decode_levels of every case, once: tag -> (levels, A, pred (B, 7 + nk, A) device tensor whose rows 7.. the kernel wrote)."""
    from edge_yolo_amd.nn import _ops
    out = {}
    for case in pose_synth.DECODE_CASES:
        levels, A = _device_levels(case)
        nk = case[3][0] * case[3][1]
        pred = torch.full((case[4], 7 + nk, A), NAN, dtype=torch.float32, device="cuda")
        _ops.kpts_decode_levels(levels, case[3], pred[:, 7:])  # rows 4 + nc .. of a prediction tensor, in place
        out[case[0]] = (levels, A, pred)
    return out


# ------------------------------------------------------------------------------------------------------------------ ey_kpts_decode_levels
@pytest.mark.parametrize("case", pose_synth.DECODE_CASES, ids=[c[0] for c in pose_synth.DECODE_CASES])
def test_decode_levels(pose_ops, decoded, case):
    tag, maps, strides, kpt_shape, B = case[:5]
    nk, ndim = kpt_shape[0] * kpt_shape[1], kpt_shape[1]
    pred = decoded[tag][2].cpu().numpy()
    assert np.isnan(pred[:, :7]).all()  # the rows in front belong to the box / class decode: untouched
    got = pred[:, 7:]
    assert np.isfinite(got).all()
    ref32 = pose_ops[tag + "_y"]
    logits = [t.numpy() for t in pose_synth.decode_case(*case)]  # (f16 cases: drawn f16-representable, so these ARE the rounded logits)
    xy = np.arange(nk) % ndim < 2
    np.testing.assert_array_equal(got[:, xy], ref32[:, xy])
    np.testing.assert_array_equal(got[:, xy], f64.decode(logits, strides, kpt_shape, np.float32)[:, xy])
    if ndim == 3:
        _check(tag + " sigmoid", got[:, ~xy], ref32[:, ~xy], f64.decode(logits, strides, kpt_shape)[:, ~xy])


def test_decode_refusals():
    from edge_yolo_amd import _lib as L
    from edge_yolo_amd.nn import _ops
    levels, A = _device_levels(pose_synth.DECODE_BY_TAG["kd_1x1_17x3_b1_f32"])
    out = torch.empty((1, 51, A), device="cuda")
    idx, cnt = torch.zeros((1, 4), dtype=torch.int32, device="cuda"), torch.ones(1, dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError):
        _ops.kpts_decode_levels(levels, (17, 3), torch.empty((1, 50, A), device="cuda"))
    with pytest.raises(ValueError):
        _ops.kpts_decode_levels(levels, (17, 3), torch.empty((1, 51, A), device="cuda", dtype=torch.float16))
    with pytest.raises(NotImplementedError, match="levels"):
        _ops.kpts_decode_levels(levels * 5, (17, 3), out)
    with pytest.raises(NotImplementedError, match="levels"):
        _ops.kpts_decode_rows(levels * 5, (17, 3), idx, cnt)
    m4 = [(L.empty_nhwc(1, 8, 1, 1, torch.float32, "cuda"), 8.0, 0)]
    with pytest.raises(NotImplementedError, match="ndim"):
        _ops.kpts_decode_levels(m4, (2, 4), torch.empty((1, 8, 1), device="cuda"))
    with pytest.raises(NotImplementedError, match="ndim"):
        _ops.kpts_decode_rows(m4, (2, 4), idx, cnt)
    big = [(L.empty_nhwc(1, 258, 1, 1, torch.float32, "cuda"), 8.0, 0)]
    with pytest.raises(NotImplementedError, match="channels"):
        _ops.kpts_decode_levels(big, (86, 3), torch.empty((1, 258, 1), device="cuda"))
    with pytest.raises(NotImplementedError, match="channels"):
        _ops.kpts_decode_rows(big, (129, 2), idx, cnt)
    with pytest.raises(ValueError):
        _ops.kpts_decode_rows(levels, (17, 3), idx.long(), cnt)
    g, p = torch.zeros((1, 65, 3), device="cuda"), torch.zeros((1, 65, 3), device="cuda")
    with pytest.raises(NotImplementedError, match="keypoints"):
        _ops.kpt_iou(p, [0, 1], g, [0, 1], torch.ones(1, device="cuda"), torch.ones(65, device="cuda"))
    with pytest.raises(ValueError):
        _ops.kpt_iou(p, [0, 1], g, [0, 2], torch.ones(1, device="cuda"), torch.ones(65, device="cuda"))


# ------------------------------------------------------------------------------------------------------------------ ey_kpts_decode_rows
@pytest.mark.parametrize("max_det", [1, 300])
@pytest.mark.parametrize("case", pose_synth.DECODE_CASES, ids=[c[0] for c in pose_synth.DECODE_CASES])
def test_decode_rows(decoded, case, max_det):
    from edge_yolo_amd.nn import _ops
    tag, maps, strides, kpt_shape, B = case[:5]
    nkpt, ndim = kpt_shape
    levels, A, pred = decoded[tag]
    full = pred[:, 7:].cpu().numpy()  # (B, nk, A)
    index, count = pose_synth.rows_index(maps, B, max_det)
    if max_det > 8:
        ends = {int(v) for v in np.concatenate([[0], np.cumsum([h * w for h, w in maps])[:-1], np.cumsum([h * w for h, w in maps]) - 1])}
        live = set(index[0, :count[0]].tolist())
        assert ends <= live and -1 in live and (count == 0).any() == (B > 1) and (count < max_det).any()
    di, dc = torch.tensor(index).cuda(), torch.tensor(count).cuda()
    out = torch.full((B, max_det, nkpt, ndim), NAN, dtype=torch.float32, device="cuda")
    assert _ops.kpts_decode_rows(levels, kpt_shape, di, dc, A, out=out) is out
    got = out.cpu().numpy()
    want = np.zeros_like(got)
    for b in range(B):
        for r in range(int(count[b])):
            if index[b, r] >= 0:
                want[b, r] = full[b, :, index[b, r]].reshape(nkpt, ndim)
    np.testing.assert_array_equal(got, want)  # kept rows: the levels kernel's bits; all others exactly zero (the NaN fill is gone)
    again = _ops.kpts_decode_rows(levels, kpt_shape, di, dc)  # (A defaults to the end of the last level)
    assert got.tobytes() == again.cpu().numpy().tobytes()


def test_decode_rows_graph_replay(decoded):
    from edge_yolo_amd.nn import _ops
    case = pose_synth.DECODE_BY_TAG["kd_3lv_17x3_b2_f16_sliced"]
    levels, A, _ = decoded[case[0]]
    index, count = pose_synth.rows_index(case[1], 2, 300)
    di, dc = torch.tensor(index).cuda(), torch.tensor(count).cuda()
    eager = _ops.kpts_decode_rows(levels, case[3], di, dc).clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = _ops.kpts_decode_rows(levels, case[3], di, dc)
    out.fill_(NAN)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)


# ------------------------------------------------------------------------------------------------------------------ ey_kpt_iou
@pytest.mark.parametrize("tag", pose_synth.OKS_CASES)
def test_kpt_iou(pose_ops, tag):
    from edge_yolo_amd.utils import metrics
    g, p, a, sg = pose_synth.oks_case(tag)
    got = metrics.kpt_iou(torch.tensor(g).cuda(), torch.tensor(p).cuda(), torch.tensor(a).cuda(), sg)
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (len(g), len(p))
    got = got.cpu().numpy()
    ref64 = f64.kpt_iou64(g, p, a, sg)
    E, _ = _check(tag, got, pose_ops[tag], ref64)
    assert abs(E - float(pose_ops[tag + "_E"])) <= 1e-12
    novis = ~(g[..., 2] != 0).any(1)
    assert (got[novis] == 0).all()
    if tag == "oks_novis":
        assert novis.sum() == 2 and (got[~novis] > 0).any()
    if tag == "oks_area0":
        assert (got[0, 1:] == 0).all() and got[0, 0] > 0.999
    if tag == "oks_k5_ndim2":
        assert p.shape[2] == 2 and len(sg) == 5


def test_kpt_iou_batch_writes_only_its_matrices(pose_ops):
    """Three images in one call (one without ground truth, one without predictions), matrices at caller-chosen offsets of a NaN-filled
    buffer: every matrix under the rule, every other element still NaN."""
    from edge_yolo_amd.nn import _ops
    parts, sg = pose_synth.oks_batch()
    n, m = [len(p) for _, p, _ in parts], [len(g) for g, _, _ in parts]
    assert m[1] == 0 and n[2] == 0 and n[0] * m[0] > 0
    pred = torch.tensor(np.concatenate([p for _, p, _ in parts])).cuda()
    gt = torch.tensor(np.concatenate([g for g, _, _ in parts])).cuda()
    area = torch.tensor(np.concatenate([a for _, _, a in parts])).cuda()
    pred_off, gt_off = np.concatenate([[0], np.cumsum(n)]), np.concatenate([[0], np.cumsum(m)])
    buf = torch.full((5 + n[0] * m[0] + 9,), NAN, dtype=torch.float32, device="cuda")
    out, off = _ops.kpt_iou(pred, pred_off, gt, gt_off, area, torch.tensor(sg).cuda(), out_off=[5, 0, 0], out=buf)
    assert out is buf and off == [5, 0, 0]
    host = buf.cpu().numpy()
    g0, p0, a0 = parts[0]
    _check("oks_batch image 0", host[5:5 + n[0] * m[0]].reshape(m[0], n[0]), pose_ops["oks_batch0"], f64.kpt_iou64(g0, p0, a0, sg))
    assert np.isnan(host[:5]).all() and np.isnan(host[5 + n[0] * m[0]:]).all()
    packed, poff = _ops.kpt_iou(pred, pred_off, gt, gt_off, area, torch.tensor(sg).cuda())  # default: packed one after the other
    assert poff == [0, n[0] * m[0], n[0] * m[0]] and packed.numel() == n[0] * m[0]
    assert packed.cpu().numpy().tobytes() == host[5:5 + n[0] * m[0]].tobytes()
    empty, _ = _ops.kpt_iou(pred[:0], [0], gt[:0], [0], area[:0], torch.tensor(sg).cuda())  # B == 0
    assert empty.numel() == 0
