"""-m gpu: ey_match_batch against the reference's recorded results (tests/golden/confusion_cases.npz, cases of tests/confusion_synth.py).
Every case runs in one launch per class count (B >= 3): the true positives and the confusion matrix equal the goldens exactly; boxes mode
equals matrix mode; xform given equals rows scaled by ops.scale_boxes on the host; rows beyond count are NaN and must not be read, tp beyond
count holds a sentinel and must come back untouched; the rows are channel windows of wider NaN-filled buffers; a second call accumulates the
matrix to exactly twice the first; T = 1 and T = 10; refusals leave sentinels in both outputs; a second run gives the same bits."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import confusion_synth as S  # noqa: E402

MAX_DET, SENT = 300, 0xA5
NCS = [1, 3, 80]


@pytest.fixture(scope="module")
def cases(golden_dir):
    return S.golden_cases(golden_dir)


def _group(cases, nc):
    return [c for c in cases[0] if c["nc"] == nc]


def _pack(group, key, stride):
    """The group's rows as a (B, MAX_DET, 6) channel window of a NaN-filled (B, MAX_DET, stride) buffer, and the counts."""
    buf = torch.full((len(group), MAX_DET, stride), float("nan"))
    for i, c in enumerate(group):
        buf[i, :len(c[key]), :6] = torch.from_numpy(c[key][:, :6])
    return buf.cuda()[:, :, :6], torch.tensor([len(c[key]) for c in group], dtype=torch.int32).cuda()


def _labels(group):
    gt = torch.from_numpy(np.concatenate([c["gt"].reshape(-1, 4) for c in group]).astype(np.float32)).cuda()
    cls = torch.from_numpy(np.concatenate([c["gt_cls"] for c in group]).astype(np.int32)).cuda()
    return gt, cls, np.concatenate([[0], np.cumsum([len(c["gt"]) for c in group])]).tolist()


def _outputs(B, T, nc):
    return torch.full((B, MAX_DET, T), SENT, dtype=torch.uint8).cuda(), torch.zeros((nc + 1) ** 2, dtype=torch.int32).cuda()


def _check(group, tp, matrix, nc, T=10, times=1):
    tp = tp.cpu().numpy()
    for i, c in enumerate(group):
        n = len(c["det"])
        assert np.array_equal(tp[i, :n], c["tp"][:, :T].astype(np.uint8)), c["name"]
        assert (tp[i, n:] == SENT).all(), c["name"]
    if matrix is not None:
        assert np.array_equal(matrix.cpu().numpy().reshape(nc + 1, nc + 1), times * sum(c["matrix"] for c in group))


@pytest.fixture(scope="module")
def first_run(cases):
    """boxes mode with xform, stride 38, all three class counts: computed once, shared."""
    from edge_yolo_amd.nn import _ops
    out = {}
    for nc in NCS:
        group = _group(cases, nc)
        assert len(group) >= 3
        rows, count = _pack(group, "det", 38)
        gt, cls, gt_off = _labels(group)
        xform = torch.from_numpy(np.stack([S.xform_row(c["ori_shape"], c["ratio_pad"]) for c in group])).cuda()
        tp, matrix = _outputs(len(group), 10, nc)
        _ops.match_batch(rows, count, cls, gt_off, S.IOUV, nc, gt=gt, xform=xform, cm_conf=S.CM_CONF, cm_iou=S.CM_IOU, tp=tp, matrix=matrix)
        out[nc] = (rows, count, gt, cls, gt_off, xform, tp.clone(), matrix.clone())
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("nc", NCS)
def test_boxes_mode_with_xform_equals_the_reference(cases, first_run, nc):
    from edge_yolo_amd.nn import _ops
    group = _group(cases, nc)
    rows, count, gt, cls, gt_off, xform, tp, matrix = first_run[nc]
    assert rows.stride(1) == 38 and torch.isnan(rows[0, int(count[0]):]).all()
    _check(group, tp, matrix, nc)
    # the same bits on a second run, and the matrix accumulates to exactly twice the first
    tp2, m2 = _outputs(len(group), 10, nc)
    m2.copy_(matrix)
    _ops.match_batch(rows, count, cls, gt_off, S.IOUV, nc, gt=gt, xform=xform, cm_conf=S.CM_CONF, cm_iou=S.CM_IOU, tp=tp2, matrix=m2)
    assert torch.equal(tp2, tp)
    _check(group, tp2, m2, nc, times=2)


@pytest.mark.parametrize("nc", NCS)
def test_prescaled_rows_matrix_mode_and_single_threshold(cases, first_run, nc):
    from edge_yolo_amd.nn import _ops
    from edge_yolo_amd.utils import ops as uops
    group = _group(cases, nc)
    _, count, gt, cls, gt_off, _, tp0, m0 = first_run[nc]
    B = len(group)
    # rows scaled by ops.scale_boxes on the host, no xform, stride 6
    scaled = []
    for c in group:
        r = torch.from_numpy(c["det"].copy())
        if len(r):
            uops.scale_boxes(S.IMGSZ, r[:, :4], c["ori_shape"], ratio_pad=c["ratio_pad"])
        assert np.array_equal(r.numpy(), c["predn"])
        scaled.append(dict(c, rows=r.numpy()))
    rows, _ = _pack(scaled, "rows", 6)
    tp, matrix = _outputs(B, 10, nc)
    _ops.match_batch(rows, count, cls, gt_off, S.IOUV, nc, gt=gt, cm_conf=S.CM_CONF, cm_iou=S.CM_IOU, tp=tp, matrix=matrix)
    assert torch.equal(tp, tp0) and torch.equal(matrix, m0)
    # matrix mode on the box IoUs: identical outputs; the boxes of the rows are NaN there
    n = [len(c["det"]) for c in group]
    ious = [S.box_iou(c["gt"], c["predn"][:, :4]).reshape(-1) for c in group]
    off = np.concatenate([[0], np.cumsum([len(v) for v in ious])])[:-1].tolist()
    flat = torch.from_numpy(np.concatenate(ious + [np.zeros(1, np.float32)])).cuda()
    nan_rows = rows.clone()
    nan_rows[..., :4] = float("nan")
    tp, matrix = _outputs(B, 10, nc)
    _ops.match_batch(nan_rows, count, cls, gt_off, S.IOUV, nc, iou=flat, iou_off=off, iou_n=n, cm_conf=S.CM_CONF, cm_iou=S.CM_IOU, tp=tp, matrix=matrix)
    assert torch.equal(tp, tp0) and torch.equal(matrix, m0)
    # T = 1; either output alone
    tp1, _ = _outputs(B, 1, nc)
    _ops.match_batch(rows, count, cls, gt_off, S.IOUV[:1], nc, gt=gt, tp=tp1)
    _check(group, tp1, None, nc, T=1)
    _, m1 = _outputs(B, 1, nc)
    _ops.match_batch(rows, count, cls, gt_off, S.IOUV[:1], nc, gt=gt, cm_conf=S.CM_CONF, cm_iou=S.CM_IOU, matrix=m1)
    assert torch.equal(m1, m0)


def test_public_forms_and_obb(cases):
    """metrics.match_batch / ConfusionMatrix on device tensors: the batch forms, the per-image form, and oriented rows on ey_probiou."""
    from edge_yolo_amd.utils import metrics
    group = _group(cases, 80)
    rows, count = _pack(group, "det", 6)
    gt_off = np.concatenate([[0], np.cumsum([len(c["gt"]) for c in group])]).tolist()
    gt, cls = np.concatenate([c["gt"] for c in group]), np.concatenate([c["gt_cls"] for c in group])
    xform = np.stack([S.xform_row(c["ori_shape"], c["ratio_pad"]) for c in group])
    cm = metrics.ConfusionMatrix(80, conf=0.001)
    tp = cm.process_device_batch(rows, count, gt, cls, gt_off, xform=xform, iouv=S.IOUV)
    tp2 = metrics.match_batch(rows, gt, cls, S.IOUV, count=count, gt_off=gt_off, nc=80, xform=xform)
    want = sum(c["matrix"] for c in group)
    assert torch.equal(tp, tp2) and np.array_equal(cm.matrix, want) and cm.matrix.dtype == np.float64
    for i, c in enumerate(group):
        assert np.array_equal(tp[i, :len(c["det"])].cpu().numpy(), c["tp"].astype(np.uint8)) and not tp[i, len(c["det"]):].any()
    one = metrics.ConfusionMatrix(80)
    for c in group:
        one.process_batch(torch.from_numpy(c["predn"]).cuda(), torch.from_numpy(c["gt"]).cuda(), torch.from_numpy(c["gt_cls"]).cuda())
    assert np.array_equal(one.matrix, want)
    for c in cases[1]:
        o = metrics.ConfusionMatrix(c["nc"])
        o.process_batch(torch.from_numpy(c["det"]).cuda(), c["gt"], c["gt_cls"])
        assert np.array_equal(o.matrix, c["matrix"]), c["name"]


def test_oriented_cases_batched_in_matrix_mode(cases):
    """Every oriented fixture case in ONE launch (B = 5) in matrix mode on ey_probiou_batch's buffer: tp and matrix against the reference's
    match_predictions / process_batch on its batch_probiou.  The launch has one class count, 15; the cases recorded with 3 classes use
    classes 0..2 of it, and their matrices' background row and column (index 3) are the launch's (index 15)."""
    from edge_yolo_amd.nn import _ops
    group, nc = list(cases[1]), 15
    B = len(group)
    assert B >= 3 and {c["nc"] for c in group} == {3, 15}
    n, nl = [len(c["det"]) for c in group], [len(c["gt"]) for c in group]
    buf = torch.full((B, MAX_DET, 7), float("nan"))
    for i, c in enumerate(group):
        buf[i, :n[i]] = torch.from_numpy(c["det"])
    rows, count = buf.cuda(), torch.tensor(n, dtype=torch.int32).cuda()
    pk = torch.from_numpy(np.concatenate([c["det"][:, [0, 1, 2, 3, 6]] for c in group]).astype(np.float32)).cuda()
    gk = torch.from_numpy(np.concatenate([c["gt"] for c in group]).astype(np.float32)).cuda()
    pred_off, gt_off = np.concatenate([[0], np.cumsum(n)]).tolist(), np.concatenate([[0], np.cumsum(nl)]).tolist()
    flat, off = _ops.probiou_batch(pk, pred_off, gk, gt_off)
    cls = torch.from_numpy(np.concatenate([c["gt_cls"] for c in group]).astype(np.int32)).cuda()
    tp, matrix = _outputs(B, 10, nc)
    _ops.match_batch(rows, count, cls, gt_off, S.IOUV, nc, iou=flat, iou_off=off, iou_n=n, cm_conf=S.CM_CONF, cm_iou=S.CM_IOU, tp=tp, matrix=matrix)
    _check(group, tp, None, nc)
    want = np.zeros((nc + 1, nc + 1), np.int64)
    for c in group:
        at = np.r_[np.arange(c["nc"]), nc]  # the case's classes, then its background
        want[np.ix_(at, at)] += c["matrix"]
    assert np.array_equal(matrix.cpu().numpy().reshape(nc + 1, nc + 1), want) and want.sum() > 250


def test_refusals_leave_both_outputs_untouched(cases):
    from edge_yolo_amd import _lib as L
    from edge_yolo_amd.nn import _ops
    from edge_yolo_amd.utils import metrics
    group = _group(cases, 3)
    rows, count = _pack(group, "predn", 6)
    gt, cls, gt_off = _labels(group)
    B = len(group)
    tp = torch.full((B, MAX_DET, 10), SENT, dtype=torch.uint8).cuda()
    matrix = torch.full((16,), -7, dtype=torch.int32).cuda()

    def untouched():
        torch.cuda.synchronize()
        return bool((tp == SENT).all()) and bool((matrix == -7).all())

    with pytest.raises(ValueError):  # T out of range
        _ops.match_batch(rows, count, cls, gt_off, np.linspace(0.1, 0.9, 17), 3, gt=gt, tp=torch.full((B, MAX_DET, 17), SENT, dtype=torch.uint8).cuda(), matrix=matrix)
    lib = L.lib()
    thr = _ops._fa(S.IOUV)
    args = lambda T=10, gt_p=gt.data_ptr(), off=gt_off: (B, MAX_DET, 6, rows.data_ptr(), count.data_ptr(), None, gt_p, cls.data_ptr(), _ops._ia(off), None, None, None,  # noqa: E731
                                                           T, thr, 3, 0.25, 0.45, tp.data_ptr(), matrix.data_ptr(), L.stream())
    assert lib.ey_match_batch(*args(T=0)) == -1 and lib.ey_match_batch(*args(T=17)) == -1 and untouched()
    assert lib.ey_match_batch(*args(gt_p=None)) == -1 and untouched()
    # more labels in one image than the LDS holds: EY_EUNSUPPORTED before anything is launched, with the limit named
    big = [0] + [40000] * B
    assert lib.ey_match_batch(*args(off=big)) == -2 and b"163840" in lib.ey_last_error() and untouched()
    with pytest.raises(ValueError, match="class ids"):  # a host label outside [0, nc): refused before the upload
        metrics.match_batch(rows, gt.cpu().numpy(), np.where(np.arange(gt_off[-1]) == 1, 3, 0), S.IOUV, count=count, gt_off=gt_off, nc=3)
    assert untouched()


def test_large_image_runs_from_lds():
    """1024 rows x 1024 labels x 16 thresholds in one image (the documented capacity): against the numpy closed form."""
    from edge_yolo_amd.nn import _ops
    from edge_yolo_amd.utils import metrics
    g = S.case(("big", 1024, 1024, 5, False), 5)
    iouv = np.linspace(0.3, 0.9, 16)
    rows = torch.from_numpy(g["det"])[None].cuda()
    count = torch.tensor([1024], dtype=torch.int32).cuda()
    tp = torch.zeros((1, 1024, 16), dtype=torch.uint8).cuda()
    matrix = torch.zeros(36, dtype=torch.int32).cuda()
    _ops.match_batch(rows, count, torch.from_numpy(g["gt_cls"].astype(np.int32)).cuda(), [0, 1024], iouv, 5, gt=torch.from_numpy(g["gt"]).cuda(), tp=tp, matrix=matrix)
    want = metrics.match_batch(g["det"], g["gt"], g["gt_cls"], iouv)
    cm = metrics.ConfusionMatrix(5)
    cm.process_batch(g["det"], g["gt"], g["gt_cls"])
    assert np.array_equal(tp[0].cpu().numpy() != 0, want) and want[:, 0].sum() > 100
    assert np.array_equal(matrix.cpu().numpy().reshape(6, 6), cm.matrix)
