"""-m gpu: the validators' confusion_matrix / device_match keywords end to end, at 64x96, B = 2, two batches.  The labels are synthetic: the
best few kept rows of each image, some with another class, plus a stray, so that there are matches at several thresholds.  For yolo11n
(detect), -seg, -pose and -obb (validator=OBBValidator): `val(loader, confusion_matrix=True, device_match=True)` returns a results_dict
EQUAL (==) to plain `val(loader)`, its `stats` arrays equal the plain run's, and its confusion matrix equals the numpy route's on the same
kept rows; yolo11n-cls: the matrix against the host route."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import cls_synth  # noqa: E402
import obb_synth  # noqa: E402
import parent_image_stats  # noqa: E402
import pose_synth  # noqa: E402
import seg_synth  # noqa: E402
import synthdata as synth  # noqa: E402

H, W, B = 64, 96, 2


def _facade(cfg, state):
    import edge_yolo_amd
    y = edge_yolo_amd.YOLO(cfg)
    y.model.load_state_dict(state(y.model.state_dict()))
    return y


def _labels_from(rows, task, seed, nc, kpt_shape=None):
    """rows: per image the kept rows on the host -> the label part of a batch: the best rows with distinct boxes, their sizes and places moved
    by a percent or two (so that no two labels have equal IoUs), as labels, every third with another class where there is one."""
    rng = np.random.default_rng(seed)
    cls, box, bi, kp = [], [], [], []
    masks = np.zeros((len(rows), H // 4, W // 4), np.int32)
    for i, r in enumerate(rows):
        r = r[np.argsort(-r[:, 4], kind="stable")]
        first = [k for k in range(min(len(r), 64)) if not any(np.array_equal(r[k, :4], r[j, :4]) for j in range(k))]  # multi-label NMS repeats a box per class
        r = r[first[: 3 + i]]
        b = r[:, :4].astype(np.float64)
        if task != "obb":  # xyxy -> xywh
            b = np.stack([(b[:, 0] + b[:, 2]) / 2, (b[:, 1] + b[:, 3]) / 2, b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]], 1)
        b = b * (1 + rng.normal(0, 0.015, b.shape))
        b = np.concatenate([b, [[W / 2, H / 2, W / 5, H / 5]]])  # a stray label
        c = np.concatenate([r[:, 5], [0]])
        c[2::3] = (c[2::3] + 1) % nc
        ang = np.concatenate([r[:, 6], [0.3]]) if task == "obb" else None
        b = b / [W, H, W, H]
        box.append(np.concatenate([b, ang[:, None]], 1) if task == "obb" else b)
        cls.append(c.reshape(-1, 1))
        bi.append(np.full(len(c), i))
        for m, q in enumerate(b):  # the instance's box as its mask, at proto resolution
            x0, y0, x1, y1 = (q[0] - q[2] / 2) * W / 4, (q[1] - q[3] / 2) * H / 4, (q[0] + q[2] / 2) * W / 4, (q[1] + q[3] / 2) * H / 4
            masks[i, max(int(y0), 0):int(np.ceil(y1)), max(int(x0), 0):int(np.ceil(x1))] = m + 1
        if kpt_shape:
            K = kpt_shape[0]
            k = np.concatenate([b[:, None, :2] + (rng.random((len(b), K, 2)) - 0.5) * b[:, None, 2:4], np.full((len(b), K, 1), 2.0)], 2)
            kp.append(k)
    out = {"cls": np.concatenate(cls).astype(np.float32), "bboxes": np.concatenate(box).astype(np.float32), "batch_idx": np.concatenate(bi).astype(np.float32),
           "ori_shape": [(H, W)] * len(rows), "ratio_pad": None}
    if task == "segment":
        out["masks"] = masks
    if kpt_shape:
        out["keypoints"] = np.concatenate(kp).astype(np.float32)
    return out


def _loader(y, vcls, task, **kw):
    """Two batches whose labels come from the model's own kept rows."""
    v = vcls(y._ready(torch.device("cuda:0"), False), device="cuda:0", **kw)
    loader = []
    for j in range(2):
        img = synth.synth_images(B, H, W, seed=20 + j)
        with torch.no_grad(), torch.cuda.device(v.device):
            out = v.postprocess(v._forward(v.preprocess({"img": img, "masks": np.zeros((B, H // 4, W // 4), np.int32)})["img"]))
        rows = [r.float().cpu().numpy() for r in (out[0] if isinstance(out, tuple) else out)]
        assert all(len(r) >= 3 for r in rows), [len(r) for r in rows]
        kpt = [int(t) for t in y.model.model[-1].kpt_shape] if task == "pose" else None
        loader.append(dict(_labels_from(rows, task, 5 + j, len(y.model.names), kpt), img=img))
    return loader


def _stats_equal(a, b):
    assert list(a.stats) == list(b.stats)
    for k in a.stats:
        assert len(a.stats[k]) == len(b.stats[k]), k
        for x, z in zip(a.stats[k], b.stats[k]):
            assert x.dtype == z.dtype and x.shape == z.shape and np.array_equal(x, z), k


TASKS = {"detect": ("yolo11n.yaml", lambda sd: synth.synth_state_dict({k: tuple(t.shape) for k, t in sd.items()})),
         "segment": ("yolo11n-seg.yaml", seg_synth.state_dict), "pose": ("yolo11n-pose.yaml", pose_synth.state_dict),
         "obb": ("yolo11n-obb.yaml", obb_synth.state_dict)}


@pytest.mark.parametrize("task", list(TASKS))
def test_val_with_both_keywords_equals_plain_val(task):
    from edge_yolo_amd.engine import validator as V
    vcls = {"detect": V.DetectionValidator, "segment": V.SegmentationValidator, "pose": V.PoseValidator, "obb": V.OBBValidator}[task]
    y = _facade(*TASKS[task])
    extra = {"validator": V.OBBValidator} if task == "obb" else {}
    loader = _loader(y, vcls, task)
    plain = dict(y.val(loader, device="cuda:0", **extra))
    pv = y.validator
    both = dict(y.val(loader, device="cuda:0", confusion_matrix=True, device_match=True, **extra))
    bv = y.validator
    print(f"\n[{task}] results {plain}\n matrix sum {bv.confusion_matrix.matrix.sum()} trace {np.trace(bv.confusion_matrix.matrix)} "
          f"tp50 {int(np.concatenate(pv.stats['tp'])[:, 0].sum())} rows {len(np.concatenate(pv.stats['tp']))}")
    assert both == plain and pv.confusion_matrix is None and isinstance(bv, vcls)
    _stats_equal(bv, pv)
    assert np.concatenate(pv.stats["tp"])[:, 0].sum() >= 4 and plain["metrics/mAP50(B)"] > 0
    only = dict(y.val(loader, device="cuda:0", confusion_matrix=True, **extra))  # the matrix alone: the statistics stay on the host route
    assert only == plain and np.array_equal(y.validator.confusion_matrix.matrix, bv.confusion_matrix.matrix)
    _stats_equal(y.validator, pv)
    # the numpy route on the same kept rows
    d = vcls(y.model, device="cuda:0")
    d.keep_outputs = True
    h = vcls(y.model, device="cuda:0", confusion_matrix=True)
    par = vcls(y.model, device="cuda:0")  # detect: fed through the statistics loop as it stood before the keywords existed
    for batch in loader:
        pb = d.preprocess(batch)
        with torch.no_grad(), torch.cuda.device(d.device):
            out = d.postprocess(d._forward(pb["img"]))
            d.kept = []
            d.update_metrics(out, pb)
        hb = dict(pb, img=pb["img"].cpu())
        if task == "detect":
            parent_image_stats.image_stats(par, out, pb)
        if task in ("detect", "obb"):
            h.update_metrics([r.float().cpu().numpy() for r in out], hb)
        elif task == "segment":
            hb["masks"] = pb["masks"].cpu()
            h.update_metrics(([r for r, _ in d.kept], None), hb, pred_masks=[k for _, k in d.kept])
        else:
            h.update_metrics(([r for r, _ in d.kept], [k for _, k in d.kept]), hb)
    m = bv.confusion_matrix.matrix
    assert np.array_equal(h.confusion_matrix.matrix, m) and m.dtype == np.float64 and m.shape == (bv.nc + 1, bv.nc + 1)
    if task == "detect":
        _stats_equal(par, pv)
        assert par.get_stats() == plain
    labels = np.bincount(np.concatenate([b["cls"].reshape(-1) for b in loader]).astype(int), minlength=bv.nc)
    assert np.array_equal(m[:, :-1].sum(0), labels)  # every label is counted once, in its class's column: matched or background
    assert m[:, -1].sum() + m[:-1, :-1].sum() <= sum(len(x) for x in pv.stats["conf"]) and m[-1, -1] == 0


def test_classify_matrix_equals_host_route():
    from edge_yolo_amd.utils import metrics
    nc = 10
    import edge_yolo_amd
    y = edge_yolo_amd.YOLO("yolo11n-cls.yaml", nc=nc)
    y.model.load_state_dict(cls_synth.state_dict(y.model.state_dict()))
    loader = [{"img": synth.synth_images(B, 64, 64, seed=30 + j), "cls": np.array([j, (3 * j + 1) % nc])} for j in range(2)]
    plain = dict(y.val(loader, device="cuda:0"))
    assert y.validator.confusion_matrix is None
    res = dict(y.val(loader, device="cuda:0", confusion_matrix=True))
    v = y.validator
    want = metrics.ConfusionMatrix(nc, task="classify")
    want.process_cls_preds(v.pred, v.targets)
    assert res == plain and np.array_equal(v.confusion_matrix.matrix, want.matrix) and want.matrix.shape == (nc, nc) and want.matrix.sum() == 2 * B
