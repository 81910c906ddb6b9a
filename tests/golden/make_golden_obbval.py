"""Golden vectors for obb validation: non_max_suppression(multi_label=True, rotated=True) (reference ultralytics/utils/ops.py:270-297 with
nms_rotated :146-164), batch_probiou per image (utils/metrics.py:244-275) and an end-to-end case run through the reference's own
OBBValidator.update_metrics / get_stats / OBBMetrics (models/yolo/obb/val.py, utils/metrics.py:1240-1308), from the real reference imported
through _ref_import.  CPU fp32, synthetic weights and inputs (tests/obbval_synth.py, tests/obb_synth.py).  The rotated path of the reference's
NMS is pure torch.

    python tests/golden/make_golden_obbval.py

writes obbval_ops.npz and obbval_case.npz.  Every NMS case takes the first seed at which every column's float64 margin |colmax - thr|
(tests/fp64_obbval_ref.py) exceeds 1e-3 and all candidate scores are distinct (both asserted); the reference's rows then equal the
restatement's bit for bit (asserted too).  The files hold seeds, kept (anchor, class) lists and rows, not candidate matrices.  The validation
case takes the first image seed at which, besides that, every [ground truth x prediction] ProbIoU is further than 1e-4 (float64) from each of
the thresholds 0.50:0.05:0.95, no class score is within 1e-4 of conf (conf is put into the widest gap of the batch's scores), the kept rows'
scores are more than 1e-4 apart within an image and, for rows of one class, across the batch (ap_per_class orders a class's rows over all
images), and no two candidates whose scores are within 1e-4 suppress one another: a forward that agrees to a few 1e-5 then keeps the same
rows in the same order.  Precision and recall are read off curves over the confidences: the case is one where the reference's
ap_per_class gives the same four means (to 1e-9) when every confidence moves by up to 5e-5 (asserted; the gaps and the shift are stored).
Runs only where the reference exists."""
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
import _ref_import  # noqa: E402

_ref_import.setup()
import numpy as np  # noqa: E402
import torch  # noqa: E402
import yaml  # noqa: E402

import fp64_obb_ref as f64  # noqa: E402
import fp64_obbval_ref as f64v  # noqa: E402
import obb_synth  # noqa: E402
import obbval_synth as S  # noqa: E402
import synthdata as synth  # noqa: E402
from ultralytics.models.yolo.obb.val import OBBValidator as ROV  # noqa: E402
from ultralytics.nn.tasks import OBBModel  # noqa: E402
from ultralytics.utils import metrics as rm  # noqa: E402
from ultralytics.utils import ops as rops  # noqa: E402

torch.set_grad_enabled(False)
CFG = os.path.join(ROOT, "edge-yolo_amd", "cfg", "models", "11")


def _save(name, d):
    path = os.path.join(HERE, name)
    np.savez_compressed(path, **{k: (v.numpy() if torch.is_tensor(v) else v) for k, v in d.items()})
    size = os.path.getsize(path)
    print(name, len(d), size)
    assert size < 1 << 20, name


def ref_kept(pred_b, rows, nc):
    """(anchor, class) of each reference row: rows copy the input's values and candidate scores are distinct, so the score names the pair."""
    sc = pred_b[4:4 + nc].numpy()
    where = {}
    for c in range(nc):
        for a in range(sc.shape[1]):
            where.setdefault(sc[c, a].item(), []).append((a, c))
    out = []
    for r in rows:
        (a, c), = where[r[4].item()]
        assert c == int(r[5]) and all(r[k].item() == pred_b[k, a].item() for k in range(4)) and r[6].item() == pred_b[4 + nc, a].item()
        out.append((a, c))
    return np.array(out, np.int64).reshape(-1, 2)


def nms_cases(d):
    for case in S.NMS_CASES:
        tag, nc, A = case["tag"], case["nc"], case["A"]
        kw = dict(conf_thres=case["conf"], iou_thres=case["iou"], classes=case["classes"], agnostic=case["agnostic"], nc=nc, max_nms=case["max_nms"],
                  max_time_img=1e6, multi_label=True, rotated=True)
        for seed in range(200):
            pred = S.nms_case(case, seed)
            ora = f64v.nms_rotated_ml64(pred.numpy(), case["conf"], case["iou"], case["classes"], case["agnostic"], case["max_det"], case["max_nms"], S.MAX_WH)
            worst = min([float(o["margin"].min()) for o in ora if len(o["margin"])] or [1.0])
            ok = worst > S.MARGIN and f64v.distinct_scores(pred.numpy(), case["conf"])
            if tag == "ml_cut":  # the anchor of the last survivor has a class beyond the cut as well
                o = ora[0]
                cut_a = f64v.candidates_ml(pred[0].numpy(), nc, case["conf"], None, A * nc)[0][case["max_nms"]:]
                ok = ok and o["anchor"][-1] in cut_a
            if ok:
                break
        assert ok and worst > S.MARGIN and f64v.distinct_scores(pred.numpy(), case["conf"]), tag
        rows = rops.non_max_suppression(pred.clone(), max_det=case["max_det"], **kw)
        full = rops.non_max_suppression(pred.clone(), max_det=A * nc, **kw)  # every kept column: the reference's own flags
        d[tag + "_seed"] = np.int64(seed)
        d[tag + "_margin"] = np.float64(worst)
        E = 0.0
        for b, o in enumerate(ora):
            d[f"{tag}_rows{b}"] = rows[b].numpy().astype(np.float32).reshape(-1, 7)
            d[f"{tag}_kept{b}"] = ref_kept(pred[b], full[b], nc)
            d[f"{tag}_total{b}"] = np.int64(o["total"])
            if len(o["boxes"]):
                bt = torch.tensor(o["boxes"])
                err = np.abs(rm.batch_probiou(bt, bt).numpy().astype(np.float64) - f64.probiou64(o["boxes"], o["boxes"]))
                E = max(E, float(np.triu(err, 1).max()))
            np.testing.assert_array_equal(rows[b].numpy().reshape(-1, 7), o["rows"], err_msg=tag)
            np.testing.assert_array_equal(d[f"{tag}_kept{b}"][:, 0], o["anchor"][o["keep"]], err_msg=tag)
            np.testing.assert_array_equal(d[f"{tag}_kept{b}"][:, 1], o["cls"][o["keep"]], err_msg=tag)
        d[tag + "_E"] = np.float64(E)
        print(tag, "seed", seed, "candidates", [o["total"] for o in ora], "after the cut", [len(o["anchor"]) for o in ora], "kept", [len(r) for r in rows],
              f"worst margin {worst:.2e} E {E:.2e}")
    t = S.NMS_BY_TAG
    assert all(d[f"{k}_total0"] == t[k]["counts"][0] for k in ("ml_exact_max_nms", "ml_max_nms_plus1")) and d["ml_all270_total0"] == 270
    assert d["ml_b3_empty_total1"] == 0 and d["ml_large_total0"] == d["ml_large_total1"] == 6000
    # one anchor, three classes: all three rows without the class offset's help only the best
    for tag, want in (("ml_triple", 3), ("ml_triple_agnostic", 1)):
        assert int((d[tag + "_kept0"][:, 0] == S.TRIPLE_ANCHOR).sum()) == want, tag


def pair_cases(d):
    pred, gt, poff, goff = S.pair_case()
    E = 0.0
    for b in range(len(S.PAIR_SIZES)):
        p, g = pred[poff[b]:poff[b + 1]], gt[goff[b]:goff[b + 1]]
        if len(p) and len(g):
            d[f"pb_{b}"] = rm.batch_probiou(torch.tensor(g), torch.tensor(p))
            E = max(E, float(np.abs(d[f"pb_{b}"].numpy().astype(np.float64) - f64.probiou64(g, p)).max()))
    print("probiou_batch E", f"{E:.2e}")


# ---------------------------------------------------------------------------------------------------------------- the validation case
def _validator():
    class V(ROV):
        def __init__(self):  # the validator's own set-up needs a dataset / cfg; only the metric plumbing is exercised
            pass
    v = V()
    v.device = torch.device("cpu")
    v.args = types.SimpleNamespace(single_cls=False, plots=False, save_json=False, save_txt=False, save_conf=False)
    v.iouv = torch.linspace(0.5, 0.95, 10)
    v.niou, v.nc, v.seen, v.batch_i = 10, 80, 0, 0
    v.names = {i: str(i) for i in range(80)}
    v.metrics = rm.OBBMetrics(names=v.names)
    v.stats = dict(tp=[], conf=[], pred_cls=[], target_cls=[], target_img=[])
    v.confusion_matrix = None
    return v


SCORE_GAP = 1e-4  # scores further apart than this keep their order when the forward agrees to a few 1e-5 (the fp32 runs agree to about 1e-5)
LABELS_PER_IMAGE = [4, 0, 5, 3]  # image 1 has no labels


def _labels(preds, r, H, W):
    """ground truth made from the predictions: picked rows, disturbed; xywh normalised to the input frame, the angle as it is."""
    cls, box, bidx = [], [], []
    for i, q in enumerate(preds):
        k = LABELS_PER_IMAGE[i]
        pick = r.permutation(len(q))[:k]
        assert len(pick) == k, (i, len(q))
        for j in pick:
            x, y, w, h = q[j, :4].numpy().astype(np.float64)
            x, y = np.clip(x + r.normal(0, 1.5), 1, W - 1), np.clip(y + r.normal(0, 1.5), 1, H - 1)
            w, h = min(w, W) * r.uniform(0.7, 1.0), min(h, H) * r.uniform(0.7, 1.0)
            c = float(q[j, 5]) if r.random() < 0.8 else float(r.integers(0, 80))
            cls.append([c]); bidx.append(i)
            box.append([x / W, y / H, w / W, h / H, float(q[j, 6]) + r.normal(0, 0.05)])
    return torch.tensor(cls, dtype=torch.float32), torch.tensor(np.array(box), dtype=torch.float32), torch.tensor(bidx, dtype=torch.float32)


def _iou_margin(v, preds, batch):
    """smallest |value - threshold| over every [gt x pred] ProbIoU of the batch, in float64 on the reference's own prepared values."""
    worst, pairs = 1.0, 0
    for si, pred in enumerate(preds):
        pb = v._prepare_batch(si, batch)
        if not len(pb["cls"]) or not len(pred):
            continue
        predn = v._prepare_pred(pred, pb)
        m = f64.probiou64(pb["bbox"].numpy(), torch.cat([predn[:, :4], predn[:, -1:]], -1).numpy())
        worst = min(worst, float(np.abs(m[..., None] - S.THRESHOLDS).min()))
        pairs += m.size
    return worst, pairs


def _stable(y, conf, iou):
    """the conditions of the module docstring under which a forward within 1e-4 keeps the same rows in the same order; -> (ok, text)."""
    ora = f64v.nms_rotated_ml64(y, conf, iou, None, False, 300, 30000, S.MAX_WH)
    for o in ora:
        if len(o["margin"]) and o["margin"].min() <= S.MARGIN:
            return False, f"margin {o['margin'].min():.1e}"
    for p, o in zip(y, ora):
        sc = p[4:-1]
        if (np.abs(sc.astype(np.float64) - conf) < SCORE_GAP).any():
            return False, "a score next to conf"
        s = o["score"].astype(np.float64)
        kept = s[o["keep"]]
        if len(kept) > 1 and (kept[:-1] - kept[1:]).min() <= SCORE_GAP:
            return False, "kept scores too close"
        iou64 = f64.probiou64(o["boxes"], o["boxes"])
        close = np.abs(s[:, None] - s[None, :]) < SCORE_GAP
        np.fill_diagonal(close, False)
        if (iou64[close] > iou - S.MARGIN).any():
            return False, "near-equal scores that suppress one another"
    if _class_gap(ora) <= SCORE_GAP:  # ap_per_class orders a class's rows across the images of the batch
        return False, "kept scores of one class, in different images, too close"
    return True, ""


def _class_gap(ora):
    """smallest distance between the scores of two kept rows of the same class anywhere in the batch."""
    s = np.concatenate([o["score"][o["keep"]].astype(np.float64) for o in ora])
    c = np.concatenate([o["cls"][o["keep"]] for o in ora])
    gap = 1.0
    for k in np.unique(c):
        t = np.sort(s[c == k])
        if len(t) > 1:
            gap = min(gap, float(np.diff(t).min()))
    return gap


def _gaps(y, conf, ora):
    """(smallest |class score - conf|, smallest gap between consecutive kept scores of an image, _class_gap) of the batch."""
    near = float(np.abs(y[:, 4:-1].astype(np.float64) - conf).min())
    kept = min([float(-np.diff(o["score"][o["keep"]].astype(np.float64)).min()) for o in ora if o["keep"].sum() > 1] or [1.0])
    return near, kept, _class_gap(ora)


def _metric_shift(stats):
    """largest change of precision, recall, mAP50 and mAP50-95 (the reference's ap_per_class) when every confidence moves by up to half of
    SCORE_GAP: all up, all down, and 20 random patterns."""
    def run(conf):
        p, r, _, ap = rm.ap_per_class(stats["tp"], conf, stats["pred_cls"], stats["target_cls"])[2:6]
        return np.array([p.mean(), r.mean(), ap[:, 0].mean(), ap.mean()])
    base, worst = run(stats["conf"]), 0.0
    rng = np.random.default_rng(3)
    n = len(stats["conf"])
    for delta in [np.full(n, 1.0), np.full(n, -1.0)] + [rng.uniform(-1, 1, n) for _ in range(20)]:
        worst = max(worst, float(np.abs(run((stats["conf"] + delta * SCORE_GAP / 2).astype(stats["conf"].dtype)) - base).max()))
    return worst


def _ref_stats(preds, base, variant="full"):
    v = _validator()
    ps = [q.clone() if not (variant == "nopred" and i == 3) else q[:0].clone() for i, q in enumerate(preds)]
    v.update_metrics(ps, dict(base))
    return v, {k: torch.cat(t, 0).cpu().numpy() for k, t in v.stats.items()}


def case_file():
    d_cfg = yaml.safe_load(open(os.path.join(CFG, "yolo11-obb.yaml"), encoding="utf-8"))
    d_cfg["scale"] = "n"
    m = OBBModel(d_cfg, ch=3, nc=80, verbose=False).eval()
    m.load_state_dict(obb_synth.state_dict(m.state_dict()))
    m.fuse(verbose=False)
    B, H, W = 4, 64, 96
    iou = 0.7
    ori = [(64, 96), (128, 128), (100, 160), (48, 72)]
    ratio_pad = []
    for h0, w0 in ori:  # LetterBox geometry (data/augment.py:1556-1591) as the dataset records it
        g = min(H / h0, W / w0)
        nw, nh = round(w0 * g), round(h0 * g)
        dw, dh = (W - nw) / 2, (H - nh) / 2
        ratio_pad.append(((g, g), (int(round(dw - 0.1)), int(round(dh - 0.1)))))
    found = False
    for image_seed in range(200):
        x = synth.synth_images(B, H, W, seed=image_seed)
        y, _ = m(x)
        # the synthetic weights put every class score near 0.5: conf leaves some tens of candidates per image, and sits in the middle of the
        # widest gap between the batch's scores in [0.61, 0.64]
        pool = np.sort(y[:, 4:-1].numpy().astype(np.float64).ravel())
        pool = pool[(pool > 0.61) & (pool < 0.64)]
        k = int(np.argmax(np.diff(pool)))
        conf = round(float(pool[k] + pool[k + 1]) / 2, 6)
        ok, why = _stable(y.numpy(), conf, iou)
        if not ok:
            print("image seed", image_seed, why)
            continue
        preds = rops.non_max_suppression(y.clone(), conf, iou, multi_label=True, max_det=300, nc=80, max_time_img=1e6, rotated=True)
        if min(len(q) for q in preds) < max(LABELS_PER_IMAGE):
            print("image seed", image_seed, "too few rows", [len(q) for q in preds])
            continue
        for seed in range(50):
            cls, box, bidx = _labels(preds, np.random.default_rng([11, seed]), H, W)
            base = dict(img=x, cls=cls, bboxes=box, batch_idx=bidx, ori_shape=ori, ratio_pad=ratio_pad, im_file=[f"im{i}.jpg" for i in range(B)])
            worst, pairs = _iou_margin(_validator(), [q.clone() for q in preds], base)
            if worst > S.IOU_MARGIN and _ref_stats(preds, base)[1]["tp"].any():
                shift = _metric_shift(_ref_stats(preds, base)[1])
                if shift < 1e-9:  # precision and recall are read off curves over the confidences: here they do not move with them
                    found = True
                    break
                print("image seed", image_seed, "label seed", seed, f"the metrics move by {shift:.1e} with the confidences")
        print("image seed", image_seed, "label seed", seed, f"worst IoU margin {worst:.2e} over {pairs} values, rows {[len(q) for q in preds]}")
        if found:
            break
    assert found
    ora = f64v.nms_rotated_ml64(y.numpy(), conf, iou, None, False, 300, 30000, S.MAX_WH)
    single = rops.non_max_suppression(y.clone(), conf, iou, max_det=300, nc=80, max_time_img=1e6, rotated=True)
    assert sum(len(q) for q in preds) > sum(len(q) for q in single), "the case must have anchors with several classes"
    d = dict(image_seed=np.int64(image_seed), seed=np.int64(seed), margin=np.float64(worst), conf=np.float64(conf), iou=np.float64(iou), cls=cls.numpy(),
             bboxes=box.numpy(), batch_idx=bidx.numpy(), ori_shape=np.array(ori), ratio_gain=np.array([rp[0][0] for rp in ratio_pad]),
             ratio_padwh=np.array([rp[1] for rp in ratio_pad]), empty_pred_image=np.int64(3), image_shape=np.array([B, H, W]),
             nms_margin=np.float64(min(float(o["margin"].min()) for o in ora if len(o["margin"]))), score_gap=np.float64(SCORE_GAP),
             metric_shift=np.float64(shift))
    d["gap_conf"], d["gap_kept"], d["gap_class"] = (np.float64(t) for t in _gaps(y.numpy(), conf, ora))
    assert min(d["gap_conf"], d["gap_kept"], d["gap_class"]) > SCORE_GAP and shift < 1e-9
    print("gaps", float(d["gap_conf"]), float(d["gap_kept"]), float(d["gap_class"]), "metric shift", shift)
    for i, (q, o) in enumerate(zip(preds, ora)):
        d[f"pred{i}"] = q.numpy()
        np.testing.assert_array_equal(q.numpy(), o["rows"])
    # two runs of the reference's validator: all predictions ("full", what a model run reproduces) and image 3's predictions removed
    # ("nopred": labels without predictions, the npr == 0 bookkeeping)
    for variant in ("full", "nopred"):
        v, _ = _ref_stats(preds, base, variant)
        d[variant + "_tp"] = torch.cat(v.stats["tp"], 0).numpy()
        d[variant + "_conf"] = torch.cat(v.stats["conf"], 0).numpy()
        res = v.get_stats()
        d[variant + "_keys"], d[variant + "_values"] = np.array(list(res.keys())), np.array([float(t) for t in res.values()])
        d[variant + "_means"] = np.array([float(t) for t in v.metrics.box.mean_results()])  # precision, recall, mAP50, mAP75, mAP50-95
        d[variant + "_seen"], d[variant + "_nt_per_class"] = np.int64(v.seen), v.nt_per_class
        d[variant + "_ap"], d[variant + "_ap_class_index"] = v.metrics.box.all_ap, np.asarray(v.metrics.box.ap_class_index)
        print(variant, dict(zip(res.keys(), d[variant + "_values"])), "tp", d[variant + "_tp"].shape, int(d[variant + "_tp"].sum()))
        assert d[variant + "_tp"].any()
    _save("obbval_case.npz", d)


if __name__ == "__main__":
    if "case" not in sys.argv[1:]:  # (`... make_golden_obbval.py case` writes obbval_case.npz alone)
        ops = {}
        nms_cases(ops)
        pair_cases(ops)
        _save("obbval_ops.npz", ops)
    case_file()
