"""Golden vectors for segment validation, from the real reference imported through _ref_import: mask_iou (utils/metrics.py:137-153), the
overlap_mask expansion of SegmentationValidator._process_batch (models/yolo/segment/val.py:204-213) and an end-to-end case run through the
reference's own SegmentationValidator.update_metrics / get_stats / SegmentMetrics.  CPU fp32, synthetic weights (tests/seg_synth.py).

    python tests/golden/make_golden_segval.py

writes segval_ops.npz and segval_case.npz.  Mask bits are stored with np.packbits.  Runs only where the reference exists.
"""
import os
import types

import make_golden_seg as mgs  # (sets up the reference import and the NMS stand-in of make_golden.py)
import numpy as np
import torch

import seg_synth
import synthdata as synth
from ultralytics.models.yolo.segment.val import SegmentationValidator as RSV
from ultralytics.nn.tasks import SegmentationModel
from ultralytics.utils import metrics as rm
from ultralytics.utils import ops as rops

torch.set_grad_enabled(False)
HERE = mgs.HERE


def _rand_masks(r, k, n, density):
    return (r.random((k, n)) < density).astype(np.uint8)


def ops_file():
    d = {}
    r = np.random.default_rng(11)
    cases = []
    for tag, M, N, n in (("a", 5, 7, 35), ("b", 3, 4, 64), ("c", 9, 6, 65), ("d", 4, 70, 640), ("e", 2, 3, 1)):
        g, p = _rand_masks(r, M, n, 0.5), _rand_masks(r, N, n, 0.3)
        g[0] = 0                      # all-zero row
        p[0] = 1                      # all-one row
        if M > 1:
            g[1] = p[min(1, N - 1)]   # identical pair
        if M > 2 and N > 2:           # disjoint pair
            g[2] = 1 - p[2]
        if N > 3 and n > 1:           # union of 1: one pixel on each side, the same one / one pixel against none
            p[3] = 0
            p[3, n // 2] = 1
            if M > 3:
                g[3] = p[3]
        cases.append((tag, g, p))
    z = np.zeros((2, 9), np.uint8)
    cases.append(("zero", z, z.copy()))  # union of 0 everywhere -> exactly 0
    one = np.zeros((3, 130), np.uint8)
    one[0, 0] = one[1, 129] = one[2, 64] = 1
    cases.append(("single", one, one.copy()))  # unions of 1 and 2
    for tag, g, p in cases:
        iou = rm.mask_iou(torch.tensor(g, dtype=torch.float32), torch.tensor(p, dtype=torch.float32))
        d[f"iou_{tag}_gt"], d[f"iou_{tag}_pred"] = np.packbits(g, axis=1), np.packbits(p, axis=1)
        d[f"iou_{tag}_n"] = np.int64(g.shape[1])
        d[f"iou_{tag}"] = iou.numpy()
        assert iou.dtype == torch.float32
    d["iou_tags"] = np.array([c[0] for c in cases])
    # the overlap expansion (val.py:206-209) on index maps: instances hidden completely, values above 255
    maps = []
    m = r.integers(0, 5, (9, 13)).astype(np.int32)
    m[m == 3] = 0  # instance 3 of 6 is painted over, 5 and 6 never appear
    maps.append(("small", m, 6))
    maps.append(("wide", r.integers(0, 301, (16, 24)).astype(np.int32), 300))
    for tag, m, nl in maps:
        gt = torch.tensor(m, dtype=torch.float32)[None]
        index = torch.arange(nl).view(nl, 1, 1) + 1
        ex = torch.where(gt.repeat(nl, 1, 1) == index, 1.0, 0.0)
        d[f"ex_{tag}_map"], d[f"ex_{tag}_nl"] = m, np.int64(nl)
        d[f"ex_{tag}"] = np.packbits(ex.numpy().astype(np.uint8).reshape(nl, -1), axis=1)
    d["ex_tags"] = np.array([c[0] for c in maps])
    np.savez_compressed(os.path.join(HERE, "segval_ops.npz"), **d)
    print("segval_ops", len(d), os.path.getsize(os.path.join(HERE, "segval_ops.npz")))


def _shift(m, dy, dx):
    out = np.zeros_like(m)
    h, w = m.shape
    out[max(dy, 0):h + min(dy, 0), max(dx, 0):w + min(dx, 0)] = m[max(-dy, 0):h + min(-dy, 0), max(-dx, 0):w + min(-dx, 0)]
    return out


def _erode(m):
    return m & _shift(m, 1, 0) & _shift(m, -1, 0) & _shift(m, 0, 1) & _shift(m, 0, -1)


def _overlap(ms):
    """data/utils.py polygons2masks_overlap on ready masks: largest first, later (smaller) instances paint over -> (index map, order)."""
    order = np.argsort(-ms.reshape(len(ms), -1).sum(1), kind="stable")
    out = np.zeros(ms.shape[1:], np.int32)
    for i, j in enumerate(order):
        out = np.clip(out + ms[j].astype(np.int32) * (i + 1), 0, i + 1)
    return out, order


def _validator(overlap):
    class V(RSV):
        def __init__(self):  # the validator's own set-up needs a dataset / cfg; only the metric plumbing is exercised
            pass
    v = V()
    v.device = torch.device("cpu")
    v.args = types.SimpleNamespace(single_cls=False, plots=False, save_json=False, save_txt=False, save_conf=False, overlap_mask=overlap)
    v.iouv = torch.linspace(0.5, 0.95, 10)
    v.niou, v.nc, v.seen, v.batch_i = 10, 80, 0, 0
    v.names = {i: str(i) for i in range(80)}
    v.metrics = rm.SegmentMetrics(names=v.names)
    v.stats = dict(tp_m=[], tp=[], conf=[], pred_cls=[], target_cls=[], target_img=[])
    v.confusion_matrix = None
    v.process = rops.process_mask
    v.plot_masks = []
    return v


def case_file():
    m = SegmentationModel(mgs.cfg("n"), ch=3, nc=80, verbose=False).eval()
    m.load_state_dict(seg_synth.state_dict(m.state_dict()))
    m.fuse(verbose=False)
    B, H, W = 6, 128, 160
    x = synth.synth_images(B, H, W, seed=9)
    y, (_, _, p) = m(x)
    preds = rops.non_max_suppression(y.clone(), 0.001, 0.7, multi_label=True, max_det=300, nc=80, max_time_img=1e6)
    mh, mw = p.shape[2:]
    pmasks = [rops.process_mask(p[i], q[:, 6:], q[:, :4].clone(), shape=(H, W)).numpy().astype(np.uint8) for i, q in enumerate(preds)]
    r = np.random.default_rng(7)
    ori = [(100, 160), (128, 128), (256, 320), (128, 160), (90, 120), (64, 80)]
    ratio_pad = []
    for h0, w0 in ori:  # LetterBox geometry (data/augment.py:1556-1591) as the dataset records it
        g = min(H / h0, W / w0)
        nw, nh = round(w0 * g), round(h0 * g)
        dw, dh = (W - nw) / 2, (H - nh) / 2
        ratio_pad.append(((g, g), (int(round(dw - 0.1)), int(round(dh - 0.1)))))
    cls, box, bidx, stack, maps = [], [], [], [], []
    for i, q in enumerate(preds):
        k = [3, 0, 5, 2, 4, 1][i]  # image 1 has no labels
        cand = [j for j in range(min(len(q), 60)) if pmasks[i][j].sum() >= 40]
        pick = [cand[t] for t in r.permutation(len(cand))[:k]]
        assert len(pick) == k, (i, len(cand))
        inst = []
        for j in pick:
            b = q[j, :4].numpy() + r.normal(0, 2.0, 4)
            c = float(q[j, 5]) if r.random() < 0.8 else float(r.integers(0, 80))
            g = pmasks[i][j]
            kind = r.integers(0, 5)  # the synthetic weights give speckled masks: a shift or an erosion leaves little overlap, so most
            if kind == 0:            # instances drop a share of the predicted pixels and gain a few instead (IoU spread over the thresholds)
                g = _erode(g)
            elif kind == 1:
                g = _shift(g, int(r.integers(-1, 2)), int(r.integers(-1, 2)))
            else:
                keep = r.random(g.shape) >= r.uniform(0.05, 0.45)
                g = ((g & keep) | (r.random(g.shape) < 0.01)).astype(np.uint8)
            if g.sum() == 0:
                g = pmasks[i][j].copy()
            inst.append((c, [(b[0] + b[2]) / 2 / W, (b[1] + b[3]) / 2 / H, abs(b[2] - b[0]) / W, abs(b[3] - b[1]) / H], g))
        if inst:
            ms = np.stack([t[2] for t in inst])
            imap, order = _overlap(ms)  # the dataset reorders the labels with the masks (data/dataset.py: sorted_idx)
            inst = [inst[j] for j in order]
        else:
            imap = np.zeros((mh, mw), np.int32)
        maps.append(imap)
        for c, bb, g in inst:
            cls.append([c]); bidx.append(i); box.append(bb); stack.append(g)
    stack = np.stack(stack)
    maps = np.stack(maps)
    base = dict(img=x, cls=torch.tensor(cls, dtype=torch.float32), bboxes=torch.tensor(np.array(box), dtype=torch.float32),
                batch_idx=torch.tensor(bidx, dtype=torch.float32), ori_shape=ori, ratio_pad=ratio_pad, im_file=[f"im{i}.jpg" for i in range(B)])
    d = dict(cls=base["cls"].numpy(), bboxes=base["bboxes"].numpy(), batch_idx=base["batch_idx"].numpy(), ori_shape=np.array(ori),
             ratio_gain=np.array([rp[0][0] for rp in ratio_pad]), ratio_padwh=np.array([rp[1] for rp in ratio_pad]),
             gt_stack=np.packbits(stack.reshape(len(stack), -1), axis=1), gt_index=maps.astype(np.uint8), mask_shape=np.array([mh, mw]),
             empty_pred_image=np.int64(3))
    assert maps.max() <= 255
    for i, q in enumerate(preds):
        d[f"pred{i}"] = q.numpy()
        d[f"pmask{i}"] = np.packbits(pmasks[i].reshape(len(q), -1), axis=1)
    # four runs of the reference's validator: both ground-truth layouts, with all predictions ("full", what a model run reproduces) and
    # with image 3's predictions removed ("nopred": labels without predictions, the npr == 0 bookkeeping)
    for overlap in (True, False):
        for variant in ("full", "nopred"):
            v = _validator(overlap)
            batch = dict(base)
            batch["masks"] = torch.tensor(maps if overlap else stack, dtype=torch.float32)
            ps = [q.clone() if not (variant == "nopred" and i == 3) else q[:0].clone() for i, q in enumerate(preds)]
            v.update_metrics((ps, p), batch)
            tag = f"{'overlap' if overlap else 'stack'}_{variant}"
            d[tag + "_tp"] = torch.cat(v.stats["tp"], 0).numpy()
            d[tag + "_tp_m"] = torch.cat(v.stats["tp_m"], 0).numpy()
            res = v.get_stats()
            d[tag + "_keys"], d[tag + "_values"] = np.array(list(res.keys())), np.array([float(t) for t in res.values()])
            d[tag + "_seen"], d[tag + "_nt_per_class"] = np.int64(v.seen), v.nt_per_class
            d[tag + "_ap_box"], d[tag + "_ap_mask"] = v.metrics.box.all_ap, v.metrics.seg.all_ap
            d[tag + "_ap_class_index"] = np.asarray(v.metrics.box.ap_class_index)
            print(tag, {k: round(float(t), 4) for k, t in res.items()}, "tp", int(d[tag + "_tp"].sum()), "tp_m", int(d[tag + "_tp_m"].sum()))
            assert d[tag + "_tp_m"].sum() > 0
    np.savez_compressed(os.path.join(HERE, "segval_case.npz"), **d)
    size = os.path.getsize(os.path.join(HERE, "segval_case.npz"))
    print("segval_case", len(d), [len(q) for q in preds], "labels", len(cls), size)
    assert size < 1 << 20


if __name__ == "__main__":
    ops_file()
    case_file()
