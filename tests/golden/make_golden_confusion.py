"""Golden results for the validation matching: the reference's ConfusionMatrix.process_batch matrices (ultralytics/utils/metrics.py:326-382),
its BaseValidator.match_predictions arrays at torch.linspace(0.5, 0.95, 10) (engine/validator.py:222-262), the same for oriented rows on
its batch_probiou, and ConfusionMatrix.process_cls_preds for a classify case, from the real reference imported through _ref_import.  CPU.

    python tests/golden/make_golden_confusion.py

writes confusion_cases.npz.  Inputs are tests/confusion_synth.py's; a draw that violates its tie-free conditions (`violations`: an IoU
within 2^-18 relative of a threshold, a confidence within 1e-6 of 0.25, an exact tie among a detection's or a label's candidates) is redrawn
with the next seed, and the file holds the seed used per case together with the recorded results, not the inputs.  It holds zero skipped
cases (asserted).  Runs only where the reference exists."""
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import _ref_import  # noqa: E402

_ref_import.setup()
import numpy as np  # noqa: E402
import torch  # noqa: E402

import confusion_synth as S  # noqa: E402
from ultralytics.engine.validator import BaseValidator  # noqa: E402
from ultralytics.utils import metrics as rm  # noqa: E402
from ultralytics.utils import ops as rops  # noqa: E402

IOUV = torch.linspace(0.5, 0.95, 10)
SELF = types.SimpleNamespace(iouv=IOUV)


def reference(det, gt, gt_cls, nc, iou):
    """-> (matrix int64 (nc+1, nc+1), tp bool (n, 10)) from the reference's own code."""
    cm = rm.ConfusionMatrix(nc, conf=0.001)  # (the validation default: becomes 0.25)
    assert cm.conf == S.CM_CONF and cm.iou_thres == S.CM_IOU
    d, g, c = torch.from_numpy(det), torch.from_numpy(gt), torch.from_numpy(gt_cls)
    cm.process_batch(d if len(d) else None, g, c)  # (no rows: the reference's validators pass None)
    tp = BaseValidator.match_predictions(SELF, d[:, 5], c, torch.from_numpy(iou)).numpy() if len(d) else np.zeros((0, 10), bool)
    assert (cm.matrix == np.round(cm.matrix)).all()
    return cm.matrix.astype(np.int64), tp


def main():
    out, skipped = {}, 0
    for i, spec in enumerate(S.SPECS):
        for seed in range(1000 * i, 1000 * i + 200):
            c = S.case(spec, seed)
            predn = c["det"].copy()
            if len(predn):
                predn[:, :4] = rops.scale_boxes(S.IMGSZ, torch.from_numpy(c["det"][:, :4].copy()), c["ori_shape"], ratio_pad=c["ratio_pad"]).numpy()
                assert np.array_equal(predn, S.scale_boxes(c["det"], c["ori_shape"], c["ratio_pad"])), "scale_boxes restatement"
            iou = rm.box_iou(torch.from_numpy(c["gt"]), torch.from_numpy(predn[:, :4])).numpy()
            assert np.array_equal(iou, S.box_iou(c["gt"], predn[:, :4]))
            if not S.violations(iou, predn, c["gt_cls"]):
                break
        else:
            skipped += 1
            continue
        m, tp = reference(predn, c["gt"], c["gt_cls"], c["nc"], iou)
        out[f"{c['name']}_seed"], out[f"{c['name']}_matrix"], out[f"{c['name']}_tp"] = np.int64(seed), m, tp
        print(c["name"], "seed", seed, "matrix sum", int(m.sum()), "diag", int(np.trace(m)), "tp50", int(tp[:, 0].sum()) if len(tp) else 0)
    for i, spec in enumerate(S.OBB_SPECS):
        for seed in range(100000 + 1000 * i, 100000 + 1000 * i + 200):
            c = S.obb_case(spec, seed)
            d, g = torch.from_numpy(c["det"]), torch.from_numpy(c["gt"])
            iou = rm.batch_probiou(g, torch.cat([d[:, :4], d[:, -1:]], -1)).numpy() if len(d) and len(g) else np.zeros((len(g), len(d)), np.float32)
            if not S.violations(iou, c["det"], c["gt_cls"]):
                break
        else:
            skipped += 1
            continue
        m, tp = reference(c["det"], c["gt"], c["gt_cls"], c["nc"], iou)
        out[f"{c['name']}_seed"], out[f"{c['name']}_matrix"], out[f"{c['name']}_tp"] = np.int64(seed), m, tp
        print(c["name"], "seed", seed, "matrix sum", int(m.sum()), "diag", int(np.trace(m)), "tp50", int(tp[:, 0].sum()) if len(tp) else 0)
    top, tgt, nc = S.cls_case(7)
    cm = rm.ConfusionMatrix(nc, task="classify")
    cm.process_cls_preds([torch.from_numpy(top[:100]), torch.from_numpy(top[100:])], [torch.from_numpy(tgt[:100]), torch.from_numpy(tgt[100:])])
    out["cls_seed"], out["cls_matrix"] = np.int64(7), cm.matrix.astype(np.int64)
    assert skipped == 0, f"{skipped} cases found no clean seed"
    out["skipped"] = np.int64(skipped)
    path = os.path.join(HERE, "confusion_cases.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
