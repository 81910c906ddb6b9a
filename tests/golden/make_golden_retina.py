"""Golden vectors for masks at the original resolution, from the real reference imported through _ref_import: process_mask_native
(utils/ops.py:696-713, with scale_masks :716-737 and crop_mask :644-660), the retina branch of SegmentationPredictor.postprocess
(models/yolo/segment/predict.py:48-50: scale_boxes, then process_mask_native) and SegmentationValidator with
`process = ops.process_mask_native` (models/yolo/segment/val.py:52).  CPU fp32, synthetic inputs (tests/retina_synth.py, tests/seg_synth.py).

    python tests/golden/make_golden_retina.py

writes retina_ops.npz:
  * <tag>_bits / <tag>_shape for every op case of retina_synth.OP_CASES with N > 0, f32 and f16-representable inputs;
  * model_<h>x<w>_boxes / _bits / _shape: the yolo11n-seg 64x96 golden's own prototypes and NMS rows (yolo11n_seg_64x96.npz) as if the
    original image had been h x w, for retina_synth.MODEL_SHAPES;
  * val_<layout>_keys / _values / _tp_m: the reference validator's results on the inputs of segval_case.npz, `process` set to
    process_mask_native behind init_metrics' choice (a subclass), for both ground-truth layouts.
Mask bits are stored with np.packbits.  Runs only where the reference exists.
"""
import os

import make_golden_segval as mgv  # (sets up the reference import and the NMS stand-in through make_golden_seg)
import numpy as np
import torch

import retina_synth as rs
import seg_synth
import synthdata as synth
from ultralytics.nn.tasks import SegmentationModel
from ultralytics.utils import ops as rops

torch.set_grad_enabled(False)
HERE = mgv.HERE
mgs = mgv.mgs


def ops_cases(d):
    for case in rs.OP_CASES:
        if case[5] == 0:
            continue
        for half in (False, True):
            protos, coef, boxes, shape = rs.golden_case(case, half)
            bits = rops.process_mask_native(torch.tensor(protos), torch.tensor(coef), torch.tensor(boxes), shape)
            assert tuple(bits.shape) == (len(coef), *shape)
            tag = rs.golden_tag(case, half)
            d[tag + "_bits"], d[tag + "_shape"] = rs.pack(bits.to(torch.uint8).numpy())
            print(tag, tuple(bits.shape), int(bits.sum()))


def model_cases(d):
    g = np.load(os.path.join(HERE, "yolo11n_seg_64x96.npz"))
    det, p = torch.tensor(g["det0"]), torch.tensor(g["p"][0])
    for h, w in rs.MODEL_SHAPES:
        boxes = rops.scale_boxes((64, 96), det[:, :4].clone(), (h, w))  # segment/predict.py:49
        bits = rops.process_mask_native(p, det[:, 6:], boxes, (h, w))   # :50
        tag = f"model_{h}x{w}"
        d[tag + "_boxes"] = boxes.numpy()
        d[tag + "_bits"], d[tag + "_shape"] = rs.pack(bits.to(torch.uint8).numpy())
        print(tag, tuple(bits.shape), int(bits.sum()))
        assert bits.any()


def validator_cases(d):
    g = np.load(os.path.join(HERE, "segval_case.npz"))
    m = SegmentationModel(mgs.cfg("n"), ch=3, nc=80, verbose=False).eval()
    m.load_state_dict(seg_synth.state_dict(m.state_dict()))
    m.fuse(verbose=False)
    B = len(g["ori_shape"])
    x = synth.synth_images(B, 128, 160, seed=9)
    y, (_, _, p) = m(x)
    preds = rops.non_max_suppression(y.clone(), 0.001, 0.7, multi_label=True, max_det=300, nc=80, max_time_img=1e6)
    for i, q in enumerate(preds):  # the fixture's own rows
        np.testing.assert_array_equal(q.numpy(), g[f"pred{i}"])
    mh, mw = (int(v) for v in g["mask_shape"])
    stack = np.unpackbits(g["gt_stack"], axis=1)[:, :mh * mw].reshape(-1, mh, mw)
    base = dict(img=x, cls=torch.tensor(g["cls"]), bboxes=torch.tensor(g["bboxes"]), batch_idx=torch.tensor(g["batch_idx"]),
                ori_shape=[tuple(int(v) for v in s) for s in g["ori_shape"]],
                ratio_pad=[((float(a), float(a)), (int(q[0]), int(q[1]))) for a, q in zip(g["ratio_gain"], g["ratio_padwh"])], im_file=[f"im{i}.jpg" for i in range(B)])
    for overlap in (True, False):
        v = mgv._validator(overlap)
        v.process = rops.process_mask_native  # what init_metrics chooses for save_json / save_txt (val.py:52), set behind it
        batch = dict(base)
        batch["masks"] = torch.tensor(g["gt_index"].astype(np.float32) if overlap else stack.astype(np.float32))
        v.update_metrics(([q.clone() for q in preds], p), batch)
        tag = f"val_{'overlap' if overlap else 'stack'}"
        d[tag + "_tp_m"] = torch.cat(v.stats["tp_m"], 0).numpy()
        res = v.get_stats()
        d[tag + "_keys"], d[tag + "_values"] = np.array(list(res.keys())), np.array([float(t) for t in res.values()])
        print(tag, {k: round(float(t), 4) for k, t in res.items()}, "tp_m", int(d[tag + "_tp_m"].sum()))
        assert d[tag + "_tp_m"].sum() > 0


if __name__ == "__main__":
    d = {}
    ops_cases(d)
    model_cases(d)
    validator_cases(d)
    path = os.path.join(HERE, "retina_ops.npz")
    np.savez_compressed(path, **d)
    print("retina_ops", len(d), os.path.getsize(path))
    assert os.path.getsize(path) < 1 << 20
