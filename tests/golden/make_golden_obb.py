"""Golden vectors for the obb task: the OBB head (reference ultralytics/nn/modules/head.py:372-399, dist2rbox utils/tal.py:366-385), its
parse rule and OBBModel (nn/tasks.py:416-428), batch_probiou (utils/metrics.py:244-275), non_max_suppression(rotated=True) with
nms_rotated (utils/ops.py:146-164,230-297), regularize_rboxes (:775-790), xywhr2xyxyxyxy (:556-584), the OBB results container
(engine/results.py:1519) and the predict-time post-process (models/yolo/obb/predict.py:30-53), from the real reference imported through
_ref_import.  CPU fp32, synthetic weights and inputs (tests/obb_synth.py).

    python tests/golden/make_golden_obb.py

writes structure_obb.json, obb_ops.npz and yolo11n_obb_64x96.npz.  For every NMS case the float64 restatement (tests/fp64_obb_ref.py) gives
each column's margin |colmax - thr|; the cases marked exact get the first seed at which every margin exceeds 1e-3 (asserted), and the
reference's rows then equal the restatement's bit for bit (asserted too).  Runs only where the reference exists.
"""
import json
import os
import sys

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
import obb_synth  # noqa: E402
import synthdata as synth  # noqa: E402
from ultralytics.engine.results import OBB as RefOBB  # noqa: E402
from ultralytics.nn.modules.head import OBB  # noqa: E402
from ultralytics.nn.tasks import OBBModel, guess_model_task  # noqa: E402
from ultralytics.utils import ops as rops  # noqa: E402
from ultralytics.utils.metrics import batch_probiou  # noqa: E402

torch.set_grad_enabled(False)
CFG = os.path.join(ROOT, "edge-yolo_amd", "cfg", "models", "11")
MARGIN = 1e-3


def cfg(scale, name="yolo11-obb.yaml"):
    d = yaml.safe_load(open(os.path.join(CFG, name), encoding="utf-8"))
    d["scale"] = scale
    return d


def structure():
    out = {}
    for sc in obb_synth.SCALES:
        d = cfg(sc)
        assert guess_model_task(d) == "obb"
        m = OBBModel(d, ch=3, nc=80, verbose=False)
        assert guess_model_task(m) == "obb"
        out[obb_synth.NAME.format(sc)] = dict(params=sum(p.numel() for p in m.parameters()), save=list(m.save), stride=[float(s) for s in m.stride],
                                              layers=[dict(i=l.i, f=l.f, type=l.type, np=int(l.np)) for l in m.model],
                                              head=dict(ne=m.model[-1].ne), keys=list(m.state_dict()))
        print(sc, out[obb_synth.NAME.format(sc)]["params"])
    assert out[obb_synth.NAME.format("n")]["params"] == 2695747
    with open(os.path.join(HERE, "structure_obb.json"), "w") as f:
        f.write("{\n" + ",\n".join(json.dumps(k) + ": " + json.dumps(v, separators=(",", ":")) for k, v in out.items()) + "\n}\n")


def ref_decode(levels, strides, nc):
    """The reference's own eval-mode decode (OBB.forward's angle transform + Detect._inference + dist2rbox) on raw tower outputs."""
    import math
    m = OBB(nc=nc, ne=1, ch=tuple(16 for _ in levels)).eval()
    m.stride = torch.tensor(strides)
    bs = levels[0][0].shape[0]
    angle = torch.cat([a.view(bs, 1, -1) for _, _, a in levels], 2)
    m.angle = (angle.sigmoid() - 0.25) * math.pi
    y = m._inference([torch.cat((b, c), 1) for b, c, _ in levels])
    return torch.cat([y, m.angle], 1)


def ref_kept(pred_b, rows, nc):
    """anchor index of each reference row (rows are copies of the input's values)."""
    sc = pred_b[4:4 + nc]
    key = {}
    for a in range(pred_b.shape[1]):
        key[(pred_b[0, a].item(), pred_b[1, a].item(), pred_b[2, a].item(), pred_b[3, a].item(), sc[:, a].max().item(), pred_b[4 + nc, a].item())] = a
    return np.array([key[(r[0].item(), r[1].item(), r[2].item(), r[3].item(), r[4].item(), r[6].item())] for r in rows], np.int64)


def nms_cases(d):
    for case in obb_synth.NMS_CASES:
        tag, nc = case["tag"], case["nc"]
        kw = dict(conf_thres=case["conf"], iou_thres=case["iou"], classes=case["classes"], agnostic=case["agnostic"], nc=nc, max_nms=case["max_nms"],
                  max_time_img=1e6, rotated=True)
        for seed in range(200):
            pred = obb_synth.nms_case(case, seed)
            ora = f64.nms_rotated64(pred.numpy(), case["conf"], case["iou"], case["classes"], case["agnostic"], case["max_det"], case["max_nms"], obb_synth.MAX_WH)
            worst = min([float(o["margin"].min()) for o in ora if len(o["margin"])] or [1.0])
            if not case["exact"] or worst > MARGIN:
                break
        assert not case["exact"] or worst > MARGIN, tag
        rows = rops.non_max_suppression(pred.clone(), max_det=case["max_det"], **kw)
        full = rops.non_max_suppression(pred.clone(), max_det=case["A"], **kw)  # every kept column: the reference's own flags
        d[tag + "_seed"] = np.int64(seed)
        E = 0.0
        for b, o in enumerate(ora):
            d[f"{tag}_rows{b}"] = rows[b].numpy().astype(np.float32).reshape(-1, 7)
            d[f"{tag}_kept{b}"] = ref_kept(pred[b], full[b], nc)
            d[f"{tag}_margin{b}"] = o["margin"]
            if len(o["boxes"]):
                bt = torch.tensor(o["boxes"])
                err = np.abs(batch_probiou(bt, bt).numpy().astype(np.float64) - f64.probiou64(o["boxes"], o["boxes"]))
                E = max(E, float(np.triu(err, 1).max()))  # the pairs the columns see: i before j
            if case["exact"]:
                np.testing.assert_array_equal(rows[b].numpy().reshape(-1, 7), o["rows"], err_msg=tag)
        d[tag + "_E"] = np.float64(E)
        print(tag, "seed", seed, "counts", [len(o["order"]) for o in ora], "kept", [len(r) for r in rows], f"worst margin {worst:.2e} E {E:.2e}")


def ops_file():
    d = {}
    # the OBB head on small maps
    tag, kw, shapes = obb_synth.HEAD_CASE
    OBB.legacy = False
    m = OBB(**kw).eval()
    m.stride = torch.tensor([8.0, 16.0, 32.0])
    m.load_state_dict(obb_synth.state_dict(m.state_dict(), prefix=tag + "."))
    xs = [obb_synth.case_input(f"{tag}{i}", s) for i, s in enumerate(shapes)]
    y, (raw, angle) = m([x.clone() for x in xs])
    d[tag + "_y"], d[tag + "_angle"] = y, angle
    for i, r in enumerate(raw):
        d[f"{tag}_raw{i}"] = r
    d[tag + "_keys"] = np.array(list(m.state_dict()))
    # the decode alone
    for case in obb_synth.DECODE_CASES:
        levels = obb_synth.decode_case(*case)
        d[case[0] + "_y"] = ref_decode(levels, case[2], case[3])
        print(case[0], tuple(d[case[0] + "_y"].shape))
    # ProbIoU matrices
    for tag in obb_synth.PROBIOU_CASES:
        o1, o2 = obb_synth.probiou_case(tag)
        d[tag] = batch_probiou(torch.tensor(o1), torch.tensor(o2))
        E = float(np.abs(d[tag].numpy().astype(np.float64) - f64.probiou64(o1, o2)).max())
        print(tag, tuple(d[tag].shape), f"E {E:.2e}")
    nms_cases(d)
    rb = obb_synth.rbox_vectors()
    d["rboxes_regularized"] = rops.regularize_rboxes(rb)
    d["rboxes_corners"] = rops.xywhr2xyxyxyxy(rb)
    np.savez_compressed(os.path.join(HERE, "obb_ops.npz"), **{k: (v.numpy() if torch.is_tensor(v) else v) for k, v in d.items()})
    size = os.path.getsize(os.path.join(HERE, "obb_ops.npz"))
    print("obb_ops", len(d), size)
    assert size < 1 << 20


def model(d_cfg, tag, b, h, w, conf):
    m = OBBModel(d_cfg, ch=3, nc=80, verbose=False).eval()
    m.load_state_dict(obb_synth.state_dict(m.state_dict()))
    m.fuse(verbose=False)
    x = synth.synth_images(b, h, w)
    y, (raw, angle) = m(x)
    assert torch.isfinite(y).all() and y.shape[1] == 85, tag
    d = {"y": y, "angle": angle}
    for i, r in enumerate(raw):
        d[f"raw{i}"] = r
    # the predict-time post-process (obb/predict.py:30-53) on the reference's own output
    dets = rops.non_max_suppression(y.clone(), conf, 0.7, nc=80, max_det=300, max_time_img=1e6, rotated=True)
    for i, det in enumerate(dets):
        rboxes = rops.regularize_rboxes(torch.cat([det[:, :4], det[:, -1:]], dim=-1))
        rboxes[:, :4] = rops.scale_boxes((h, w), rboxes[:, :4], (h, w, 3), xywh=True)
        obb = torch.cat([rboxes, det[:, 4:6]], dim=-1)
        d[f"det{i}"], d[f"obb{i}"] = det, obb
        r = RefOBB(obb, (h, w))
        d[f"obb{i}_xyxyxyxy"], d[f"obb{i}_xyxyxyxyn"], d[f"obb{i}_xyxy"] = r.xyxyxyxy, r.xyxyxyxyn, r.xyxy
        assert torch.equal(r.xywhr, obb[:, :5]) and torch.equal(r.conf, obb[:, 5]) and torch.equal(r.cls, obb[:, 6])
        print(tag, "image", i, "kept", len(det))
    assert sum(len(t) for t in dets) >= 5, "lower conf"
    ora = f64.nms_rotated64(y.numpy(), conf, 0.7, None, False, 300, 30000, obb_synth.MAX_WH)
    for i, o in enumerate(ora):
        d[f"margin{i}"] = o["margin"]
        print(tag, "image", i, "candidates", len(o["order"]), f"worst margin {float(o['margin'].min()):.2e}")
        np.testing.assert_array_equal(dets[i].numpy(), o["rows"])
    d["conf"] = np.float64(conf)
    np.savez_compressed(os.path.join(HERE, f"{tag}.npz"), **{k: (v.numpy() if torch.is_tensor(v) else v) for k, v in d.items()})
    size = os.path.getsize(os.path.join(HERE, f"{tag}.npz"))
    print(tag, len(d), tuple(y.shape), size)
    assert size < 1 << 20


if __name__ == "__main__":
    structure()
    ops_file()
    model(cfg("n"), "yolo11n_obb_64x96", 1, 64, 96, conf=0.05)
