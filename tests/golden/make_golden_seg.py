"""Golden vectors for the segment task: Proto (reference ultralytics/nn/modules/block.py:112-129), Segment (nn/modules/head.py:347-369),
the Segment parse rule (nn/tasks.py:1094-1095), process_mask / crop_mask (utils/ops.py:644-693) and non_max_suppression with mask
coefficients (:167-316), from the real reference imported through _ref_import.  CPU fp32, synthetic weights (tests/seg_synth.py) and
inputs.  The reference builds yolo11{n,s,m,l,x}-seg.yaml from this repository's YAML read as data, and the EdgeLine graph
(yolo11-test.yaml) with its last row swapped to Segment from the same dict the tests build.

    python tests/golden/make_golden_seg.py

writes structure_seg.json, seg_ops.npz, yolo11n_seg_64x96.npz and edgeline_n_seg_64.npz (layers 0-22 of the last repeat
edgeline_n_64.npz bit for bit -- checked here -- and are read from that file by the tests).  torchvision.ops.nms is the documented
stand-in of make_golden.py (oracle/nms.py).  Runs only where the reference exists; the GPU box never runs this.
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

tv = _ref_import.setup()
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
import yaml  # noqa: E402

import seg_synth  # noqa: E402
import synthdata as synth  # noqa: E402
from oracle.nms import tv_nms  # noqa: E402

tv.ops.nms = lambda b, s, t: torch.as_tensor(tv_nms(b.numpy(), s.numpy(), t), dtype=torch.long)
from ultralytics.nn.tasks import SegmentationModel, guess_model_task  # noqa: E402
from ultralytics.nn.modules.block import Proto  # noqa: E402
from ultralytics.nn.modules.head import Segment  # noqa: E402
from ultralytics.utils import ops as rops  # noqa: E402

torch.set_grad_enabled(False)
CFG = os.path.join(ROOT, "edge-yolo_amd", "cfg", "models", "11")


def cfg(scale, name="yolo11-seg.yaml"):
    d = yaml.safe_load(open(os.path.join(CFG, name), encoding="utf-8"))
    d["scale"] = scale
    return d


def structure():
    out = {}
    for sc in seg_synth.SCALES:
        d = cfg(sc)
        assert guess_model_task(d) == "segment"
        m = SegmentationModel(d, ch=3, nc=80, verbose=False)
        out[seg_synth.NAME.format(sc)] = dict(params=sum(p.numel() for p in m.parameters()), save=list(m.save), stride=[float(s) for s in m.stride],
                                              layers=[dict(i=l.i, f=l.f, type=l.type, np=int(l.np)) for l in m.model],
                                              head=dict(nm=m.model[-1].nm, npr=m.model[-1].npr), keys=list(m.state_dict()))
        print(sc, out[seg_synth.NAME.format(sc)]["params"])
    assert out[seg_synth.NAME.format("n")]["params"] == 2876848
    with open(os.path.join(HERE, "structure_seg.json"), "w") as f:  # one line per model: read by the tests only
        f.write("{\n" + ",\n".join(json.dumps(k) + ": " + json.dumps(v, separators=(",", ":")) for k, v in out.items()) + "\n}\n")


def pre_threshold(protos, masks_in, bboxes, shape, upsample):
    """process_mask (ops.py:678-692) up to, not including, the compare: the reference's own fp32 values."""
    c, mh, mw = protos.shape
    ih, iw = shape
    masks = (masks_in @ protos.float().view(c, -1)).view(-1, mh, mw)
    b = bboxes.clone()
    b[:, 0] *= mw / iw
    b[:, 2] *= mw / iw
    b[:, 3] *= mh / ih
    b[:, 1] *= mh / ih
    masks = rops.crop_mask(masks, b)
    if upsample:
        masks = F.interpolate(masks[None], shape, mode="bilinear", align_corners=False)[0]
    return masks


def ops_file():
    d = {}
    for tag, args, shape in seg_synth.PROTO_CASES:
        m = Proto(*args).eval()
        m.load_state_dict(seg_synth.state_dict(m.state_dict(), prefix=tag + "."))
        x = seg_synth.case_input(tag, shape)
        d[tag + "_x"], d[tag] = x, m(x)
        d[tag + "_up"] = m.upsample(m.cv1(x))
        d[tag + "_keys"] = np.array(list(m.state_dict()))
    tag, kw, shapes = seg_synth.SEGMENT_CASE
    Segment.legacy = False
    m = Segment(**kw).eval()
    m.stride = torch.tensor([8.0, 16.0, 32.0])
    m.load_state_dict(seg_synth.state_dict(m.state_dict(), prefix=tag + "."))
    xs = [seg_synth.case_input(f"{tag}{i}", s) for i, s in enumerate(shapes)]
    y, (raw, mc, p) = m([x.clone() for x in xs])
    d[tag + "_y"], d[tag + "_mc"], d[tag + "_p"] = y, mc, p
    for i, r in enumerate(raw):
        d[f"{tag}_raw{i}"] = r
    d[tag + "_keys"] = np.array(list(m.state_dict()))
    for case in seg_synth.PM_GOLDEN:
        tag, s = case[0], case[1]
        protos, coef, boxes, shape = (torch.tensor(a) if isinstance(a, np.ndarray) else a for a in seg_synth.pm_golden_case(*case))
        bits = rops.process_mask(protos, coef, boxes.clone(), shape, upsample=True)
        d[tag + "_bits"] = bits.to(torch.uint8)
        d[tag + "_pre"] = pre_threshold(protos, coef, boxes, shape, True)
        assert torch.equal(d[tag + "_pre"] > 0, bits.bool()), tag
        if s > 1:  # upsample=False: the low-resolution form
            d[tag + "_bits_lowres"] = rops.process_mask(protos, coef, boxes.clone(), shape, upsample=False).to(torch.uint8)
        print(tag, tuple(bits.shape), int(bits.sum()))
    pred = seg_synth.nms_pred()
    for conf, iou, key in ((0.25, 0.7, "nms_a"), (0.5, 0.45, "nms_b")):
        rows = rops.non_max_suppression(pred.clone(), conf, iou, nc=4, max_det=50, max_time_img=1e6)[0]
        assert rows.shape[1] == 6 + 32 and len(rows) >= 5
        d[key] = rows
        print(key, tuple(rows.shape))
    np.savez_compressed(os.path.join(HERE, "seg_ops.npz"), **{k: (v.numpy() if torch.is_tensor(v) else v) for k, v in d.items()})
    print("seg_ops", len(d), os.path.getsize(os.path.join(HERE, "seg_ops.npz")))


def model(d_cfg, tag, b, h, w, conf, base=None):
    m = SegmentationModel(d_cfg, ch=3, nc=80, verbose=False).eval()
    m.load_state_dict(seg_synth.state_dict(m.state_dict()))
    m.fuse(verbose=False)
    d = {}
    hs = [l.register_forward_hook(lambda mod, inp, out, i=l.i: d.__setitem__(f"layer{i}", out.clone()) if torch.is_tensor(out) else None) for l in m.model]
    x = synth.synth_images(b, h, w)
    y, (raw, mc, p) = m(x)
    for hk in hs:
        hk.remove()
    assert torch.isfinite(y).all() and tuple(p.shape[2:]) == (h // 4, w // 4), tag
    if base:
        g = np.load(os.path.join(HERE, base + ".npz"))
        same = [k for k in d if k in g and np.array_equal(g[k], d[k].numpy())]
        assert {f"layer{i}" for i in range(len(m.model) - 1) if f"layer{i}" in d} == set(same), same
        for k in same:
            del d[k]
        print(tag, "layers shared with", base, ":", len(same))
    d["y"], d["mc"], d["p"] = y, mc, p
    for i, r in enumerate(raw):
        d[f"raw{i}"] = r
    # the predict-time post-process (segment/predict.py:27-57) on the reference's own output
    dets = rops.non_max_suppression(y.clone(), conf, 0.7, nc=80, max_det=300, max_time_img=1e6)
    for i, det in enumerate(dets):
        d[f"det{i}"] = det
        d[f"masks{i}"] = rops.process_mask(p[i], det[:, 6:], det[:, :4].clone(), (h, w), upsample=True).to(torch.uint8)
        assert torch.equal(pre_threshold(p[i], det[:, 6:], det[:, :4], (h, w), True) > 0, d[f"masks{i}"].bool())
        print(tag, "image", i, "kept", len(det), "mask pixels", int(d[f"masks{i}"].sum()))
    assert sum(len(t) for t in dets) >= 5, "lower conf"
    d["conf"] = np.float64(conf)
    np.savez_compressed(os.path.join(HERE, f"{tag}.npz"), **{k: (v.numpy() if torch.is_tensor(v) else v) for k, v in d.items()})
    size = os.path.getsize(os.path.join(HERE, f"{tag}.npz"))
    print(tag, len(d), tuple(y.shape), tuple(mc.shape), tuple(p.shape), size)
    assert size < 1 << 20


if __name__ == "__main__":
    structure()
    ops_file()
    model(cfg("n"), "yolo11n_seg_64x96", 1, 64, 96, conf=0.05)
    model(seg_synth.edgeline_seg_cfg(cfg("n", "yolo11-test.yaml")), "edgeline_n_seg_64", 2, 64, 64, conf=0.05, base="edgeline_n_64")
