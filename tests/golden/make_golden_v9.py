"""Golden vectors for YOLOv9 (GELAN): RepConv (reference ultralytics/nn/modules/conv.py:196-297), RepNCSPELAN4, ELAN1, AConv, ADown, SPPELAN,
CBLinear and CBFuse (nn/modules/block.py:695-833), their parse rules (nn/tasks.py:1012-1016, 1100-1105) and the seven model files, from the
real reference imported through _ref_import.  CPU fp32, synthetic weights and inputs (tests/v9_synth.py).  The reference builds the models
from this repository's YAML files read as data.

    python tests/golden/make_golden_v9.py

writes structure_v9.json (the state_dict keys packed by v9_synth.pack_keys), v9_ops.npz, yolov9t_64x96.npz, yolov9e_64.npz,
yolov9c_seg_64x96.npz and yolov9m_64x96.npz.  torchvision.ops.nms is the documented stand-in of make_golden.py (oracle/nms.py).  Runs only
where the reference exists.
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
import yaml  # noqa: E402

import synthdata as synth  # noqa: E402
import v9_synth as vs  # noqa: E402
from oracle.nms import tv_nms  # noqa: E402

tv.ops.nms = lambda b, s, t: torch.as_tensor(tv_nms(b.numpy(), s.numpy(), t), dtype=torch.long)
from ultralytics.nn.modules import block as rblock, conv as rconv  # noqa: E402
from ultralytics.nn.tasks import DetectionModel, SegmentationModel, guess_model_task  # noqa: E402
from ultralytics.utils import ops as rops  # noqa: E402

torch.set_grad_enabled(False)
CFG = os.path.join(ROOT, "edge-yolo_amd", "cfg", "models", "v9")


def cfg(name):
    return yaml.safe_load(open(os.path.join(CFG, name), encoding="utf-8"))


def build(name):
    d = cfg(name)
    assert guess_model_task(d) == vs.TASK[name]
    return (SegmentationModel if vs.TASK[name] == "segment" else DetectionModel)(d, ch=3, nc=80, verbose=False)


def structure():
    out = {}
    for name in vs.FILES:
        m = build(name)
        out[name] = dict(params=sum(p.numel() for p in m.parameters()), save=list(m.save), stride=[float(s) for s in m.stride],
                         layers=[dict(i=l.i, f=l.f, type=l.type, np=int(l.np)) for l in m.model], legacy=bool(m.model[-1].legacy),
                         keys=vs.pack_keys(list(m.state_dict())))
        assert vs.unpack_keys(out[name]["keys"]) == list(m.state_dict())
        print(name, out[name]["params"])
        assert name not in vs.PARAMS or out[name]["params"] == vs.PARAMS[name]
    with open(os.path.join(HERE, "structure_v9.json"), "w") as f:  # one line per model: read by the tests only
        f.write("{\n" + ",\n".join(json.dumps(k) + ": " + json.dumps(v, separators=(",", ":")) for k, v in out.items()) + "\n}\n")


def ops_file():
    d = {}
    for tag, cls, args, kw, shape in vs.MODULE_CASES:
        m = (getattr(rconv, cls) if cls == "RepConv" else getattr(rblock, cls))(*args, **kw).eval()
        m.load_state_dict(vs.state_dict(m.state_dict(), prefix=tag + "."))
        x = vs.case_input(tag, shape)
        seen = {}
        if cls in ("AConv", "ADown"):  # what the pooling front end hands to the convs: the reference's own intermediate tensors
            m.cv1.register_forward_hook(lambda mod, inp, out: seen.__setitem__("a", inp[0].clone()))
            if cls == "ADown":
                m.cv2.register_forward_hook(lambda mod, inp, out: seen.__setitem__("m", inp[0].clone()))
        d[tag + "_y"] = m(x)
        d[tag + "_keys"] = np.array(list(m.state_dict()))
        for k, v in seen.items():
            d[f"{tag}_{k}"] = v
        if cls == "RepConv":
            m.fuse_convs()
            d[tag + "_fused_keys"] = np.array(list(m.state_dict()))
            d[tag + "_fused_y"] = m.forward_fuse(x)
        print(tag, tuple(d[tag + "_y"].shape))
    tag, args, shape = vs.CBLINEAR_CASE
    m = rblock.CBLinear(*args).eval()
    m.load_state_dict(vs.state_dict(m.state_dict(), prefix=tag + "."))
    for i, y in enumerate(m(vs.case_input(tag, shape))):
        d[f"{tag}_y{i}"] = y.contiguous()
    d[tag + "_keys"] = np.array(list(m.state_dict()))
    tag, idx, _, _ = vs.CBFUSE_CASE
    d[tag + "_y"] = rblock.CBFuse(idx)(vs.cbfuse_inputs())
    print(tag, tuple(d[tag + "_y"].shape))
    np.savez_compressed(os.path.join(HERE, "v9_ops.npz"), **{k: (v.numpy() if torch.is_tensor(v) else v) for k, v in d.items()})
    size = os.path.getsize(os.path.join(HERE, "v9_ops.npz"))
    print("v9_ops", len(d), size)
    assert size < 1 << 20


def model(tag, conf):
    name, shape, gain = vs.MODEL_CASES[tag]
    seg = vs.TASK[name] == "segment"
    m = build(name).eval()
    m.load_state_dict(vs.state_dict(m.state_dict(), gain=gain))
    m.fuse(verbose=False)
    x = synth.synth_images(*shape)
    y, rest = m(x)
    raw, mc, p = rest if seg else (rest, None, None)
    assert torch.isfinite(y).all(), tag
    d = {"y": y}
    for i, r in enumerate(raw):
        d[f"raw{i}"] = r
    if seg:
        d["mc"], d["p"] = mc, p
    dets = rops.non_max_suppression(y.clone(), conf, 0.7, nc=80, max_det=300, max_time_img=1e6)  # detect/predict.py:25-33
    for i, det in enumerate(dets):
        det = det.clone()
        if seg:
            d[f"masks{i}"] = rops.process_mask(p[i], det[:, 6:], det[:, :4].clone(), shape[1:], upsample=True).to(torch.uint8)
        det[:, :4] = rops.scale_boxes(shape[1:], det[:, :4], (*shape[1:], 3))  # a tensor source, gain 1, no padding: a clip
        d[f"det{i}"] = det
        print(tag, "image", i, "kept", len(det), "max score", float(y[i, 4:84].max()))
    assert sum(len(t) for t in dets) >= 5, "lower conf"
    d["conf"] = np.float64(conf)
    np.savez_compressed(os.path.join(HERE, f"{tag}.npz"), **{k: (v.numpy() if torch.is_tensor(v) else v) for k, v in d.items()})
    size = os.path.getsize(os.path.join(HERE, f"{tag}.npz"))
    print(tag, len(d), tuple(y.shape), size)
    assert size < 1 << 20


if __name__ == "__main__":
    structure()
    ops_file()
    for tag, conf in (("yolov9t_64x96", 0.05), ("yolov9e_64", 0.05), ("yolov9c_seg_64x96", 0.05), ("yolov9m_64x96", 0.05)):
        model(tag, conf)
