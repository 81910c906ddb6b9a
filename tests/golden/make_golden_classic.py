"""Golden vectors for YOLOv3, YOLOv5 and YOLOv6: SPP (reference ultralytics/nn/modules/block.py:186-201), a repeated Bottleneck row, the torch
rows nn.MaxPool2d / nn.ZeroPad2d / nn.ConvTranspose2d, the two image stems that are not 3x3 stride 2, and the six model files, from the real
reference imported through _ref_import.  CPU fp32, synthetic weights and inputs (tests/classic_synth.py).  The reference builds the models from
this repository's YAML files read as data, and from its own files: parameter counts and state_dict keys of the two must agree, and the eight
counts of classic_synth.PARAMS are asserted.

    python tests/golden/make_golden_classic.py

writes structure_classic.json (the state_dict keys packed by v9_synth.pack_keys), classic_ops.npz and one .npz per model case of classic_synth:
the decoded prediction y, the raw level maps and the rows the reference's non_max_suppression keeps at the file's conf.  conf is chosen so that,
per image, at least 5 rows are kept, the kept rows' scores are more than 1e-3 apart and no candidate's best score lies within 1e-3 of conf: a
test may then demand exact classes and exact row order.  torchvision.ops.nms is the documented stand-in of make_golden.py (oracle/nms.py).
The reference's parse_model leaves a YAML's `activation:` in Conv.default_act for the rest of the process; this script puts SiLU back before
every build.  Runs only where the reference exists.
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

import classic_synth as cs  # noqa: E402
from oracle.nms import tv_nms  # noqa: E402

tv.ops.nms = lambda b, s, t: torch.as_tensor(tv_nms(b.numpy(), s.numpy(), t), dtype=torch.long)
from ultralytics.nn.modules import block as rblock, conv as rconv  # noqa: E402
from ultralytics.nn import tasks as rtasks  # noqa: E402
from ultralytics.nn.tasks import DetectionModel, guess_model_task  # noqa: E402
from ultralytics.utils import ops as rops  # noqa: E402

torch.set_grad_enabled(False)
CFG = os.path.join(ROOT, "edge-yolo_amd", "cfg", "models")
REF_CFG = os.path.join(_ref_import.REF, "ultralytics", "cfg", "models")
BY_NAME = {n: (f, s) for n, f, s in cs.NAMES}


def load_yaml(name, own=True):
    f, scale = BY_NAME[name]
    d = yaml.safe_load(open(os.path.join(CFG if own else REF_CFG, f), encoding="utf-8"))
    d["scale"] = scale
    return d


def build(cfg, own=True):
    d = load_yaml(cfg, own) if isinstance(cfg, str) else cfg
    assert guess_model_task(d) == "detect"
    rconv.Conv.default_act = torch.nn.SiLU()  # (see the module docstring)
    m = DetectionModel(d, ch=3, nc=80, verbose=False)
    rconv.Conv.default_act = torch.nn.SiLU()
    return m


def structure():
    out = {}
    for name in cs.STRUCT_FILES:
        m = build(name)
        out[name] = dict(params=sum(p.numel() for p in m.parameters()), save=list(m.save), stride=[float(s) for s in m.stride],
                         layers=[dict(i=l.i, f=l.f, type=l.type, np=int(l.np)) for l in m.model], legacy=bool(m.model[-1].legacy),
                         keys=cs.pack_keys(list(m.state_dict())))
        assert cs.unpack_keys(out[name]["keys"]) == list(m.state_dict())
        theirs = build(name, own=False)
        print(name, out[name]["params"], "reference file:", sum(p.numel() for p in theirs.parameters()), out[name]["stride"])
        assert out[name]["params"] == sum(p.numel() for p in theirs.parameters()) == cs.PARAMS[name] and list(m.state_dict()) == list(theirs.state_dict())
        assert [(l.i, l.f, l.type, int(l.np)) for l in m.model] == [(l.i, l.f, l.type, int(l.np)) for l in theirs.model]
        assert out[name]["stride"] == cs.STRIDES[name] and out[name]["legacy"] is True
        del m, theirs
    path = os.path.join(HERE, "structure_classic.json")
    with open(path, "w") as f:  # one line per model: read by the tests only
        f.write("{\n" + ",\n".join(json.dumps(k) + ": " + json.dumps(v, separators=(",", ":")) for k, v in out.items()) + "\n}\n")
    print("structure_classic.json", os.path.getsize(path))
    assert os.path.getsize(path) < 1 << 20


REF_NS = {"Conv": rconv.Conv, "SPP": rblock.SPP, "MaxPool2d": torch.nn.MaxPool2d, "ZeroPad2d": torch.nn.ZeroPad2d, "ConvTranspose2d": torch.nn.ConvTranspose2d,
          "parse": lambda d, ch: rtasks.parse_model(d, ch, verbose=False)}


def ops_file():
    d = {}
    rconv.Conv.default_act = torch.nn.SiLU()
    for tag in cs.OPS_CASES:
        m = cs.prepare(cs.make_module(tag, REF_NS), tag)
        x = cs.ops_input(tag)
        d[tag + "_y"] = m(x)
        d[tag + "_keys"] = np.array(list(m.state_dict()), dtype=str)
        print(tag, tuple(d[tag + "_y"].shape), float(d[tag + "_y"].abs().max()), len(m.state_dict()))
    assert float(d["zeropad_maxpool_y"][:, :, -1].abs().max()) == 0.0 and float(d["zeropad_maxpool_y"][:, :, :, -1].abs().max()) == 0.0  # the zero padding won
    assert float(d["zeropad_maxpool_y"][:, :, :-1, :-1].max()) < 0.0
    np.savez_compressed(os.path.join(HERE, "classic_ops.npz"), **{k: (v.numpy() if torch.is_tensor(v) else v) for k, v in d.items()})
    size = os.path.getsize(os.path.join(HERE, "classic_ops.npz"))
    print("classic_ops", len(d), size)
    assert size < 1 << 20


def nms_rows(y, conf):
    return rops.non_max_suppression(y.clone(), conf, 0.7, nc=80, max_det=300, max_time_img=1e6)  # detect/predict.py:25-33


def pick_conf(y):
    """The highest conf of a 0.001 grid at which every image keeps >= MIN_ROWS rows that meet the row condition of classic_synth."""
    for conf in np.round(np.arange(0.999, 0.009, -0.001), 3):
        best = y[:, 4:].max(1).values
        if int((best > conf).sum(1).min()) < cs.MIN_ROWS:
            continue
        dets = nms_rows(y, float(conf))
        stats = [cs.kept_rows_separated(y[i].numpy(), dets[i].numpy(), float(conf)) for i in range(y.shape[0])]
        if all(n >= cs.MIN_ROWS and gap > cs.ROW_GAP and margin > cs.ROW_GAP for n, gap, margin in stats):
            return float(conf), dets, stats
    raise AssertionError("no conf of the grid separates the rows; change the gain or the seed")


def model(tag):
    shape = cs.MODEL_CASES[tag][1]
    m = build(cs.model_cfg(tag, load_yaml)).eval()
    assert len(m.stride) == cs.NL[tag]
    m.load_state_dict(cs.model_weights(tag, m.state_dict()))
    m.fuse(verbose=False)
    x = cs.model_images(tag)
    y, raw = m(x)
    assert torch.isfinite(y).all() and len(raw) == len(m.stride), tag
    d = {"y": y}
    for i, r in enumerate(raw):
        d[f"raw{i}"] = r
    conf, dets, stats = pick_conf(y)
    for i, det in enumerate(dets):
        n, gap, margin = stats[i]
        assert n == len(det) >= cs.MIN_ROWS and gap > cs.ROW_GAP and margin > cs.ROW_GAP  # the row condition, asserted on the reference alone
        print(tag, "image", i, "kept", n, "smallest gap", gap, "margin to conf", margin, "max score", float(y[i, 4:].max()))
        det = det.clone()
        det[:, :4] = rops.scale_boxes(shape[1:], det[:, :4], (*shape[1:], 3))  # a tensor source, gain 1, no padding: a clip
        d[f"det{i}"] = det
    d["conf"] = np.float64(conf)
    path = os.path.join(HERE, f"{tag}.npz")
    np.savez_compressed(path, **{k: (v.numpy() if torch.is_tensor(v) else v) for k, v in d.items()})
    print(tag, len(d), tuple(y.shape), [tuple(r.shape) for r in raw], "conf", conf, os.path.getsize(path))
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    which = sys.argv[1:] or ["structure", "ops", "models"]
    if "structure" in which:
        structure()
    if "ops" in which:
        ops_file()
    if "models" in which:
        for tag in cs.MODEL_CASES:
            if len(which) > 1 and "models" in which and any(w in cs.MODEL_CASES for w in which) and tag not in which:
                continue
            model(tag)
