"""Golden vectors for YOLOv8 and YOLOv8-ghost: GhostConv (reference ultralytics/nn/modules/conv.py:180-193), C2, C3Ghost and GhostBottleneck
(nn/modules/block.py:339-354, 436-464), their parse rules and the six model files at all five scales, from the real reference imported through
_ref_import.  CPU fp32, synthetic weights and inputs (tests/ghost_synth.py).  The reference builds the models from this repository's YAML files
read as data, and from its own files: parameter counts and state_dict keys of the two must agree for every file and scale.

    python tests/golden/make_golden_ghost.py

writes structure_ghost.json (the state_dict keys packed by v9_synth.pack_keys), ghost_ops.npz and one .npz per model case of ghost_synth: the
decoded prediction y, the raw level maps and the rows the reference's non_max_suppression keeps at the file's conf.  conf is chosen so that,
per image, at least 5 rows are kept, the kept rows' scores are more than 1e-3 apart and no candidate's best score lies within 1e-3 of conf: a
test may then demand exact classes and exact row order.  torchvision.ops.nms is the documented stand-in of make_golden.py (oracle/nms.py).
Runs only where the reference exists.
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

import ghost_synth as gs  # noqa: E402
from oracle.nms import tv_nms  # noqa: E402

tv.ops.nms = lambda b, s, t: torch.as_tensor(tv_nms(b.numpy(), s.numpy(), t), dtype=torch.long)
from ultralytics.nn.modules import block as rblock, conv as rconv  # noqa: E402
from ultralytics.nn.tasks import DetectionModel, guess_model_scale, guess_model_task  # noqa: E402
from ultralytics.utils import ops as rops  # noqa: E402

torch.set_grad_enabled(False)
CFG = os.path.join(ROOT, "edge-yolo_amd", "cfg", "models", "v8")
REF_CFG = os.path.join(_ref_import.REF, "ultralytics", "cfg", "models", "v8")


def build(name, own=True):
    scale = guess_model_scale(name)
    d = yaml.safe_load(open(os.path.join(CFG if own else REF_CFG, name.replace("yolov8" + scale, "yolov8", 1)), encoding="utf-8"))
    d["scale"] = scale
    assert guess_model_task(d) == "detect"
    return DetectionModel(d, ch=3, nc=80, verbose=False)


def structure():
    out = {}
    for name in gs.FILES:
        m = build(name)
        out[name] = dict(params=sum(p.numel() for p in m.parameters()), save=list(m.save), stride=[float(s) for s in m.stride],
                         layers=[dict(i=l.i, f=l.f, type=l.type, np=int(l.np)) for l in m.model], legacy=bool(m.model[-1].legacy),
                         keys=gs.pack_keys(list(m.state_dict())))
        assert gs.unpack_keys(out[name]["keys"]) == list(m.state_dict())
        theirs = build(name, own=False)
        print(name, out[name]["params"], "reference file:", sum(p.numel() for p in theirs.parameters()), out[name]["stride"])
        assert out[name]["params"] == sum(p.numel() for p in theirs.parameters()) and list(m.state_dict()) == list(theirs.state_dict())
        assert name not in gs.PARAMS or out[name]["params"] == gs.PARAMS[name]
        if name in gs.GHOST_FILES and name[6] in gs.HIDDEN:  # the hidden widths of the 1x1 GhostConvs (the P6 files have more)
            hid = sorted({mod.cv1.conv.out_channels for mod in m.modules() if isinstance(mod, rconv.GhostConv) and mod.cv1.conv.kernel_size == (1, 1)})
            assert all(mod.cv1.conv.in_channels % 8 == 0 for mod in m.modules() if isinstance(mod, rconv.GhostConv) and mod.cv1.conv.kernel_size == (1, 1))
            assert hid == (gs.HIDDEN[name[6]] if "-p6" not in name or name[6] != "n" else gs.HIDDEN_P6_N) and any(h % 8 == 4 for h in hid), (name, hid)
            print("   hidden widths", hid)
    path = os.path.join(HERE, "structure_ghost.json")
    with open(path, "w") as f:  # one line per model: read by the tests only
        f.write("{\n" + ",\n".join(json.dumps(k) + ": " + json.dumps(v, separators=(",", ":")) for k, v in out.items()) + "\n}\n")
    print("structure_ghost.json", os.path.getsize(path))
    assert os.path.getsize(path) < 1 << 20


def ops_file():
    d = {}
    for tag, cls, args, kw, shape in gs.MODULE_CASES:
        m = (getattr(rconv, cls) if cls == "GhostConv" else getattr(rblock, cls))(*args, **kw).eval()
        for mod in m.modules():  # as in a model (initialize_weights)
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.eps = 1e-3
        m.load_state_dict(gs.state_dict(m.state_dict(), prefix=tag + "."))
        d[tag + "_y"] = m(gs.case_input(tag, shape))
        d[tag + "_keys"] = np.array(list(m.state_dict()))
        print(tag, tuple(d[tag + "_y"].shape), float(d[tag + "_y"].abs().max()))
    np.savez_compressed(os.path.join(HERE, "ghost_ops.npz"), **{k: (v.numpy() if torch.is_tensor(v) else v) for k, v in d.items()})
    size = os.path.getsize(os.path.join(HERE, "ghost_ops.npz"))
    print("ghost_ops", len(d), size)
    assert size < 1 << 20


def nms_rows(y, conf):
    return rops.non_max_suppression(y.clone(), conf, 0.7, nc=80, max_det=300, max_time_img=1e6)  # detect/predict.py:25-33


def pick_conf(y):
    """The highest conf of a 0.001 grid at which every image keeps >= MIN_ROWS rows that meet the row condition of ghost_synth."""
    for conf in np.round(np.arange(0.999, 0.009, -0.001), 3):
        best = y[:, 4:].max(1).values
        if int((best > conf).sum(1).min()) < gs.MIN_ROWS:
            continue
        dets = nms_rows(y, float(conf))
        stats = [gs.kept_rows_separated(y[i].numpy(), dets[i].numpy(), float(conf)) for i in range(y.shape[0])]
        if all(n >= gs.MIN_ROWS and gap > gs.ROW_GAP and margin > gs.ROW_GAP for n, gap, margin in stats):
            return float(conf), dets, stats
    raise AssertionError("no conf of the grid separates the rows; change the gain or the seed")


def model(tag):
    name, shape = gs.MODEL_CASES[tag][:2]
    m = build(name).eval()
    m.load_state_dict(gs.model_weights(tag, m.state_dict()))
    m.fuse(verbose=False)
    x = gs.model_images(tag)
    y, raw = m(x)
    assert torch.isfinite(y).all() and len(raw) == len(m.stride), tag
    d = {"y": y}
    for i, r in enumerate(raw):
        d[f"raw{i}"] = r
    conf, dets, stats = pick_conf(y)
    for i, det in enumerate(dets):
        n, gap, margin = stats[i]
        assert n == len(det) >= gs.MIN_ROWS and gap > gs.ROW_GAP and margin > gs.ROW_GAP  # the row condition, asserted on the reference alone
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
        for tag in gs.MODEL_CASES:
            model(tag)
