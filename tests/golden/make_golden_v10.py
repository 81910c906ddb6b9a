"""Golden vectors for YOLOv10: SCDown, RepVGGDW, CIB, C2fCIB, PSA (reference ultralytics/nn/modules/block.py:879-997, 1057-1097, 1174-1206), v10Detect
(nn/modules/head.py:764-797), their parse rules (nn/tasks.py:1026-1027, 1059, 1092-1097) and the six model files, from the real reference imported
through _ref_import.  CPU fp32, synthetic weights and inputs (tests/v10_synth.py).  The reference builds the models from this repository's YAML
files read as data, and from its own files: the parameter counts of the two must agree for every scale.

    python tests/golden/make_golden_v10.py

writes structure_v10.json (the state_dict keys packed by v10_synth.pack_keys), v10_ops.npz, yolov10n_64x96.npz and yolov10x_64.npz.  Each model
file holds y (B, k, 6), the raw maps of both branches, and the rows non_max_suppression (its end-to-end branch: a filter) returns at the file's
conf.  conf is chosen so that, per image, the reference's scores of the rows at or above it -- and the one after them -- are more than 1e-3
apart and at least 5 rows pass: a test may then demand exact classes and exact row order on those rows.  Runs only where the reference exists.
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
import v10_synth as vs  # noqa: E402

from ultralytics.nn.modules import block as rblock  # noqa: E402
from ultralytics.nn.tasks import DetectionModel, guess_model_task  # noqa: E402
from ultralytics.utils import ops as rops  # noqa: E402

torch.set_grad_enabled(False)
CFG = os.path.join(ROOT, "edge-yolo_amd", "cfg", "models", "v10")
REF_CFG = os.path.join(_ref_import.REF, "ultralytics", "cfg", "models", "v10")


def build(name, own=True):
    d = yaml.safe_load(open(os.path.join(CFG if own else REF_CFG, name), encoding="utf-8"))
    assert guess_model_task(d) == "detect"
    return DetectionModel(d, ch=3, nc=80, verbose=False)


def structure():
    out = {}
    for name in vs.FILES:
        m = build(name)
        h = m.model[-1]
        out[name] = dict(params=sum(p.numel() for p in m.parameters()), save=list(m.save), stride=[float(s) for s in m.stride],
                         layers=[dict(i=l.i, f=l.f, type=l.type, np=int(l.np)) for l in m.model], legacy=bool(h.legacy), end2end=bool(h.end2end),
                         keys=vs.pack_keys(list(m.state_dict())))
        assert vs.unpack_keys(out[name]["keys"]) == list(m.state_dict())
        theirs = build(name, own=False)
        print(name, out[name]["params"], "reference file:", sum(p.numel() for p in theirs.parameters()))
        assert out[name]["params"] == sum(p.numel() for p in theirs.parameters()) and list(m.state_dict()) == list(theirs.state_dict())
        assert name not in vs.PARAMS or out[name]["params"] == vs.PARAMS[name]
    with open(os.path.join(HERE, "structure_v10.json"), "w") as f:  # one line per model: read by the tests only
        f.write("{\n" + ",\n".join(json.dumps(k) + ": " + json.dumps(v, separators=(",", ":")) for k, v in out.items()) + "\n}\n")


def ops_file():
    d = {}
    for tag, cls, args, kw, shape in vs.MODULE_CASES:
        m = getattr(rblock, cls)(*args, **kw).eval()
        for mod in m.modules():  # as in a model (initialize_weights)
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.eps = 1e-3
        m.load_state_dict(vs.state_dict(m.state_dict(), prefix=tag + "."))
        x = vs.case_input(tag, shape)
        d[tag + "_y"] = m(x)
        d[tag + "_keys"] = np.array(list(m.state_dict()))
        if cls == "RepVGGDW":
            m.fuse()
            d[tag + "_fused_keys"] = np.array(list(m.state_dict()))
            d[tag + "_fused_y"] = m.forward_fuse(x)
        print(tag, tuple(d[tag + "_y"].shape), float(d[tag + "_y"].abs().max()))
    np.savez_compressed(os.path.join(HERE, "v10_ops.npz"), **{k: (v.numpy() if torch.is_tensor(v) else v) for k, v in d.items()})
    size = os.path.getsize(os.path.join(HERE, "v10_ops.npz"))
    print("v10_ops", len(d), size)
    assert size < 1 << 20


def pick_conf(y):
    """The conf of a 0.001 grid at which every image has >= MIN_ROWS rows whose scores (and the next one's) are > ROW_GAP apart and the image
    with the fewest such rows has the most (the higher conf on a tie)."""
    best = None
    for conf in np.round(np.arange(0.99, 0.009, -0.001), 3):
        stats = [vs.separated_rows(y[i, :, 4].numpy(), float(conf)) for i in range(y.shape[0])]
        if all(n >= vs.MIN_ROWS and gap > vs.ROW_GAP for n, gap in stats) and (best is None or min(n for n, _ in stats) > min(n for n, _ in best[1])):
            best = (float(conf), stats)
    assert best is not None, "no conf of the grid separates the rows; change the gain or the seed"
    return best


def model(tag):
    name, shape = vs.MODEL_CASES[tag][:2]
    m = build(name).eval()
    m.load_state_dict(vs.model_weights(tag, m.state_dict()))
    m.fuse(verbose=False)
    assert all(list(mod.state_dict()) == ["conv.weight", "conv.bias"] for mod in m.modules() if isinstance(mod, rblock.RepVGGDW))
    x = vs.model_images(tag)
    y, aux = m(x)
    A = sum(r.shape[2] * r.shape[3] for r in aux["one2one"])
    assert torch.isfinite(y).all() and tuple(y.shape) == (shape[0], min(300, A), 6), tag
    d = {"y": y}
    for br in ("one2one", "one2many"):
        for i, r in enumerate(aux[br]):
            d[f"{br}{i}"] = r
    conf, stats = pick_conf(y)
    for i, (n, gap) in enumerate(stats):  # the row-order condition, asserted on the reference alone
        assert n >= vs.MIN_ROWS and gap > vs.ROW_GAP
        print(tag, "image", i, "rows >= conf:", n, "smallest gap:", gap, "best:", float(y[i, 0, 4]))
    dets = rops.non_max_suppression(y.clone(), conf, 0.7, nc=80, max_det=300, max_time_img=1e6)  # (B, k, 6): the end-to-end filter, utils/ops.py:224-228
    for i, det in enumerate(dets):
        assert len(det) == stats[i][0]
        det = det.clone()
        det[:, :4] = rops.scale_boxes(shape[1:], det[:, :4], (*shape[1:], 3))  # a tensor source, gain 1, no padding: a clip
        d[f"det{i}"] = det
    cl = sorted({int(c) for c in dets[0][:3, 5]})
    d["detc_classes"] = np.array(cl)
    for i, det in enumerate(rops.non_max_suppression(y.clone(), conf, 0.7, classes=cl, nc=80, max_det=3, max_time_img=1e6)):
        d[f"detc{i}"] = det
    d["conf"] = np.float64(conf)
    path = os.path.join(HERE, f"{tag}.npz")
    np.savez_compressed(path, **{k: (v.numpy() if torch.is_tensor(v) else v) for k, v in d.items()})
    print(tag, len(d), tuple(y.shape), "conf", conf, os.path.getsize(path))
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    structure()
    ops_file()
    for tag in vs.MODEL_CASES:
        model(tag)
