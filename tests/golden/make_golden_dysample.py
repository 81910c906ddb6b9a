"""Golden vectors for DySample (reference ultralytics/nn/modules/dysample.py:20-93, parse rule nn/tasks.py:1127-1130) and for
yolov13*-DySample.yaml, this repository's yolov13.yaml with its three nn.Upsample rows replaced by DySample.  The reference has no such
file; it builds the graph from the same dict (this repository's YAML, read as data) plus the `scale` key.  CPU fp32, synthetic weights
and inputs (synthdata.py; tests/dysample_synth.py keeps every module's own init_pos), the real reference imported through _ref_import:

    python tests/golden/make_golden_dysample.py

writes tests/golden/dysample_ops.npz (module level), yolov13n_dysample_64x96.npz (per-layer outputs + y; the layers that repeat
yolov13n_64x96.npz bit for bit are left out), yolov13n_dysample_96x160.npz, yolov13l_dysample_64.npz (likewise against yolov13l_64.npz)
and structure_dysample.json.  Runs only where the reference exists; the GPU box never runs this.
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

import dysample_synth  # noqa: E402
import synthdata as synth  # noqa: E402
from ultralytics.nn.tasks import DetectionModel  # noqa: E402
from ultralytics.nn.modules.dysample import DySample  # noqa: E402

torch.set_grad_enabled(False)
GAIN = dysample_synth.GAIN
NAME = dysample_synth.NAME
YAML = os.path.join(ROOT, "edge-yolo_amd", "cfg", "models", "13", "yolov13-DySample.yaml")


def modules():
    d = {}
    for tag, args, shape in dysample_synth.CASES:
        m = dysample_synth.fill(DySample(*args), tag)
        x = dysample_synth.case_input(shape)
        d[tag + "_x"] = x
        d[tag] = m(x)
        assert torch.isfinite(d[tag]).all(), tag
        d[tag + "_keys"] = np.array(sorted(m.state_dict()))
        d[tag + "_init_pos"] = m.init_pos
        off = (m.offset(torch.nn.functional.pixel_shuffle(x, 2) if args[2] == "pl" else x)).abs().max() * (0.5 if args[4] else 0.25)
        print(tag, tuple(d[tag].shape), f"largest offset term {float(off):.2f} px")
    np.savez_compressed(os.path.join(HERE, "dysample_ops.npz"), **{k: (v.numpy() if torch.is_tensor(v) else v) for k, v in d.items()})
    print("dysample_ops", len(d))


def cfg(scale):
    d = yaml.safe_load(open(YAML, encoding="utf-8"))
    d["scale"] = scale
    return d


def build(scale, gain=GAIN):
    m = DetectionModel(cfg(scale), ch=3, nc=80, verbose=False).eval()
    m.load_state_dict(dysample_synth.state_dict(m.state_dict(), gain))
    m.fuse(verbose=False)
    return m


def model(scale, tag, b, h, w, layers, gain=GAIN, first=0, skip_copies=False, base=None, skip=()):
    """layers: record the outputs of layers >= first too; first > 0 and skip_copies (no Concat outputs: the tests rebuild them from their
    inputs) keep the file under the size limit.  base: the yolov13 golden of the same scale and image.  The synthetic weights depend on
    key name and shape only and the graph is yolov13's up to layer 9, so layers 0-9, 11, 12 and 14 repeat that file bit for bit: they are
    left out here (checked, not assumed) and the tests read them from `base`.  skip: layers left out to stay at the size of `base`
    (layer 13 of the l file, FullPAD_Tunnel: x0 + gate * x1 of two stored maps, which the tests rebuild in float64 where a later layer
    reads it; the module itself is checked in the n file)."""
    m = build(scale, gain)
    d = {}
    hs = [l.register_forward_hook(lambda mod, inp, out, i=l.i: d.__setitem__(f"layer{i}", out.clone()) if torch.is_tensor(out) else None)
          for l in (m.model if layers else []) if l.i >= first and l.i not in skip and not (skip_copies and l.type.endswith("Concat"))]
    y, raw = m(synth.synth_images(b, h, w))
    for hk in hs:
        hk.remove()
    assert torch.isfinite(y).all(), tag
    if base:
        g = np.load(os.path.join(HERE, base + ".npz"))
        same = [k for k in d if k in g and np.array_equal(g[k], d[k].numpy())]
        assert {f"layer{i}" for i in (4, 5, 6, 7, 8, 9, 11, 12, 14)} <= set(same), same
        for k in same:
            del d[k]
        print(tag, "shared with", base, ":", " ".join(k[5:] for k in same))
    d["y"] = y
    for i, r in enumerate(raw):
        d[f"raw{i}"] = r
    np.savez_compressed(os.path.join(HERE, f"{tag}.npz"), **{k: v.numpy() for k, v in d.items()})
    print(tag, len(d), tuple(y.shape), os.path.getsize(os.path.join(HERE, f"{tag}.npz")))


def structure():
    out = {}
    for sc in "nslx":
        m = DetectionModel(cfg(sc), ch=3, nc=80, verbose=False)
        out[NAME.format(sc)] = dict(params=sum(p.numel() for p in m.parameters()), save=list(m.save),
                                    layers=[dict(i=l.i, f=l.f, type=l.type, np=int(l.np)) for l in m.model],
                                    init_pos={str(i): m.model[i].init_pos.flatten().tolist() for i in dysample_synth.DYSAMPLE_LAYERS},
                                    keys=list(m.state_dict()))
        print(sc, out[NAME.format(sc)]["params"])
    with open(os.path.join(HERE, "structure_dysample.json"), "w") as f:  # one line per model: read by the tests only
        f.write("{\n" + ",\n".join(json.dumps(k) + ": " + json.dumps(v, separators=(",", ":")) for k, v in out.items()) + "\n}\n")


if __name__ == "__main__":
    modules()
    model("n", "yolov13n_dysample_64x96", 1, 64, 96, layers=True, base="yolov13n_64x96")
    model("n", "yolov13n_dysample_96x160", 1, 96, 160, layers=False)
    model("l", "yolov13l_dysample_64", 1, 64, 64, layers=True, first=4, skip_copies=True, base="yolov13l_64", skip=(13,))
    structure()
