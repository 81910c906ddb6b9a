"""Golden vectors for YOLOv13-LGL (reference ultralytics/cfg/models/v13/yolov13-DSC3K2_LGL.yaml; Mlp ... DSC3K2_LGL at
ultralytics/nn/modules/block.py:3042-3345, the parse rules at nn/tasks.py:1031-1072).  CPU fp32, synthetic weights and inputs
(synthdata.py with the LGL override of tests/lgl_synth.py), the real reference imported through _ref_import:

    python tests/golden/make_golden_v13_lgl.py

writes tests/golden/v13_lgl_ops.npz (module level), yolov13n_lgl_64x96.npz (per-layer outputs + y; layer 30 is a 2x3 map there: the
odd un-pool path inside the model), yolov13n_lgl_96x160.npz, yolov13l_lgl_64.npz and structure_v13_lgl.json.  Runs only where the
reference exists; the GPU box never runs this.
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

import lgl_synth  # noqa: E402
import synthdata as synth  # noqa: E402
from ultralytics.nn.tasks import DetectionModel  # noqa: E402
from ultralytics.nn.modules import block as rb  # noqa: E402

torch.set_grad_enabled(False)
GAIN = lgl_synth.GAIN
NAME = "yolov13{}-DSC3K2_LGL.yaml"


def modules():
    d = {}
    for tag, prefix, cls, args, kw, shape, lgl in lgl_synth.CASES:
        m = lgl_synth.fill(getattr(rb, cls)(*args, **kw), prefix, lgl)
        x = lgl_synth.case_input(shape)
        d[tag + "_x"] = x
        d[tag] = m(x)
        assert torch.isfinite(d[tag]).all(), tag
        d[prefix + "_keys"] = np.array(sorted(m.state_dict()))
    np.savez_compressed(os.path.join(HERE, "v13_lgl_ops.npz"), **{k: (v.numpy() if torch.is_tensor(v) else v) for k, v in d.items()})
    print("v13_lgl_ops", len(d))


def build(name, gain=GAIN):
    m = DetectionModel(name, ch=3, nc=80, verbose=False).eval()
    m.load_state_dict(lgl_synth.state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, gain=gain))
    m.fuse(verbose=False)
    return m


def model(name, tag, b, h, w, layers, gain=GAIN, first=0, skip_copies=False):
    """layers: record the outputs of layers >= first too; first > 0 and skip_copies (no Concat / Upsample outputs: the tests rebuild
    them from their inputs) keep the file under the size limit."""
    m = build(name, gain)
    d = {}
    copies = ("Concat", "Upsample")
    hs = [l.register_forward_hook(lambda mod, inp, out, i=l.i: d.__setitem__(f"layer{i}", out.clone()) if torch.is_tensor(out) else None)
          for l in (m.model if layers else []) if l.i >= first and not (skip_copies and l.type.endswith(copies))]
    y, raw = m(synth.synth_images(b, h, w))
    for hk in hs:
        hk.remove()
    assert torch.isfinite(y).all(), tag
    d["y"] = y
    for i, r in enumerate(raw):
        d[f"raw{i}"] = r
    np.savez_compressed(os.path.join(HERE, f"{tag}.npz"), **{k: v.numpy() for k, v in d.items()})
    print(tag, len(d), tuple(y.shape), os.path.getsize(os.path.join(HERE, f"{tag}.npz")))


def structure():
    out = {}
    for sc in "nslx":
        m = DetectionModel(NAME.format(sc), ch=3, nc=80, verbose=False)
        heads = {str(l.i): [u.lgl.lgl.SelfAttn.attn.num_heads for u in l.m] for l in m.model if l.type.endswith("DSC3K2_LGL")}
        out[NAME.format(sc)] = dict(params=sum(p.numel() for p in m.parameters()), save=list(m.save),
                                    layers=[dict(i=l.i, f=l.f, type=l.type, np=int(l.np)) for l in m.model], heads=heads,
                                    keys=list(m.state_dict()))
        print(sc, out[NAME.format(sc)]["params"], heads)
    with open(os.path.join(HERE, "structure_v13_lgl.json"), "w") as f:  # one line per model: read by the tests only
        f.write("{\n" + ",\n".join(json.dumps(k) + ": " + json.dumps(v, separators=(",", ":")) for k, v in out.items()) + "\n}\n")


if __name__ == "__main__":
    modules()
    model(NAME.format("n"), "yolov13n_lgl_64x96", 1, 64, 96, layers=True)
    model(NAME.format("n"), "yolov13n_lgl_96x160", 1, 96, 160, layers=False)
    model(NAME.format("l"), "yolov13l_lgl_64", 1, 64, 64, layers=True, first=4, skip_copies=True)
    structure()
