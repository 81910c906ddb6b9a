"""Golden vectors for YOLOv12 (reference ultralytics/cfg/models/v12/yolov12.yaml; A2C2f / ABlock / AAttn at
ultralytics/nn/modules/block.py:1272-1465, the l/x rule at nn/tasks.py:1073-1077).  CPU fp32, synthetic weights and inputs
(synthdata.py), the real reference imported through _ref_import:

    python tests/golden/make_golden_v12.py

writes tests/golden/v12_ops.npz (module level), yolov12n_64x96.npz (per-layer outputs + y), yolov12n_96x160.npz,
yolov12l_64.npz and structure_v12.json.  Runs only where the reference exists; the GPU box never runs this.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import _ref_import  # noqa: E402

_ref_import.setup()
import numpy as np  # noqa: E402
import torch  # noqa: E402

import synthdata as synth  # noqa: E402
from ultralytics.nn.tasks import DetectionModel  # noqa: E402
from ultralytics.nn.modules import block as rb  # noqa: E402

torch.set_grad_enabled(False)
# synthetic-weight gain of the whole-model goldens.  Area attention has no key-dim reduction, so its scores grow with the square of
# the activations: at gain 1.9 (n) or 1.0 (l) the P4/P5 softmax rows are near one-hot and the reference's own fp32 forward differs
# from its fp64 forward by more than the 1e-4 bar in up to 2 % of a layer's outputs; at 0.5 every layer of n and l is within it
GAIN = 0.5

# (tag, constructor, args, input shape): token counts not a multiple of 16, areas that split rows, a2=False, residual + gamma
MODULES = [
    ("aattn_a1", rb.AAttn, (64, 2, 1), (2, 64, 5, 7)),         # 35 tokens
    ("aattn_a4", rb.AAttn, (64, 2, 4), (1, 64, 6, 10)),        # 15 tokens per area, areas split rows
    ("aattn_a1_big", rb.AAttn, (32, 1, 1), (1, 32, 20, 21)),   # 420 tokens: several key tiles
    ("aattn_a4_h4", rb.AAttn, (128, 4, 4), (1, 128, 8, 10)),   # 20 tokens per area, 4 heads
    ("ablock_a4", rb.ABlock, (64, 2, 1.2, 4), (2, 64, 4, 6)),  # 6 tokens per area
    ("a2c2f_a2", rb.A2C2f, (64, 64, 1, True, 4), (2, 64, 6, 10)),
    ("a2c2f_c3k", rb.A2C2f, (64, 64, 2, False, -1), (2, 64, 6, 10)),
    ("a2c2f_res", rb.A2C2f, (64, 64, 1, True, 1, True, 1.5), (1, 64, 5, 7)),
]


def filled(mod, prefix, gain=1.9):
    mod.eval()
    for mm in mod.modules():
        if isinstance(mm, torch.nn.BatchNorm2d):
            mm.eps = 1e-3  # initialize_weights, torch_utils.py:416
    mod.load_state_dict({k: synth.synth_tensor(prefix + "." + k, tuple(v.shape), gain=gain) for k, v in mod.state_dict().items()})
    return mod


def modules():
    d = {}
    for tag, cls, args, shape in MODULES:
        m = filled(cls(*args), tag)
        x = synth.synth_images(shape[0], shape[2], shape[3], c=shape[1]) * 2 - 1
        d[tag + "_x"] = x
        d[tag] = m(x)
        d[tag + "_keys"] = np.array(sorted(m.state_dict()))
    np.savez_compressed(os.path.join(HERE, "v12_ops.npz"), **{k: (v.numpy() if torch.is_tensor(v) else v) for k, v in d.items()})
    print("v12_ops", len(d))


def build(name, gain=1.9):
    m = DetectionModel(name, ch=3, nc=80, verbose=False).eval()
    m.load_state_dict(synth.synth_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, gain=gain))
    m.fuse(verbose=False)
    return m


def model(name, tag, b, h, w, layers, gain=1.9, first=0):
    """layers: record the outputs of layers >= first too (first > 0 keeps the file under the size limit)."""
    m = build(name, gain)
    d = {}
    hs = [l.register_forward_hook(lambda mod, inp, out, i=l.i: d.__setitem__(f"layer{i}", out.clone()) if torch.is_tensor(out) else None)
          for l in (m.model if layers else []) if l.i >= first]
    y, raw = m(synth.synth_images(b, h, w))
    for hk in hs:
        hk.remove()
    d["y"] = y
    for i, r in enumerate(raw):
        d[f"raw{i}"] = r
    np.savez_compressed(os.path.join(HERE, f"{tag}.npz"), **{k: v.numpy() for k, v in d.items()})
    print(tag, len(d), tuple(y.shape))


def structure():
    out = {}
    for sc in "nslmx":
        m = DetectionModel(f"yolov12{sc}.yaml", ch=3, nc=80, verbose=False)
        out[f"yolov12{sc}.yaml"] = dict(params=sum(p.numel() for p in m.parameters()), save=list(m.save),
                                        layers=[dict(i=l.i, f=l.f, type=l.type, np=int(l.np)) for l in m.model],
                                        keys=list(m.state_dict()))
        print(sc, out[f"yolov12{sc}.yaml"]["params"])
    json.dump(out, open(os.path.join(HERE, "structure_v12.json"), "w"), indent=0)


if __name__ == "__main__":
    modules()
    model("yolov12n.yaml", "yolov12n_64x96", 1, 64, 96, layers=True, gain=GAIN)
    model("yolov12n.yaml", "yolov12n_96x160", 1, 96, 160, layers=False, gain=GAIN)
    model("yolov12l.yaml", "yolov12l_64", 1, 64, 64, layers=True, gain=GAIN, first=4)
    structure()
