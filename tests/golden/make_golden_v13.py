"""Golden vectors for YOLOv13 (reference ultralytics/cfg/models/v13/yolov13.yaml; DSC3K2 ... FullPAD_Tunnel at
ultralytics/nn/modules/block.py:1564-2008, DSConv at conv.py:87-104, the parse rules at nn/tasks.py:1029-1125).  CPU fp32, synthetic
weights and inputs (synthdata.py), the real reference imported through _ref_import:

    python tests/golden/make_golden_v13.py

writes tests/golden/v13_ops.npz (module level), yolov13n_64x96.npz (per-layer outputs + y), yolov13n_96x160.npz, yolov13l_64.npz and
structure_v13.json.  Runs only where the reference exists; the GPU box never runs this.
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
from ultralytics.nn.modules import conv as rc  # noqa: E402

torch.set_grad_enabled(False)
# synthetic-weight gain of every golden.  The reference's own fp32 forward against its fp64 forward on a 96x160 image: at 0.5 the worst
# layer is 6.7e-7 (n) / 1.2e-6 (l) of its max |value|; at 1.0 yolov13l reaches 7.8e-3 (layers 6, 12, 32), above the 1e-4 bar
GAIN = 0.5

# (tag, constructor, args, input shapes): token counts not a multiple of 16, E 4 / 8 / 12, odd maps for the stride-2 / pooling layers
MODULES = [
    ("hgc_d64_e4", rb.AdaHGComputation, (64, 4, 4), [(2, 64, 5, 7)]),
    ("hgc_d128_e8", rb.AdaHGComputation, (128, 8, 8), [(2, 128, 6, 10)]),
    ("hgc_d64_e12", rb.AdaHGComputation, (64, 12, 4), [(1, 64, 20, 21)]),
    ("hgc_d128_e12_mean", rb.AdaHGComputation, (128, 12, 8, 0.1, "mean"), [(1, 128, 3, 5)]),
    ("c3ah", rb.C3AH, (64, 64, 1.0, 8), [(2, 64, 6, 10)]),
    ("fuse_adj", rb.FuseModule, (32, True), [(2, 32, 12, 16), (2, 32, 6, 8), (2, 64, 3, 4)]),   # x0 32 + x1 32 + x2 64 = 4 c_in
    ("fuse_noadj", rb.FuseModule, (32, False), [(1, 32, 13, 17), (1, 32, 6, 8), (1, 32, 3, 4)]),  # odd x0: floor
    ("hyperace_n1", rb.HyperACE, (32, 64, 1, 4, True, True, 0.5, 1, "both", True), [(2, 32, 12, 16), (2, 32, 6, 8), (2, 64, 3, 4)]),
    ("hyperace_n2", rb.HyperACE, (32, 64, 2, 8, True, True, 0.5, 1, "both", False), [(1, 32, 12, 20), (1, 32, 6, 10), (1, 32, 3, 5)]),
    ("hyperace_dsb", rb.HyperACE, (32, 64, 1, 4, False, False, 0.5, 1, "both", False), [(1, 32, 8, 8), (1, 32, 4, 4), (1, 32, 2, 2)]),
    ("down_adj", rb.DownsampleConv, (32, True), [(2, 32, 9, 11)]),
    ("down_noadj", rb.DownsampleConv, (32, False), [(1, 32, 8, 10)]),
    ("fullpad", rb.FullPAD_Tunnel, (), [(2, 32, 5, 7), (2, 32, 5, 7)]),
    ("dsconv_s2_even", rc.DSConv, (32, 64, 3, 2), [(2, 32, 10, 12)]),
    ("dsconv_s2_odd", rc.DSConv, (32, 48, 3, 2), [(1, 32, 9, 13)]),
    ("dsc3k2_dsb", rb.DSC3K2, (64, 64, 1, False), [(2, 64, 8, 10)]),
    ("dsc3k2_dsc3k", rb.DSC3K2, (64, 64, 1, True), [(1, 64, 8, 10)]),
]


def filled(mod, prefix, gain=GAIN):
    mod.eval()
    for mm in mod.modules():
        if isinstance(mm, torch.nn.BatchNorm2d):
            mm.eps = 1e-3  # initialize_weights, torch_utils.py:416
    mod.load_state_dict({k: synth.synth_tensor(prefix + "." + k, tuple(v.shape), gain=gain) for k, v in mod.state_dict().items()})
    return mod


def modules():
    d = {}
    for tag, cls, args, shapes in MODULES:
        m = filled(cls(*args), tag)
        xs = [synth.synth_images(s[0], s[2], s[3], c=s[1]) * 2 - 1 for s in shapes]
        for i, x in enumerate(xs):
            d[f"{tag}_x{i}"] = x
        d[tag] = m(xs if len(xs) > 1 else xs[0])
        d[tag + "_keys"] = np.array(sorted(m.state_dict()))
    # the reference's own token form: AdaHGConv on (B, N, D)
    m = filled(rb.AdaHGConv(64, 8, 4), "hgconv_tokens")
    x = synth.synth_images(2, 1, 37, c=64).flatten(2).transpose(1, 2).contiguous() * 2 - 1
    d["hgconv_tokens_x0"], d["hgconv_tokens"] = x, m(x)
    d["hgconv_tokens_keys"] = np.array(sorted(m.state_dict()))
    np.savez_compressed(os.path.join(HERE, "v13_ops.npz"), **{k: (v.numpy() if torch.is_tensor(v) else v) for k, v in d.items()})
    print("v13_ops", len(d))


def build(name, gain=GAIN):
    m = DetectionModel(name, ch=3, nc=80, verbose=False).eval()
    m.load_state_dict(synth.synth_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, gain=gain))
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
    d["y"] = y
    for i, r in enumerate(raw):
        d[f"raw{i}"] = r
    np.savez_compressed(os.path.join(HERE, f"{tag}.npz"), **{k: v.numpy() for k, v in d.items()})
    print(tag, len(d), tuple(y.shape))


def structure():
    out = {}
    for sc in "nslx":
        m = DetectionModel(f"yolov13{sc}.yaml", ch=3, nc=80, verbose=False)
        out[f"yolov13{sc}.yaml"] = dict(params=sum(p.numel() for p in m.parameters()), save=list(m.save),
                                        layers=[dict(i=l.i, f=l.f, type=l.type, np=int(l.np)) for l in m.model],
                                        keys=list(m.state_dict()))
        print(sc, out[f"yolov13{sc}.yaml"]["params"])
    json.dump(out, open(os.path.join(HERE, "structure_v13.json"), "w"), indent=0)


if __name__ == "__main__":
    modules()
    model("yolov13n.yaml", "yolov13n_64x96", 1, 64, 96, layers=True)
    model("yolov13n.yaml", "yolov13n_96x160", 1, 96, 160, layers=False)
    model("yolov13l.yaml", "yolov13l_64", 1, 64, 64, layers=True, first=4, skip_copies=True)
    structure()
