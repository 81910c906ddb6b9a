"""Golden vectors for YOLO-World v2: MaxSigmoidAttnBlock and C2fAttn (reference ultralytics/nn/modules/block.py:544-603), WorldDetect with
BNContrastiveHead (nn/modules/head.py:479-521, block.py:670-692), the C2fAttn parse rule and WorldModel (nn/tasks.py:624-695, 1037-1041), from
the real reference imported through _ref_import.  CPU fp32, synthetic weights, inputs and text (tests/world_synth.py).

    python tests/golden/make_golden_world.py

writes structure_world.json, world_ops.npz and yolov8n_worldv2_64x96.npz.  Next to every module output the file holds the reference's own
fp32 error against the float64 restatement (tests/fp64_world_ref.py) on the same operands.  torchvision.ops.nms is the documented stand-in
of make_golden.py (oracle/nms.py).  Runs only where the reference exists.
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

import fp64_world_ref as f64  # noqa: E402
import synthdata as synth  # noqa: E402
import world_synth as ws  # noqa: E402
from oracle.nms import tv_nms  # noqa: E402

tv.ops.nms = lambda b, s, t: torch.as_tensor(tv_nms(b.numpy(), s.numpy(), t), dtype=torch.long)
from ultralytics.nn.modules.block import C2fAttn, MaxSigmoidAttnBlock  # noqa: E402
from ultralytics.nn.modules.head import WorldDetect  # noqa: E402
from ultralytics.nn.tasks import WorldModel, guess_model_task  # noqa: E402
from ultralytics.utils import ops as rops  # noqa: E402

torch.set_grad_enabled(False)
CFG = os.path.join(ROOT, "edge-yolo_amd", "cfg", "models", "v8", "yolov8-worldv2.yaml")


def cfg(scale):
    d = yaml.safe_load(open(CFG, encoding="utf-8"))
    d["scale"] = scale
    return d


def structure():
    out = {}
    for sc in ws.SCALES:
        d = cfg(sc)
        assert guess_model_task(d) == "detect"
        m = WorldModel(d, ch=3, nc=80, verbose=False)
        assert guess_model_task(m) == "detect"
        attn = [dict(i=l.i, nh=l.attn.nh, hc=l.attn.hc, ec=l.attn.ec is not None, c=l.c) for l in m.model if isinstance(l, C2fAttn)]
        assert all(a["hc"] == 32 and not a["ec"] and a["c"] == 32 * a["nh"] for a in attn), attn
        y = m.eval()(synth.synth_images(2, 64, 96))[0]
        assert tuple(y.shape) == (2, 84, 126)
        out[ws.NAME.format(sc)] = dict(params=sum(p.numel() for p in m.parameters()), save=list(m.save), stride=[float(s) for s in m.stride],
                                       layers=[dict(i=l.i, f=l.f, type=l.type, np=int(l.np)) for l in m.model], attn=attn, keys=list(m.state_dict()))
        print(sc, out[ws.NAME.format(sc)]["params"], [(a["nh"], a["hc"]) for a in attn])
    assert out[ws.NAME.format("n")]["params"] == ws.N_PARAMS
    with open(os.path.join(HERE, "structure_world.json"), "w") as f:
        f.write("{\n" + ",\n".join(json.dumps(k) + ": " + json.dumps(v, separators=(",", ":")) for k, v in out.items()) + "\n}\n")


def ops_file():
    d = {}
    for tag, kw, shape, n in ws.ATTN_CASES:
        m = MaxSigmoidAttnBlock(**kw).eval()
        m.load_state_dict(ws.state_dict(m.state_dict(), prefix=tag + "."))
        x = ws.case_input(tag, shape)
        guide = ws.normalized(ws.text(tag, n)).repeat(shape[0], 1, 1)
        y = m(x, guide)
        p, g = m.proj_conv(x), m.gl(guide)
        scale = m.scale.flatten().numpy() if torch.is_tensor(m.scale) else None
        y64, _ = f64.max_sigmoid_attn64(x.numpy(), p.numpy(), g.numpy(), m.bias.numpy(), scale)
        d[tag + "_y"], d[tag + "_p"], d[tag + "_g"] = y, p, g
        d[tag + "_E"] = np.float64(np.abs(y.numpy().astype(np.float64) - y64).max())
        print(tag, tuple(y.shape), f"E {float(d[tag + '_E']):.2e}")
    tag, kw, shape, n = ws.C2FATTN_CASE
    m = C2fAttn(**kw).eval()
    m.load_state_dict(ws.state_dict(m.state_dict(), prefix=tag + "."))
    d[tag + "_y"] = m(ws.case_input(tag, shape), ws.normalized(ws.text(tag, n)).repeat(shape[0], 1, 1))
    d[tag + "_keys"] = np.array(list(m.state_dict()))
    print(tag, tuple(d[tag + "_y"].shape))
    # WorldDetect: raw and decoded outputs, the class towers' hidden maps and the reference's fp32 error on its own class tail
    tag, kw, shapes, n = ws.HEAD_CASE
    m = WorldDetect(**kw).eval()
    m.stride = torch.tensor([8.0, 16.0, 32.0])
    m.load_state_dict(ws.state_dict(m.state_dict(), prefix=tag + "."))
    m.nc = n
    txt = ws.text(tag, n)[None]
    xs = [ws.case_input(f"{tag}{i}", s) for i, s in enumerate(shapes)]
    y, raw = m([x.clone() for x in xs], txt)
    d[tag + "_y"] = y
    d[tag + "_keys"] = np.array(list(m.state_dict()))
    E = 0.0
    for i, r in enumerate(raw):
        h = m.cv3[i][1](m.cv3[i][0](xs[i]))
        d[f"{tag}_raw{i}"], d[f"{tag}_h{i}"] = r, h
        c, bn, hd = m.cv3[i][2], m.cv4[i].norm, m.cv4[i]
        l64 = f64.contrastive_tail64(h.numpy(), c.weight.numpy(), c.bias.numpy(), bn.weight.numpy(), bn.bias.numpy(), bn.running_mean.numpy(),
                                     bn.running_var.numpy(), bn.eps, txt.numpy(), hd.logit_scale.numpy(), hd.bias.numpy())
        E = max(E, float(np.abs(r[:, 64:].numpy().astype(np.float64) - l64).max()))
    d[tag + "_E"] = np.float64(E)
    print(tag, tuple(y.shape), f"E {E:.2e}")
    np.savez_compressed(os.path.join(HERE, "world_ops.npz"), **{k: (v.numpy() if torch.is_tensor(v) else v) for k, v in d.items()})
    size = os.path.getsize(os.path.join(HERE, "world_ops.npz"))
    print("world_ops", len(d), size)
    assert size < 1 << 20


def model(tag, shape, n, conf):
    m = WorldModel(cfg("n"), ch=3, nc=80, verbose=False).eval()
    m.load_state_dict(ws.state_dict(m.state_dict()))
    m.fuse(verbose=False)
    m.txt_feats = ws.normalized(ws.text(tag, n))  # what set_classes leaves behind CLIP (tasks.py:650-652)
    m.model[-1].nc = n
    x = synth.synth_images(*shape)
    y, raw = m(x)
    assert torch.isfinite(y).all() and tuple(y.shape) == (shape[0], 4 + n, 126), tag
    d = {"y": y}
    for i, r in enumerate(raw):
        d[f"raw{i}"] = r
    dets = rops.non_max_suppression(y.clone(), conf, 0.7, max_det=300, max_time_img=1e6)  # detect/predict.py:25-33
    for i, det in enumerate(dets):
        det = det.clone()
        det[:, :4] = rops.scale_boxes(shape[1:], det[:, :4], (*shape[1:], 3))  # detect/predict.py:36-39: a tensor source, gain 1, no padding: a clip
        d[f"det{i}"] = det
        print(tag, "image", i, "kept", len(det), "max score", float(y[i, 4:].max()))
    assert sum(len(t) for t in dets) >= 5, "lower conf"
    d["conf"] = np.float64(conf)
    np.savez_compressed(os.path.join(HERE, f"{tag}.npz"), **{k: (v.numpy() if torch.is_tensor(v) else v) for k, v in d.items()})
    size = os.path.getsize(os.path.join(HERE, f"{tag}.npz"))
    print(tag, len(d), tuple(y.shape), size)
    assert size < 1 << 20


if __name__ == "__main__":
    structure()
    ops_file()
    model(ws.MODEL_TAG, ws.MODEL_SHAPE, ws.MODEL_TEXTS, conf=0.25)
