"""Golden vectors for the ResNet classifiers (ResNetLayer, reference ultralytics/nn/modules/block.py:505-541, parse rule nn/tasks.py:1086-1087)
and the YOLOv8 task models (cls, seg, seg-p6, pose, pose-p6, obb), from the real reference imported through _ref_import.  CPU fp32,
synthetic weights and inputs (tests/resnet_synth.py).  The structure file is built from the REFERENCE's own YAML files, so it also pins
that the YAMLs written for this project build the same graphs.

    python tests/golden/make_golden_resnet.py

writes structure_v8tasks.json, resnet50_cls.npz, resnet101_cls.npz, resnetval_case.npz and one npz per entry of resnet_synth.V8_MODELS.
Asserted here: for both ResNets the reference, run again with weights and image rounded to f16, keeps its top-1 class and its top-5 set (the
condition under which the f16 test is decidable; resnet_synth.RESNET_SEED holds the first seed for which it is true).  Runs only where the
reference exists.
"""
import hashlib
import json
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
import _ref_import  # noqa: E402

tv = _ref_import.setup()
import numpy as np  # noqa: E402
import torch  # noqa: E402

import resnet_synth as rs  # noqa: E402
import synthdata as synth  # noqa: E402
from oracle.nms import tv_nms  # noqa: E402

tv.ops.nms = lambda b, s, t: torch.as_tensor(tv_nms(b.numpy(), s.numpy(), t), dtype=torch.long)
from ultralytics.models.yolo.classify.val import ClassificationValidator as RCV  # noqa: E402
from ultralytics.nn.tasks import ClassificationModel, OBBModel, PoseModel, SegmentationModel, guess_model_task, yaml_model_load  # noqa: E402
from ultralytics.utils import metrics as rm  # noqa: E402
from ultralytics.utils import ops as rops  # noqa: E402

torch.set_grad_enabled(False)
ClassificationModel.info = lambda self, *a, **k: None  # (the summary line needs thop, which _ref_import replaces by an inert stand-in)
MODEL = {"classify": ClassificationModel, "segment": SegmentationModel, "pose": PoseModel, "obb": OBBModel}


def _save(name, d):
    path = os.path.join(HERE, name)
    np.savez_compressed(path, **{k: (v.numpy() if torch.is_tensor(v) else v) for k, v in d.items()})
    size = os.path.getsize(path)
    print(name, len(d), size)
    assert size < 1 << 20, name


def keys_sha1(keys):
    return hashlib.sha1("\n".join(keys).encode()).hexdigest()


def structure():
    out = {}
    for base in rs.V8_TASK_YAMLS:
        task = rs.task_of(base)
        for sc in rs.SCALES:
            name = rs.scaled(base, sc)
            d = yaml_model_load(name)  # the reference's own file
            assert guess_model_task(d) == task and d["scale"] == sc, name
            m = MODEL[task](d, ch=3, nc=1000 if task == "classify" else None, verbose=False)
            keys = list(m.state_dict())
            e = dict(task=task, params=sum(p.numel() for p in m.parameters()), save=list(m.save), stride=[float(s) for s in m.stride],
                     layers=[dict(i=l.i, f=l.f, type=l.type, np=int(l.np)) for l in m.model], nkeys=len(keys), keys_sha1=keys_sha1(keys))
            if sc == "n":  # the full list once per file; the other scales are pinned by count and digest
                e["keys"] = keys
            out[name] = e
            print(name, e["params"], e["nkeys"], e["stride"])
    for base in ("yolov8-cls-resnet50.yaml", "yolov8-cls-resnet101.yaml"):  # parse_model does not scale a ResNetLayer row
        n, x = out[rs.scaled(base, "n")], out[rs.scaled(base, "x")]
        assert n["params"] == x["params"] and n["keys_sha1"] == x["keys_sha1"] and n["layers"] == x["layers"]
    path = os.path.join(HERE, "structure_v8tasks.json")
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join(json.dumps(k) + ": " + json.dumps(v, separators=(",", ":")) for k, v in out.items()) + "\n}\n")
    print("structure_v8tasks.json", os.path.getsize(path))
    assert os.path.getsize(path) < 1 << 20


def _resnet(name, nc, seed, f16=False):
    m = ClassificationModel(yaml_model_load(name), ch=3, nc=nc, verbose=False).eval()
    sd = rs.state_dict(m.state_dict(), seed=seed)
    m.load_state_dict(rs.f16_state_dict(sd) if f16 else sd)
    m.fuse(verbose=False)
    return m


def _layers(m, x):
    outs = []
    for layer in m.model[:-1]:
        x = layer(x)
        outs.append(x)
    return outs


def _decidable(name, seed, x):
    """top-5 of the fp32 run and of the run with f16-rounded weights and image -> (ok, probs, logits, top5)."""
    y, logits = _resnet(name, rs.RESNET_NC, seed)(x)
    yh, _ = _resnet(name, rs.RESNET_NC, seed, f16=True)(x.half().float())
    top, toph = y.argsort(1, descending=True)[:, :5], yh.argsort(1, descending=True)[:, :5]
    ok = top[:, 0].tolist() == toph[:, 0].tolist() and [set(r) for r in top.tolist()] == [set(r) for r in toph.tolist()]
    return ok, y, logits, top.type(torch.int32)


def resnet_files():
    x64 = synth.synth_images(*rs.RESNET_SHAPE)
    for name, fname in (("yolov8n-cls-resnet50.yaml", "resnet50_cls.npz"), ("yolov8n-cls-resnet101.yaml", "resnet101_cls.npz")):
        seed = next(s for s in range(16) if _decidable(name, s, x64)[0])
        assert seed == rs.RESNET_SEED[name], f"set resnet_synth.RESNET_SEED['{name}'] = {seed}"
        _, y, logits, top = _decidable(name, seed, x64)
        assert torch.isfinite(y).all() and tuple(y.shape) == (2, rs.RESNET_NC)
        d = {"logits": logits, "probs": y, "top5": top}
        print(name, "seed", seed, "top5", top.tolist(), "top1conf", y.max(1).values.tolist())
        if "resnet50" in name:
            m = _resnet(name, rs.RESNET_NC, seed)
            x32 = synth.synth_images(*rs.RESNET_LAYER_SHAPE)
            for i, o in enumerate(_layers(m, x32)):
                d[f"layer{i}"] = o
                print(" layer", i, tuple(o.shape), f"max |x| {float(o.abs().max()):.2f} mean {float(o.mean()):.3f}")
            d["probs32"], d["logits32"] = m(x32)
        _save(fname, d)


def _validator(nc):
    class V(RCV):
        def __init__(self):  # the validator's own set-up needs a dataset / cfg; only the metric plumbing is exercised
            pass
    v = V()
    v.device = torch.device("cpu")
    v.args = types.SimpleNamespace(plots=False, half=False, conf=0.001)
    v.names = {i: str(i) for i in range(nc)}
    v.nc = nc
    v.metrics = rm.ClassifyMetrics()
    v.pred, v.targets = [], []
    return v


def val_case():
    nc, name = rs.VAL_NC, "yolov8n-cls-resnet50.yaml"
    m = _resnet(name, nc, rs.RESNET_SEED[name])
    probs = [m(rs.val_images(i))[0] for i in range(rs.VAL_BATCHES)]
    allp = torch.cat(probs).numpy().astype(np.float64)
    s = -np.sort(-allp, axis=1)[:, :6]
    gap = np.abs(np.diff(s, axis=1)).min(1)
    # the fp32 parity bar on a probability p is 2e-4 + 1e-4 p <= 3e-4, and both neighbours may move by it: the ranking of the first six
    # probabilities of every row does not depend on rounding when they are more than 6e-4 apart
    assert float(gap.min()) > 6e-4, float(gap.min())
    order = np.argsort(-allp, axis=1, kind="stable")
    place = [0, 1, 4, 5, 0, nc - 1, 2, 0]  # labels from the ranking: the winner, the runner-up, the fifth, the sixth (a top-5 miss), the last ...
    cls = np.array([order[i, place[i % len(place)]] for i in range(len(allp))], np.int64)
    B = rs.VAL_SHAPE[0]
    v = _validator(nc)
    for i, p in enumerate(probs):
        v.update_metrics(p, {"cls": torch.as_tensor(cls[i * B:(i + 1) * B])})
    res = v.get_stats()
    keys, values = np.array(list(res.keys())), np.array([float(t) for t in res.values()])
    print("resnetval", dict(zip(keys.tolist(), values.tolist())), f"gap {float(gap.min()):.2e}")
    assert 0 < values[0] < values[1] < 1
    _save("resnetval_case.npz", dict(cls=cls, probs=torch.cat(probs), pred=torch.cat(v.pred).numpy(), keys=keys, values=values, gap=gap, nc=np.int64(nc),
                                     top5=torch.tensor(order[:, :5].astype(np.int32))))


def v8_files():
    for name, (tag, (b, h, w)) in rs.V8_MODELS.items():
        task = rs.task_of(name)
        m = MODEL[task](yaml_model_load(name), ch=3, nc=rs.RESNET_NC if task == "classify" else None, verbose=False).eval()
        m.load_state_dict(rs.state_dict(m.state_dict()))
        m.fuse(verbose=False)
        x = synth.synth_images(b, h, w)
        out = m(x)
        if task == "classify":
            y, logits = out
            d = {"probs": y, "logits": logits, "top5": y.argsort(1, descending=True)[:, :5].type(torch.int32)}
            _save(tag + ".npz", d)
            continue
        y, aux = out
        assert torch.isfinite(y).all(), tag
        nc = m.model[-1].nc
        d = {"y": y, "nc": np.int64(nc), "stride": m.stride.numpy()}
        for i, r in enumerate(aux[0]):
            d[f"raw{i}"] = r
        if task == "segment":
            d["mc"], d["p"] = aux[1], aux[2]
        elif task == "pose":
            d["kpt"] = aux[1]
        else:
            d["angle"] = aux[1]
        # the predict-time rows on the reference's own output: NMS, then the boxes scaled to the (equal) source size and rounded
        conf = rs.V8_CONF
        while True:
            dets = rops.non_max_suppression(y.clone(), conf, 0.7, nc=nc, max_det=300, max_time_img=1e6, rotated=task == "obb")
            if min(len(t) for t in dets) >= 3 or conf < 1e-4:
                break
            conf /= 2
        d["conf"] = np.float64(conf)
        for i, pred in enumerate(dets):
            d[f"det{i}"] = pred.clone()
            print(tag, "image", i, "kept", len(pred), "conf", conf)
        assert sum(len(t) for t in dets) >= 5, tag
        _save(tag + ".npz", d)


if __name__ == "__main__":
    which = sys.argv[1:] or ["structure", "resnet", "val", "v8"]
    if "structure" in which:
        structure()
    if "resnet" in which:
        resnet_files()
    if "val" in which:
        val_case()
    if "v8" in which:
        v8_files()
