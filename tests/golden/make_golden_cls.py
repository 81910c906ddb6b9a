"""Golden vectors for the classify task: the Classify head (reference ultralytics/nn/modules/head.py:454-476), its parse rule and
ClassificationModel (nn/tasks.py:457-500), linear + softmax with the reference's own fp32 error, the Probs container (engine/results.py:
1378-1516), Pillow's resize + crop for the image transform (data/augment.py:2346 classify_transforms; torchvision itself is not installed
where this runs, so the two size rules are restated from its documentation) and an end-to-end case run through the reference's own
ClassificationValidator.update_metrics / ClassifyMetrics.process, from the real reference imported through _ref_import.  CPU fp32, synthetic
weights and inputs (tests/cls_synth.py).

    python tests/golden/make_golden_cls.py

writes structure_cls.json, cls_ops.npz, yolo11n_cls_64.npz and clsval_case.npz.  Asserted here: in every top-k case the first six
probabilities of every row differ by more than the case's bound (so the ranking does not depend on rounding), and the float64 transform is
within 1.0 + 2^-8 grey levels of Pillow on every transform case.  Runs only where the reference exists.
"""
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
import yaml  # noqa: E402
from PIL import Image  # noqa: E402

import cls_synth  # noqa: E402
import fp64_cls_ref as f64  # noqa: E402

from ultralytics.engine.results import Probs as RefProbs  # noqa: E402
from ultralytics.models.yolo.classify.val import ClassificationValidator as RCV  # noqa: E402
from ultralytics.nn.modules.head import Classify  # noqa: E402
from ultralytics.nn.tasks import ClassificationModel, guess_model_task  # noqa: E402
from ultralytics.utils import metrics as rm  # noqa: E402

torch.set_grad_enabled(False)
ClassificationModel.info = lambda self, *a, **k: None  # (the summary line needs thop, which _ref_import replaces by an inert stand-in)
CFG = os.path.join(ROOT, "edge-yolo_amd", "cfg", "models", "11")


def cfg(scale, name="yolo11-cls.yaml"):
    d = yaml.safe_load(open(os.path.join(CFG, name), encoding="utf-8"))
    d["scale"] = scale
    return d


def _save(name, d):
    path = os.path.join(HERE, name)
    np.savez_compressed(path, **{k: (v.numpy() if torch.is_tensor(v) else v) for k, v in d.items()})
    size = os.path.getsize(path)
    print(name, len(d), size)
    assert size < 1 << 20, name


def structure():
    out = {}
    for sc in cls_synth.SCALES:
        d = cfg(sc)
        assert guess_model_task(d) == "classify"
        m = ClassificationModel(d, ch=3, nc=1000, verbose=False)
        assert guess_model_task(m) == "classify"
        out[cls_synth.NAME.format(sc)] = dict(params=sum(p.numel() for p in m.parameters()), save=list(m.save), stride=[float(s) for s in m.stride],
                                              layers=[dict(i=l.i, f=l.f, type=l.type, np=int(l.np)) for l in m.model], keys=list(m.state_dict()),
                                              params_nc3=sum(p.numel() for p in ClassificationModel(cfg(sc), ch=3, nc=3, verbose=False).parameters()))
        print(sc, out[cls_synth.NAME.format(sc)]["params"])
    with open(os.path.join(HERE, "structure_cls.json"), "w") as f:
        f.write("{\n" + ",\n".join(json.dumps(k) + ": " + json.dumps(v, separators=(",", ":")) for k, v in out.items()) + "\n}\n")
    assert os.path.getsize(os.path.join(HERE, "structure_cls.json")) < 1 << 20


def _gap6(p64, n=6):
    """smallest difference between neighbours among the six largest probabilities of every row (float64)."""
    s = -np.sort(-p64, axis=1)[:, :n]
    return np.abs(np.diff(s, axis=1)).min(1) if s.shape[1] > 1 else np.full(len(s), np.inf)


def ops_file():
    d = {}
    # the Classify head on a small map
    tag, c1, c2, shape = cls_synth.HEAD_CASE
    m = Classify(c1, c2).eval()
    m.load_state_dict(cls_synth.state_dict(m.state_dict(), prefix=tag + "."))
    y, x = m(cls_synth.case_input(tag, shape))
    d[tag + "_probs"], d[tag + "_logits"] = y, x
    d[tag + "_keys"] = np.array(list(m.state_dict()))
    assert isinstance(m([cls_synth.case_input(tag, shape)[:, :32], cls_synth.case_input(tag, shape)[:, 32:]]), tuple)  # a list is concatenated
    # linear + softmax + the ranking, with the reference's own fp32 error E
    for tag, (B, nc, half, kind) in cls_synth.LINEAR_CASES.items():
        pooled, w, b = cls_synth.linear_case(tag)
        logits = torch.nn.functional.linear(torch.tensor(pooled), torch.tensor(w), torch.tensor(b))
        probs = logits.softmax(1)
        assert logits.dtype == probs.dtype == torch.float32 and torch.isfinite(probs).all()
        l64, p64 = f64.linear_softmax64(pooled, w, b)
        El, Ep = float(np.abs(logits.numpy() - l64).max()), float(np.abs(probs.numpy() - p64).max())
        d[tag + "_El"], d[tag + "_Ep"] = np.float64(El), np.float64(Ep)
        n5 = min(nc, 5)
        top = probs.argsort(1, descending=True)[:, :n5].type(torch.int32)  # ClassificationValidator.update_metrics (classify/val.py:58-59)
        d[tag + "_top"] = top
        # both neighbours may move by the bound: the gap must exceed twice it.  The +-80 case has one class near 1 and the rest near 0: only
        # its winner is separable (and only its winner is compared)
        nsep = 2 if kind == "big" else 6
        gap = _gap6(p64, nsep)
        s = -np.sort(-p64, axis=1)[:, :nsep]
        assert (gap > 2 * f64.bound(Ep, s).max(1)).all(), (tag, float(gap.min()))
        assert np.array_equal(top.numpy()[:, :nsep - 1], f64.rank(p64)[:, :nsep - 1]), tag
        if tag in cls_synth.LINEAR_FULL:
            d[tag + "_logits"], d[tag + "_probs"] = logits, probs
        print(tag, f"E logits {El:.2e} probs {Ep:.2e} gap {float(gap.min()):.2e} max |logit| {float(np.abs(l64).max()):.1f}")
    assert float(np.abs(f64.linear_softmax64(*cls_synth.linear_case("ls_big_nc80_b3"))[0]).max()) > 60
    # Probs (engine/results.py:1378-1516) on a row of the nc = 80 case, and on one with fewer than five classes
    p = torch.tensor(d["ls_nc80_b1_probs"].numpy()[0])
    for name, row in (("probs80", p), ("probs2", torch.tensor(d["ls_nc2_b1_probs"].numpy()[0]))):
        r = RefProbs(row)
        d[name + "_data"], d[name + "_top1"], d[name + "_top5"] = r.data, np.int64(r.top1), np.array(r.top5)
        d[name + "_top1conf"], d[name + "_top5conf"] = r.top1conf, r.top5conf
        rn = r.numpy()
        assert rn.top5 == r.top5 and isinstance(rn.data, np.ndarray)
    # the image transform: Pillow is the reference for the pixels, torchvision's two size rules are restated (cls_synth.resized / crop_origin)
    for tag, h, w, S in cls_synth.TRANSFORM_CASES:
        img = cls_synth.transform_image(tag, h, w)
        nh, nw = cls_synth.resized(h, w, S)
        t, l = cls_synth.crop_origin(nh, S), cls_synth.crop_origin(nw, S)
        pil = np.asarray(Image.fromarray(img).resize((nw, nh), Image.BILINEAR))[t:t + S, l:l + S]
        assert pil.shape == (S, S, 3)
        g64 = f64.transform(img, S)
        worst = float(np.abs(g64 - pil).max())
        assert worst <= 1.0 + 2.0 ** -8, (tag, worst)
        # E of the transform: the same expressions evaluated in fp32 (coefficients rounded to fp32, fp32 sums, fp32 division by 255)
        E = float(np.abs(f64.to_tensor(f64.transform(img, S, np.float32), np.float32).astype(np.float64) - f64.to_tensor(g64)).max())
        d[tag + "_pil"], d[tag + "_E"], d[tag + "_geom"] = pil, np.float64(E), np.array([nh, nw, t, l])
        print(tag, (nh, nw), (t, l), f"max |f64 - pillow| {worst:.4f} levels, fp32 E {E:.2e}")
    _save("cls_ops.npz", d)


def model_file():
    m = ClassificationModel(cfg("n"), ch=3, nc=80, verbose=False).eval()
    m.load_state_dict(cls_synth.state_dict(m.state_dict()))
    m.fuse(verbose=False)
    import synthdata as synth
    x = synth.synth_images(2, 64, 64)
    y, logits = m(x)
    assert torch.isfinite(y).all() and tuple(y.shape) == (2, 80)
    top = y.argsort(1, descending=True)[:, :5].type(torch.int32)
    gap = _gap6(y.numpy().astype(np.float64))
    print("yolo11n_cls_64 top5", top.tolist(), "top1conf", y.max(1).values.tolist(), f"gap {float(gap.min()):.2e}")
    d = {"probs": y, "logits": logits, "top5": top, "gap": gap}
    for i in range(2):
        r = RefProbs(y[i])
        d[f"p{i}_top1"], d[f"p{i}_top5"], d[f"p{i}_top1conf"], d[f"p{i}_top5conf"] = np.int64(r.top1), np.array(r.top5), r.top1conf, r.top5conf
    _save("yolo11n_cls_64.npz", d)


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


def _run(v, probs_list, cls_list):
    for p, c in zip(probs_list, cls_list):
        v.update_metrics(torch.as_tensor(p), {"cls": torch.as_tensor(c)})
    res = v.get_stats()
    return np.array(list(res.keys())), np.array([float(t) for t in res.values()]), torch.cat(v.pred).numpy()


def case_file():
    nc = cls_synth.VAL_NC
    m = ClassificationModel(cfg("n"), ch=3, nc=nc, verbose=False).eval()
    m.load_state_dict(cls_synth.state_dict(m.state_dict()))
    m.fuse(verbose=False)
    probs = [m(cls_synth.val_images(i))[0] for i in range(cls_synth.VAL_BATCHES)]
    allp = torch.cat(probs).numpy().astype(np.float64)
    gap = _gap6(allp)
    order = np.argsort(-allp, axis=1, kind="stable")
    # labels from the ranking: the winner, the runner-up, the fifth, the sixth (a top-5 miss), the last, ... over the images
    place = [0, 1, 4, 5, 0, nc - 1, 2, 0]
    cls = np.array([order[i, place[i % len(place)]] for i in range(len(allp))], np.int64)
    B = cls_synth.VAL_SHAPE[0]
    cls_list = [cls[i * B:(i + 1) * B] for i in range(cls_synth.VAL_BATCHES)]
    keys, values, pred = _run(_validator(nc), probs, cls_list)
    print("clsval", dict(zip(keys.tolist(), values.tolist())), f"gap {float(gap.min()):.2e}")
    assert 0 < values[0] < values[1] < 1
    d = dict(cls=cls, probs=torch.cat(probs), pred=pred, keys=keys, values=values, gap=gap, image_shape=np.array(cls_synth.VAL_SHAPE), nc=np.int64(nc))
    # the host bookkeeping alone, on random probability rows: nc = 10, and nc = 3 (n5 = 3)
    for tag, Bh, nch in (("host10", 16, 10), ("host3", 16, 3)):
        p = cls_synth.host_probs(tag, Bh, nch)
        r = np.random.default_rng([11, nch])
        c = np.where(r.random(Bh) < 0.4, p.argmax(1), r.integers(0, nch, Bh)).astype(np.int64)
        halves = [p[:Bh // 2], p[Bh // 2:]], [c[:Bh // 2], c[Bh // 2:]]
        k, vals, pr = _run(_validator(nch), *halves)
        assert pr.shape == (Bh, min(nch, 5))
        d[tag + "_cls"], d[tag + "_values"], d[tag + "_pred"] = c, vals, pr
        print(tag, vals.tolist())
    _save("clsval_case.npz", d)


if __name__ == "__main__":
    structure()
    ops_file()
    model_file()
    case_file()
