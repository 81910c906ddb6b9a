"""YOLO-World v2 without a GPU: structure, state_dict keys and parameter counts of the five scales against the reference
(tests/golden/structure_world.json), the C2fAttn parse rule, guess_model_task, the float64 restatements against the reference's outputs, the
fold of WorldDetect's class tail, set_classes and its checkpoint round trip, and the refusals.

The fold.  For a fixed vocabulary the class tail exp(logit_scale) <BatchNorm(W3 h + b3), normalize(w)> + bias is affine in the tower's hidden map
h; WorldDetect.folded_tail computes the (n x c3) weight and the bias in float64 and rounds them to fp32.  Applied in float64 to the reference's
own tower activations they must reproduce the reference's logits up to what the REFERENCE's fp32 evaluation and the fold's one rounding can
differ, counted operation by operation with u = 2^-24 (any summation order):
  x = W3 h + b3        c3 products and c3 sums:                    (c3 + 2) u (|W3| |h| + |b3|)
  z = BatchNorm(x)     A = g / sqrt(var + eps), z = (x - mean) A + b:  |A| d_x + 6 u (|A| (|x| + |mean|) + |b|)
  w^ = w / |w|         a 512-term sum of squares, sqrt, division:  260 u |w^|
  dot = w^ . z         512 products and sums:                      |w^| d_z + (260 + 513) u |w^| |z|
  logit = s dot + bias exp, product, sum:                          s d_dot + 4 u |s dot| + u |logit|
  fold                 weight and bias rounded once to fp32:       u (|Wf| |h| + |bf|)
Derived from the operation count, not fitted to the result (the achieved error is printed next to it)."""
import json
import os

import numpy as np
import pytest
import torch

import fp64_world_ref as f64
import world_synth as ws

U = 2.0 ** -24


@pytest.fixture(scope="module")
def structure(golden_dir):
    with open(os.path.join(golden_dir, "structure_world.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def ops_golden(golden_dir):
    return np.load(os.path.join(golden_dir, "world_ops.npz"))


@pytest.mark.parametrize("scale", list(ws.SCALES))
def test_structure_keys_and_parse_rule(structure, scale):
    from edge_yolo_amd.nn.modules import C2fAttn, WorldDetect
    from edge_yolo_amd.nn.tasks import WorldModel
    name = ws.NAME.format(scale)
    want = structure[name]
    m = WorldModel(name, nc=80)
    assert sum(p.numel() for p in m.parameters()) == want["params"]
    if scale == "n":
        assert want["params"] == ws.N_PARAMS
    assert list(m.save) == want["save"] and [float(s) for s in m.stride] == want["stride"]
    assert [dict(i=l.i, f=l.f, type=l.type, np=int(l.np)) for l in m.model] == want["layers"]
    keys = list(m.state_dict())
    assert keys[0] == "txt_feats" and keys[1:] == want["keys"]  # the text travels in state_dict; everything else is the reference's list
    attn = [dict(i=l.i, nh=l.attn.nh, hc=l.attn.hc, ec=l.attn.ec is not None, c=l.c) for l in m.model if isinstance(l, C2fAttn)]
    assert attn == want["attn"] and len(attn) == 4
    assert all(a["hc"] == 32 and not a["ec"] and a["c"] == 32 * a["nh"] for a in attn)  # the parse rule: head width 32, no embed conv
    assert isinstance(m.model[-1], WorldDetect) and tuple(m.txt_feats.shape) == (1, 80, 512)
    assert torch.equal(m.txt_feats, WorldModel(name, nc=80).txt_feats)  # seeded, not the global generator


def test_guess_model_task():
    from edge_yolo_amd.nn.tasks import WorldModel, guess_model_task, yaml_model_load
    assert guess_model_task("yolov8n-worldv2.yaml") == "detect"
    assert guess_model_task(yaml_model_load("yolov8s-worldv2.yaml")) == "detect"
    assert guess_model_task(WorldModel("yolov8n-worldv2.yaml")) == "detect"


@pytest.mark.parametrize("tag,kw,shape,n", ws.ATTN_CASES, ids=[c[0] for c in ws.ATTN_CASES])
def test_attention_restatement_against_the_reference(ops_golden, tag, kw, shape, n):
    """The float64 restatement on the reference's own proj_conv output and projected guide reproduces its fp32 output to fp32 accuracy, and
    the module here (CPU side: parameters and the cached guide only) projects the same guide."""
    from edge_yolo_amd.nn.modules import MaxSigmoidAttnBlock
    g = ops_golden
    m = MaxSigmoidAttnBlock(**kw)
    sd = ws.state_dict(m.state_dict(), prefix=tag + ".")
    m.load_state_dict(sd)
    assert list(m.state_dict()) == list(sd) and ("scale" in sd) == bool(kw["scale"])
    x = ws.case_input(tag, shape)
    scale = m.scale.detach().flatten().numpy() if torch.is_tensor(m.scale) else None
    y64, _ = f64.max_sigmoid_attn64(x.numpy(), g[tag + "_p"], g[tag + "_g"], m.bias.detach().numpy(), scale)
    err = float(np.abs(y64 - g[tag + "_y"]).max())
    assert err == float(g[tag + "_E"]) and err < 64 * U * max(1.0, float(np.abs(g[tag + "_y"]).max()))
    m.set_text(ws.normalized(ws.text(tag, n)))
    guide, bias, sc = m.guide(torch.float32, torch.device("cpu"))
    np.testing.assert_allclose(guide.numpy(), g[tag + "_g"][:1], rtol=1e-5, atol=1e-6)
    assert m.guide(torch.float32, torch.device("cpu"))[0] is guide  # cached: not recomputed per forward
    m.set_text(ws.normalized(ws.text(tag + "x", n)))
    assert m.guide(torch.float32, torch.device("cpu"))[0] is not guide  # and dropped with the vocabulary


def _head(tag, kw, n):
    from edge_yolo_amd.nn.modules import WorldDetect
    WorldDetect.legacy = True
    m = WorldDetect(**kw)
    m.load_state_dict(ws.state_dict(m.state_dict(), prefix=tag + "."))
    m.set_text(ws.text(tag, n)[None])
    return m.eval()


def test_fold_reproduces_the_reference_logits(ops_golden):
    g = ops_golden
    tag, kw, shapes, n = ws.HEAD_CASE
    m = _head(tag, kw, n)
    assert m.nc == n and m.no == n + 64 and list(m.state_dict()) == list(g[tag + "_keys"])
    d = lambda t: t.detach().double().numpy()  # noqa: E731
    txt = d(ws.text(tag, n))
    for i in range(len(shapes)):
        h = g[f"{tag}_h{i}"].astype(np.float64)
        want = g[f"{tag}_raw{i}"][:, 64:].astype(np.float64)
        w, b = m.folded_tail(i)
        assert w.dtype == torch.float32 and tuple(w.shape) == (n, h.shape[1], 1, 1) and tuple(b.shape) == (n,)
        got = f64.apply_fold64(h, d(w), d(b))
        # the bound of the module docstring
        conv, bn, hd = m.cv3[i][2], m.cv4[i].norm, m.cv4[i]
        w3, b3 = d(conv.weight).reshape(conv.out_channels, -1), d(conv.bias)
        c3 = w3.shape[1]
        ein = lambda a, t: np.einsum("oc,bchw->bohw", a, t)  # noqa: E731
        col = lambda v: v[None, :, None, None]  # noqa: E731
        x = ein(w3, h) + col(b3)
        d_x = (c3 + 2) * U * (ein(np.abs(w3), np.abs(h)) + col(np.abs(b3)))
        A = d(bn.weight) / np.sqrt(d(bn.running_var) + bn.eps)
        z = (x - col(d(bn.running_mean))) * col(A) + col(d(bn.bias))
        d_z = col(np.abs(A)) * d_x + 6 * U * (col(np.abs(A)) * (np.abs(x) + col(np.abs(d(bn.running_mean)))) + col(np.abs(d(bn.bias))))
        wn = txt / np.linalg.norm(txt, axis=-1, keepdims=True)
        dot = ein(wn, z)
        d_dot = ein(np.abs(wn), d_z) + (260 + 513) * U * ein(np.abs(wn), np.abs(z))
        s, beta = float(np.exp(d(hd.logit_scale))), float(d(hd.bias)[0])
        logit = s * dot + beta
        d_logit = s * d_dot + 4 * U * np.abs(s * dot) + U * np.abs(logit)
        bound = d_logit + U * (ein(np.abs(d(w)).reshape(n, -1), np.abs(h)) + col(np.abs(d(b))))
        r = float((np.abs(got - want) / bound).max())
        print(f"{tag} level {i}: fold vs reference max err {float(np.abs(got - want).max()):.3e}, max err/bound {r:.3f}, reference fp32 error E {float(g[tag + '_E']):.3e}")
        assert r <= 1.0
        np.testing.assert_allclose(logit, want, rtol=0, atol=float(np.abs(d_logit).max()))  # (the unfolded restatement agrees too)


def test_set_classes_and_checkpoint_round_trip(tmp_path):
    import edge_yolo_amd
    y = edge_yolo_amd.YOLOWorld("yolov8n-worldv2.yaml")
    head = y.model.model[-1]
    assert head.nc == 80 and len(y.names) == 80
    head.folded_tail(0)
    attn = [m.attn for m in y.model.model if type(m).__name__ == "C2fAttn"]
    guide0 = attn[0].guide(torch.float32, torch.device("cpu"))[0]
    t = ws.text("ckpt", 4)
    y.set_classes(["cat", " ", "dog", "bird"], t)
    assert y.names == {0: "cat", 1: "dog", 2: "bird"} and y.model.names == y.names  # the background entry keeps its embedding, not its name
    assert head.nc == 4 and head.no == 68 and tuple(y.model.txt_feats.shape) == (1, 4, 512)
    np.testing.assert_allclose(y.model.txt_feats.norm(dim=-1).numpy(), 1.0, rtol=1e-6)
    assert torch.equal(y.model.txt_feats, ws.normalized(t))
    assert tuple(head.folded_tail(0)[0].shape)[0] == 4 and head._tails == {}  # caches dropped
    guide1 = attn[0].guide(torch.float32, torch.device("cpu"))[0]
    assert guide1 is not guide0 and tuple(guide1.shape) == (1, 4, attn[0].nh * 32)
    y.set_classes(["a", "b", "c", "d"], t[None])  # (1, n, 512) is accepted too
    assert torch.equal(y.model.txt_feats, ws.normalized(t))
    y.set_classes(["cat", " ", "dog", "bird"], t)
    path = str(tmp_path / "world.pt")
    y.save(path)
    ck = torch.load(path, map_location="cpu", weights_only=True)
    assert ck["names"] == ["cat", "dog", "bird"] and "txt_feats" in ck["state_dict"]
    z = edge_yolo_amd.YOLOWorld(path)
    assert z.names == y.names and z.model.model[-1].nc == 4 and torch.equal(z.model.txt_feats, y.model.txt_feats)
    for (k, a), (k2, b) in zip(y.model.state_dict().items(), z.model.state_dict().items()):
        assert k == k2 and torch.equal(a, b), k
    for i in range(3):
        assert torch.equal(z.model.model[-1].folded_tail(i)[0], head.folded_tail(i)[0])
    # checkpoints of other models keep their exact content
    plain = edge_yolo_amd.YOLO("yolo11n.yaml")
    plain.save(str(tmp_path / "plain.pt"))
    assert sorted(torch.load(str(tmp_path / "plain.pt"), map_location="cpu", weights_only=True)) == ["fused", "nc", "state_dict", "yaml"]


class WorldModel(torch.nn.Module):
    """Stand-in for the pickled reference WorldModel inside a training checkpoint (the pattern of tests/test_host_cpu.py): the `yaml` dict,
    the state_dict under its dotted keys, and the plain attributes `txt_feats` and `names`.  The export tool looks at the class name."""

    def __init__(self, yaml, sd, txt_feats, names):
        super().__init__()
        self.yaml, self.txt_feats, self.names = yaml, txt_feats, names
        for k, v in sd.items():
            *path, leaf = k.split(".")
            mod = self
            for p in path:
                if p not in mod._modules:
                    mod.add_module(p, torch.nn.Module())
                mod = mod._modules[p]
            mod.register_buffer(leaf, v)


def test_reference_checkpoint_bridge_carries_text_and_names(tmp_path, structure):
    import sys
    import edge_yolo_amd
    from edge_yolo_amd.nn.tasks import yaml_model_load
    own = edge_yolo_amd.YOLOWorld("yolov8n-worldv2.yaml").model.state_dict()
    sd = ws.state_dict(own)
    assert list(sd) == structure[ws.NAME.format("n")]["keys"]  # what the reference's WorldModel holds: no text among them
    txt = ws.normalized(ws.text("bridge", 3))
    stub = WorldModel(dict(yaml_model_load("yolov8n-worldv2.yaml")), sd, txt, {0: "cat", 1: "dog", 2: "bird"})
    ref_pt, out_pt = str(tmp_path / "ref_world.pt"), str(tmp_path / "bridge_world.pt")
    torch.save({"epoch": 3, "model": None, "ema": stub, "train_args": {}}, ref_pt)
    tools = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
    sys.path.insert(0, tools)
    try:
        import export_reference_weights as ex
    finally:
        sys.path.remove(tools)
    assert ex.export(ref_pt, out_pt) == (len(sd) + 1, False)
    ck = torch.load(out_pt, weights_only=True)
    assert ck["names"] == ["cat", "dog", "bird"] and ck["nc"] == 80 and tuple(ck["state_dict"]["txt_feats"].shape) == (1, 3, 512)
    y = edge_yolo_amd.YOLOWorld(out_pt)
    assert y.names == {0: "cat", 1: "dog", 2: "bird"} and y.model.model[-1].nc == 3 and torch.equal(y.model.txt_feats, txt)
    got = y.model.state_dict()
    assert all(torch.equal(got[k], v) for k, v in sd.items())


def test_refusals():
    import edge_yolo_amd
    from edge_yolo_amd.nn.modules import C2fAttn, MaxSigmoidAttnBlock, WorldDetect
    y = edge_yolo_amd.YOLOWorld("yolov8n-worldv2.yaml")
    with pytest.raises(NotImplementedError, match="text encoder"):
        y.set_classes(["cat", "dog"])
    with pytest.raises(NotImplementedError, match="text encoder"):
        y.model.set_classes(["cat", "dog"])
    with pytest.raises(NotImplementedError, match="with_bn=False"):
        WorldDetect(80, 512, False, ch=(64, 128, 256))
    with pytest.raises(NotImplementedError, match="c1=64 != ec=128"):
        MaxSigmoidAttnBlock(64, 64, nh=2, ec=128)
    with pytest.raises(NotImplementedError, match="hc=16"):
        MaxSigmoidAttnBlock(64, 64, nh=4, ec=64)
    with pytest.raises(NotImplementedError, match="hc=64"):
        C2fAttn(64, 128, 1, ec=64, nh=1)
    with pytest.raises(NotImplementedError, match="per-image"):
        y.set_classes(["cat", "dog"], torch.zeros(3, 2, 512))
    with pytest.raises(NotImplementedError, match="per-image"):
        y.model.predict(torch.zeros(3, 3, 64, 64), txt_feats=torch.zeros(3, 80, 512))
    limit = WorldDetect.max_vocab
    with pytest.raises(NotImplementedError, match=str(limit)):
        y.set_classes([f"c{i}" for i in range(limit + 1)], ws.text("big", limit + 1))
    with pytest.raises(ValueError):
        y.set_classes(["cat", "dog"], torch.zeros(3, 512))
    with pytest.raises(NotImplementedError, match="vocabulary"):
        y.predict_batches([torch.zeros(1, 3, 64, 64)])


def test_yolo_task_map_and_registry_refusal_unchanged():
    import edge_yolo_amd
    from edge_yolo_amd.engine.predictor import DetectionPredictor
    from edge_yolo_amd.engine.validator import DetectionValidator
    from edge_yolo_amd.nn.tasks import DetectionModel, WorldModel, parse_model, yaml_model_load
    assert sorted(edge_yolo_amd.YOLO("yolo11n.yaml").task_map) == ["detect", "segment"]
    assert edge_yolo_amd.YOLO("yolo11n.yaml").task_map["detect"]["model"] is DetectionModel
    w = edge_yolo_amd.YOLOWorld("yolov8n-worldv2.yaml")
    assert w.task_map == {"detect": {"model": WorldModel, "predictor": DetectionPredictor, "validator": DetectionValidator}}
    d = yaml_model_load("yolov8n-worldv2.yaml")
    d["head"] = [list(r) for r in d["head"]]
    d["head"].insert(-1, [[15, 18, 21], 1, "ImagePoolingAttn", [256]])
    with pytest.raises(NotImplementedError, match="ImagePoolingAttn"):
        parse_model(d, 3)
