"""-m gpu: YOLOv13 -- HyperACE / C3AH / AdaHGConv / FuseModule / DownsampleConv / FullPAD_Tunnel / DSC3K2 / stride-2 DSConv and whole
yolov13n / yolov13l against the reference goldens (tests/golden/make_golden_v13.py) in fp32, f16 against the fp32 path, predict() with
hipGraph capture, predict_batches, and the kernels of a 32 x 640^2 f16 forward."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import synthdata as synth  # noqa: E402

GAIN = 0.5  # the synthetic-weight gain of tests/golden/make_golden_v13.py (why: see there)


@pytest.fixture(scope="module")
def E():
    import edge_yolo_amd
    return edge_yolo_amd


def _build(name, dtype, gain=GAIN):
    from edge_yolo_amd.nn.tasks import DetectionModel
    m = DetectionModel(name)
    m.load_state_dict(synth.synth_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, gain=gain))
    m = m.to("cuda")
    m.fuse()
    m = m.half() if dtype == torch.float16 else m.float()
    return m.eval()


MODULES = [("hgc_d64_e4", "AdaHGComputation", (64, 4, 4)), ("hgc_d128_e8", "AdaHGComputation", (128, 8, 8)),
           ("hgc_d64_e12", "AdaHGComputation", (64, 12, 4)), ("hgc_d128_e12_mean", "AdaHGComputation", (128, 12, 8, 0.1, "mean")),
           ("c3ah", "C3AH", (64, 64, 1.0, 8)), ("fuse_adj", "FuseModule", (32, True)), ("fuse_noadj", "FuseModule", (32, False)),
           ("hyperace_n1", "HyperACE", (32, 64, 1, 4, True, True, 0.5, 1, "both", True)),
           ("hyperace_n2", "HyperACE", (32, 64, 2, 8, True, True, 0.5, 1, "both", False)),
           ("hyperace_dsb", "HyperACE", (32, 64, 1, 4, False, False, 0.5, 1, "both", False)),
           ("down_adj", "DownsampleConv", (32, True)), ("down_noadj", "DownsampleConv", (32, False)), ("fullpad", "FullPAD_Tunnel", ()),
           ("dsconv_s2_even", "DSConv", (32, 64, 3, 2)), ("dsconv_s2_odd", "DSConv", (32, 48, 3, 2)), ("dsc3k2_dsb", "DSC3K2", (64, 64, 1, False)),
           ("dsc3k2_dsc3k", "DSC3K2", (64, 64, 1, True)), ("hgconv_tokens", "AdaHGConv", (64, 8, 4))]


@pytest.mark.parametrize("tag,cls,args", MODULES)
def test_modules_fp32_vs_reference_golden(E, golden_dir, tag, cls, args):
    from edge_yolo_amd.nn import modules
    g = np.load(os.path.join(golden_dir, "v13_ops.npz"))
    m = getattr(modules, cls)(*args)
    m.load_state_dict({k: synth.synth_tensor(tag + "." + k, tuple(v.shape), gain=GAIN) for k, v in m.state_dict().items()})
    for mm in m.modules():
        if isinstance(mm, torch.nn.BatchNorm2d):
            mm.eps = 1e-3
    m = m.eval().to("cuda").float()
    xs = [torch.from_numpy(g[f"{tag}_x{i}"]).cuda() for i in range(3) if f"{tag}_x{i}" in g]
    y = m(xs if len(xs) > 1 else xs[0])
    np.testing.assert_allclose(y.float().cpu().numpy(), g[tag], rtol=1e-4, atol=2e-4, err_msg=tag)


@pytest.mark.parametrize("name,tag,hw,first", [("yolov13n.yaml", "yolov13n_64x96", (64, 96), 0), ("yolov13l.yaml", "yolov13l_64", (64, 64), 5)])
def test_layers_vs_reference_golden(E, golden_dir, name, tag, hw, first):
    """Each layer runs on the reference's captured inputs (the goldens of the layers it reads), so a layer's error is its own."""
    g = np.load(os.path.join(golden_dir, tag + ".npz"))
    from edge_yolo_amd.nn import _ops
    m = _build(name, torch.float32)

    def gin(j):  # golden output of layer j; the l file leaves out Concat / Upsample outputs: rebuilt from their inputs
        if f"layer{j}" in g:
            return torch.from_numpy(g[f"layer{j}"]).cuda()
        src = m.model[j]
        fs = [src.f] if isinstance(src.f, int) else src.f
        ins = [gin(j - 1 if f == -1 else f) for f in fs]
        return torch.cat(ins, 1) if len(ins) > 1 else ins[0].repeat_interleave(2, 2).repeat_interleave(2, 3)

    x = synth.synth_images(1, *hw).cuda()
    for layer in m.model[first:-1]:
        i = layer.i
        if f"layer{i}" not in g:
            continue
        if i > 0:
            x = gin(i - 1 if layer.f == -1 else layer.f) if isinstance(layer.f, int) else [gin(i - 1 if j == -1 else j) for j in layer.f]
        t = _ops.as_tensor(layer(x))
        np.testing.assert_allclose(t.float().cpu().numpy(), g[f"layer{i}"], rtol=1e-4, atol=2e-4, err_msg=f"layer {i} {layer.type}")
    if first == 0:
        yy, _ = m(synth.synth_images(1, *hw).cuda())
        np.testing.assert_allclose(yy.cpu().numpy(), g["y"], rtol=1e-4, atol=1e-3)


@pytest.mark.parametrize("name,tag,hw", [("yolov13n.yaml", "yolov13n_96x160", (96, 160)), ("yolov13l.yaml", "yolov13l_64", (64, 64))])
def test_models_fp32_vs_reference_golden(E, golden_dir, name, tag, hw):
    g = np.load(os.path.join(golden_dir, tag + ".npz"))
    m = _build(name, torch.float32)
    y, raw = m(synth.synth_images(1, *hw).cuda())
    np.testing.assert_allclose(y.cpu().numpy(), g["y"], rtol=1e-4, atol=1e-3)
    for i, r in enumerate(raw):
        np.testing.assert_allclose(r.float().cpu().numpy(), g[f"raw{i}"], rtol=1e-4, atol=2e-4)


@pytest.mark.parametrize("name", ["yolov13n.yaml", "yolov13l.yaml"])
def test_fp16_vs_fp32(E, name):
    """Throughput mode, the model-level f16 bounds of test_gpu_model.py: scores within 2e-2, boxes within 1.5 % of the image size."""
    x = synth.synth_images(2, 320, 320).cuda()
    want, _ = _build(name, torch.float32)(x)
    y, _ = _build(name, torch.float16)(x.half())
    assert y.dtype == torch.float32
    assert float((y[:, 4:] - want[:, 4:]).abs().max()) < 2e-2
    assert float((y[:, :4] - want[:, :4]).abs().max()) < 0.015 * 320


def test_predict_graph_and_batches(E):
    model = E.YOLO("yolov13n.yaml")
    model.model.load_state_dict(synth.synth_state_dict({k: tuple(v.shape) for k, v in model.model.state_dict().items()}, gain=GAIN))
    x = synth.synth_images(2, 128, 160)
    r1 = model.predict(x, conf=0.25, iou=0.7, device="cuda:0", graph=False)
    r2 = model.predict(x, conf=0.25, iou=0.7, device="cuda:0", graph=True)
    r3 = model.predict(x, conf=0.25, iou=0.7, device="cuda:0", graph=True)  # replay
    for a, b, c in zip(r1, r2, r3):
        assert torch.equal(a.boxes.data.cpu(), b.boxes.data.cpu()) and torch.equal(a.boxes.data.cpu(), c.boxes.data.cpu())
    xs = [torch.rand(2, 3, 128, 160, generator=torch.Generator().manual_seed(i)) for i in range(6)]
    outs = list(model.predict_batches(xs, conf=0.25, half=True))
    assert len(outs) == len(xs)
    for xi, res in zip(xs, outs):
        ref = model.predict(xi, conf=0.25, half=True)
        for a, b in zip(res, ref):
            assert torch.equal(a.boxes.data.cpu(), b.boxes.data.cpu())


def test_640_b32_f16_kernels(E):
    """The batch-32 640^2 f16 forward: no conv_direct launch; the HyperACE stage runs two ey_hypergraph_conv calls of five kernels each,
    the stride-2 DSConvs their depthwise kernel, and the FullPAD tunnels the scale-add kernel."""
    from edge_yolo_amd import profiling
    m = _build("yolov13n.yaml", torch.float16)
    x = synth.synth_images(32, 640, 640).cuda().half()
    m(x)
    with profiling.trace() as t:
        y, _ = m(x)
    torch.cuda.synchronize()
    labels = [r[0] for r in t.records]
    assert torch.isfinite(y).all()
    assert not any("conv_direct" in k for k in labels), sorted(set(labels))
    hg = [r for r in t.records if r[0] == "hypergraph_kernels"]
    assert len(hg) == 2 and sum(r[6] for r in hg) == 10, hg
    assert labels.count("dwconv_s2_kernel<3>") == 2
    assert labels.count("scale_add_kernel") == 7
    assert labels.count("avgpool2_kernel") == 2
