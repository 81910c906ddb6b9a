"""-m gpu: YOLOv12 -- grouped convs on the MFMA implicit GEMM (bit-exact against fp64 on dyadic data), AAttn / ABlock / A2C2f and
whole yolov12n / yolov12l against the reference goldens (tests/golden/make_golden_v12.py) in fp32, f16 against the fp32 path,
predict() with hipGraph capture, predict_batches, and the kernels a 32 x 640^2 f16 forward launches."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import synthdata as synth  # noqa: E402
from gpu_util import _traced  # noqa: E402

GAIN = 0.5  # the synthetic-weight gain of tests/golden/make_golden_v12.py (why: see there)


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


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("c1,c2,g,hw", [(16, 32, 2, (33, 47)), (64, 64, 4, (20, 18)), (32, 64, 4, (9, 7)), (128, 128, 2, (16, 16))])
def test_grouped_conv_exact(E, dtype, c1, c2, g, hw):
    """Conv(c1, c2, 3, 2, 1, g) on dyadic weights and inputs: every sum is exact in fp32 and the result representable in f16, so the MFMA
    kernel must equal fp64 bit for bit; and it must be an MFMA conv, not conv_direct."""
    from edge_yolo_amd.nn.modules import Conv
    gen = torch.Generator().manual_seed(c1 * 131 + c2 * 7 + g)
    m = Conv(c1, c2, 3, 2, 1, g, act=False)
    del m.bn  # no BatchNorm: the folded weights are the dyadic weights
    m.conv.weight.data = torch.randint(-4, 5, m.conv.weight.shape, generator=gen).float() / 16
    x = torch.randint(-8, 9, (2, c1, *hw), generator=gen).float() / 8
    want = torch.nn.functional.conv2d(x.double(), m.conv.weight.double(), None, 2, 1, 1, g)
    m = m.to("cuda").to(dtype)
    got, labels = _traced(lambda: m(x.to("cuda", dtype)))
    assert not any("conv_direct" in k for k in labels), labels
    assert len(labels) == 1 and labels[0].startswith("conv"), labels
    assert torch.equal(got.double().cpu(), want.to(dtype).double()), float((got.double().cpu() - want).abs().max())


def _module(cls, args, tag):
    m = cls(*args)
    m.load_state_dict({k: synth.synth_tensor(tag + "." + k, tuple(v.shape)) for k, v in m.state_dict().items()})
    for mm in m.modules():
        if isinstance(mm, torch.nn.BatchNorm2d):
            mm.eps = 1e-3
    return m.eval()


MODULES = [("aattn_a1", "AAttn", (64, 2, 1)), ("aattn_a4", "AAttn", (64, 2, 4)), ("aattn_a1_big", "AAttn", (32, 1, 1)),
           ("aattn_a4_h4", "AAttn", (128, 4, 4)), ("ablock_a4", "ABlock", (64, 2, 1.2, 4)), ("a2c2f_a2", "A2C2f", (64, 64, 1, True, 4)),
           ("a2c2f_c3k", "A2C2f", (64, 64, 2, False, -1)), ("a2c2f_res", "A2C2f", (64, 64, 1, True, 1, True, 1.5))]


@pytest.mark.parametrize("tag,cls,args", MODULES)
def test_modules_fp32_vs_reference_golden(E, golden_dir, tag, cls, args):
    from edge_yolo_amd.nn import modules
    g = np.load(os.path.join(golden_dir, "v12_ops.npz"))
    m = _module(getattr(modules, cls), args, tag).to("cuda").float()
    y = m(torch.from_numpy(g[tag + "_x"]).cuda())
    np.testing.assert_allclose(y.float().cpu().numpy(), g[tag], rtol=1e-4, atol=2e-4, err_msg=tag)


@pytest.mark.parametrize("name,tag,hw,first", [("yolov12n.yaml", "yolov12n_64x96", (64, 96), 0), ("yolov12l.yaml", "yolov12l_64", (64, 64), 5)])
def test_layers_vs_reference_golden(E, golden_dir, name, tag, hw, first):
    """Each layer runs on the reference's captured inputs (the goldens of the layers it reads), so a layer's error is its own: the
    attention layers amplify fp32 rounding differences of their inputs through exp()."""
    g = np.load(os.path.join(golden_dir, tag + ".npz"))
    from edge_yolo_amd.nn import _ops
    m = _build(name, torch.float32)
    gin = lambda j: torch.from_numpy(g[f"layer{j}"]).cuda()  # noqa: E731
    x = synth.synth_images(1, *hw).cuda()
    for layer in m.model[first:-1]:
        i = layer.i
        if i > 0:
            x = gin(i - 1 if layer.f == -1 else layer.f) if isinstance(layer.f, int) else [gin(i - 1 if j == -1 else j) for j in layer.f]
        t = _ops.as_tensor(layer(x))
        np.testing.assert_allclose(t.float().cpu().numpy(), g[f"layer{i}"], rtol=1e-4, atol=2e-4, err_msg=f"layer {i} {layer.type}")
    if first == 0:
        yy, _ = m(synth.synth_images(1, *hw).cuda())
        np.testing.assert_allclose(yy.cpu().numpy(), g["y"], rtol=1e-4, atol=1e-3)


@pytest.mark.parametrize("name,tag,hw", [("yolov12n.yaml", "yolov12n_96x160", (96, 160)), ("yolov12l.yaml", "yolov12l_64", (64, 64))])
def test_models_fp32_vs_reference_golden(E, golden_dir, name, tag, hw):
    g = np.load(os.path.join(golden_dir, tag + ".npz"))
    m = _build(name, torch.float32)
    y, raw = m(synth.synth_images(1, *hw).cuda())
    np.testing.assert_allclose(y.cpu().numpy(), g["y"], rtol=1e-4, atol=1e-3)
    for i, r in enumerate(raw):
        np.testing.assert_allclose(r.float().cpu().numpy(), g[f"raw{i}"], rtol=1e-4, atol=2e-4)


@pytest.mark.parametrize("name", ["yolov12n.yaml", "yolov12l.yaml"])
def test_fp16_vs_fp32(E, name):
    """Throughput mode, the model-level f16 bounds of test_gpu_model.py: scores within 2e-2, boxes within 1.5 % of the image size,
    against the fp32 path (pinned to the reference by the tests above)."""
    x = synth.synth_images(2, 320, 320).cuda()
    want, _ = _build(name, torch.float32)(x)
    y, _ = _build(name, torch.float16)(x.half())
    assert y.dtype == torch.float32
    assert float((y[:, 4:] - want[:, 4:]).abs().max()) < 2e-2
    assert float((y[:, :4] - want[:, :4]).abs().max()) < 0.015 * 320


def test_predict_graph_and_batches(E):
    model = E.YOLO("yolov12n.yaml")
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
    """The batch-32 640^2 f16 forward: grouped convs on MFMA (no conv_direct launch) and area attention only on the MFMA flash kernel."""
    m = _build("yolov12n.yaml", torch.float16)
    x = synth.synth_images(32, 640, 640).cuda().half()
    m(x)
    (y, _), labels = _traced(lambda: m(x))
    assert torch.isfinite(y).all()
    assert not any("conv_direct" in k for k in labels), sorted(set(labels))
    att = [k for k in labels if "area_attn" in k or "flash_attn" in k]
    assert att and set(att) == {"flash_attn_kernel<32>"}, sorted(set(labels))  # (the VALU kernel would show as area_attn_kernel)
    assert len(att) == 8  # layers 6 and 8: n = 2 R-ELAN units of 2 ABlocks each
