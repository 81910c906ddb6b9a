"""-m gpu: YOLOv13-LGL -- LocalAgg / SelfAttn / LGLBlock / _DSUnitWithLGL / DSC3K2_LGL and whole yolov13n-LGL / yolov13l-LGL against the
reference goldens (tests/golden/make_golden_v13_lgl.py) in fp32 at the bars of test_gpu_yolov13.py, f16 against the fp32 path,
predict() with hipGraph capture, predict_batches, the kernels of a 640^2 f16 forward and a 1280^2 forward (25 600 tokens in layer 2)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import lgl_synth  # noqa: E402
import synthdata as synth  # noqa: E402

NAME = "yolov13{}-DSC3K2_LGL.yaml"


@pytest.fixture(scope="module")
def E():
    import edge_yolo_amd
    return edge_yolo_amd


def _build(name, dtype):
    from edge_yolo_amd.nn.tasks import DetectionModel
    m = DetectionModel(name)
    m.load_state_dict(lgl_synth.state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}))
    m = m.to("cuda")
    m.fuse()
    m = m.half() if dtype == torch.float16 else m.float()
    return m.eval()


@pytest.fixture(scope="module")
def ops_golden(golden_dir):
    return np.load(os.path.join(golden_dir, "v13_lgl_ops.npz"))


@pytest.mark.parametrize("case", lgl_synth.CASES, ids=[c[0] for c in lgl_synth.CASES])
def test_modules_fp32_vs_reference_golden(E, ops_golden, case):
    from edge_yolo_amd.nn.modules import block
    tag, prefix, cls, args, kw, shape, lgl = case
    m = lgl_synth.fill(getattr(block, cls)(*args, **kw), prefix, lgl).to("cuda").float()
    x = torch.from_numpy(ops_golden[tag + "_x"]).cuda()
    assert torch.equal(x.cpu(), lgl_synth.case_input(shape))
    y = m(x)
    np.testing.assert_allclose(y.float().cpu().numpy(), ops_golden[tag], rtol=1e-4, atol=2e-4, err_msg=tag)


@pytest.mark.parametrize("scale,tag,hw,first", [("n", "yolov13n_lgl_64x96", (64, 96), 0), ("l", "yolov13l_lgl_64", (64, 64), 5)])
def test_layers_vs_reference_golden(E, golden_dir, scale, tag, hw, first):
    """Each layer runs on the reference's captured inputs (the goldens of the layers it reads), so a layer's error is its own."""
    g = np.load(os.path.join(golden_dir, tag + ".npz"))
    from edge_yolo_amd.nn import _ops
    m = _build(NAME.format(scale), torch.float32)

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


@pytest.mark.parametrize("scale,tag,hw", [("n", "yolov13n_lgl_96x160", (96, 160)), ("l", "yolov13l_lgl_64", (64, 64))])
def test_models_fp32_vs_reference_golden(E, golden_dir, scale, tag, hw):
    g = np.load(os.path.join(golden_dir, tag + ".npz"))
    m = _build(NAME.format(scale), torch.float32)
    y, raw = m(synth.synth_images(1, *hw).cuda())
    np.testing.assert_allclose(y.cpu().numpy(), g["y"], rtol=1e-4, atol=1e-3)
    for i, r in enumerate(raw):
        np.testing.assert_allclose(r.float().cpu().numpy(), g[f"raw{i}"], rtol=1e-4, atol=2e-4)


def test_fp16_vs_fp32(E):
    """Throughput mode under the model-level f16 bounds of test_gpu_model.py: scores within 2e-2, boxes within 1.5 % of the image side."""
    x = synth.synth_images(2, 320, 320).cuda()
    want, _ = _build(NAME.format("n"), torch.float32)(x)
    y, _ = _build(NAME.format("n"), torch.float16)(x.half())
    assert y.dtype == torch.float32
    es, eb = float((y[:, 4:] - want[:, 4:]).abs().max()), float((y[:, :4] - want[:, :4]).abs().max())
    print(f"yolov13n-LGL f16 vs fp32 at 320^2: scores {es:.3e} (bound 2e-2), boxes {eb:.3f} px (bound {0.015 * 320})")
    assert es < 2e-2
    assert eb < 0.015 * 320


def test_predict_graph_and_batches(E):
    model = E.YOLO(NAME.format("n"))
    model.model.load_state_dict(lgl_synth.state_dict({k: tuple(v.shape) for k, v in model.model.state_dict().items()}))
    x = synth.synth_images(2, 128, 160)
    r1 = model.predict(x, conf=0.25, iou=0.7, device="cuda:0", graph=False)
    r2 = model.predict(x, conf=0.25, iou=0.7, device="cuda:0", graph=True)
    r3 = model.predict(x, conf=0.25, iou=0.7, device="cuda:0", graph=True)  # replay
    for a, b, c in zip(r1, r2, r3):
        assert torch.equal(a.boxes.data.cpu(), b.boxes.data.cpu()) and torch.equal(a.boxes.data.cpu(), c.boxes.data.cpu())
    xs = [torch.rand(2, 3, 128, 160, generator=torch.Generator().manual_seed(i)) for i in range(4)]
    outs = list(model.predict_batches(xs, conf=0.25, half=True))
    assert len(outs) == len(xs)
    for xi, res in zip(xs, outs):
        ref = model.predict(xi, conf=0.25, half=True)
        for a, b in zip(res, ref):
            assert torch.equal(a.boxes.data.cpu(), b.boxes.data.cpu())


def test_640_b2_f16_kernels(E):
    """A batch-2 640^2 f16 forward: no conv_direct launch, no VALU attention; one flash launch per LGL unit (six), the head_dim-16 kernel
    (6400 tokens in layer 2) among them; the eight area-attention launches of the A2C2f layers run flash_attn_kernel<32> too."""
    from edge_yolo_amd import profiling
    m = _build(NAME.format("n"), torch.float16)
    x = synth.synth_images(2, 640, 640).cuda().half()
    m(x)
    with profiling.trace() as t:
        y, _ = m(x)
    torch.cuda.synchronize()
    labels = [r[0] for r in t.records]
    attn = [(r[0], r[5]) for r in t.records if "area_attn" in r[0] or "flash_attn" in r[0]]  # (kernel, trace note): area_attention's note names its area count
    assert torch.isfinite(y).all()
    assert not any("conv_direct" in k for k in labels), sorted(set(labels))
    flash = [k for k, note in attn if " area" not in note]  # the LGL units
    assert sorted(flash) == sorted(["flash_attn_kernel<16>", "flash_attn_kernel<32>", "flash_attn_kernel<64>", "flash_attn_kernel<32>",
                                    "flash_attn_kernel<64>", "flash_attn_kernel<64>"]), flash
    assert [k for k, note in attn if " area" in note] == ["flash_attn_kernel<32>"] * 8, attn  # the A2C2f layers
    assert labels.count("area_attn_kernel") == 0  # the VALU kernel
    assert labels.count("lgl_cmlp_kernel") == 6 and labels.count("lgl_unpool_ln_kernel") == 6 and labels.count("lgl_dw_kernel<9>") == 12


def test_1280_f16_is_finite(E):
    """Layer 2 attends 25 600 tokens at 1280^2: beyond the VALU kernel's LDS limit, any N for the flash kernel."""
    m = _build(NAME.format("n"), torch.float16)
    y, _ = m(synth.synth_images(1, 1280, 1280).cuda().half())
    assert torch.isfinite(y).all()
