"""-m gpu: DySample modules and whole yolov13n-DySample / yolov13l-DySample against the reference goldens
(tests/golden/make_golden_dysample.py) in fp32 at the bars of test_gpu_yolov13.py, f16 against the fp32 path, predict() with hipGraph
capture, predict_batches, save -> load -> predict, the kernels of a 640^2 f16 forward, and yolov13n.yaml unchanged beside it."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import dysample_synth  # noqa: E402
import synthdata as synth  # noqa: E402

NAME = dysample_synth.NAME


@pytest.fixture(scope="module")
def E():
    import edge_yolo_amd
    return edge_yolo_amd


def _build(name, dtype):
    from edge_yolo_amd.nn.tasks import DetectionModel
    m = DetectionModel(name)
    m.load_state_dict(dysample_synth.state_dict(m.state_dict()))
    m = m.to("cuda")
    m.fuse()
    m = m.half() if dtype == torch.float16 else m.float()
    return m.eval()


@pytest.fixture(scope="module")
def ops_golden(golden_dir):
    return np.load(os.path.join(golden_dir, "dysample_ops.npz"))


@pytest.mark.parametrize("case", dysample_synth.CASES, ids=[c[0] for c in dysample_synth.CASES])
def test_modules_fp32_vs_reference_golden(E, ops_golden, case):
    from edge_yolo_amd.nn.modules import DySample
    tag, args, shape = case
    m = dysample_synth.fill(DySample(*args), tag).to("cuda").float()
    x = torch.from_numpy(ops_golden[tag + "_x"]).cuda()
    assert torch.equal(x.cpu(), dysample_synth.case_input(shape))
    if not dysample_synth.kernel_supports(args):  # 4 channels per group: no kernel, and no fall-back either
        with pytest.raises(NotImplementedError, match="multiple of 8"):
            m(x)
        return
    y = m(x)
    np.testing.assert_allclose(y.float().cpu().numpy(), ops_golden[tag], rtol=1e-4, atol=2e-4, err_msg=tag)


def test_module_writes_into_a_concat_slot(E, ops_golden):
    """out= a channel window of a wider buffer (the slot of a concat): same values, the neighbours untouched."""
    from edge_yolo_amd import _lib as L
    from edge_yolo_amd.nn.modules import DySample
    tag, args, shape = dysample_synth.CASES[6]
    m = dysample_synth.fill(DySample(*args), tag).to("cuda").float()
    x = torch.from_numpy(ops_golden[tag + "_x"]).cuda()
    B, C, H, W = shape
    buf = L.empty_nhwc(B, C + 32, 2 * H, 2 * W, torch.float32, "cuda")
    buf.fill_(-7.0)
    y = m(x, out=buf[:, 16:16 + C])
    assert y.data_ptr() == buf[:, 16:16 + C].data_ptr()
    np.testing.assert_allclose(buf[:, 16:16 + C].cpu().numpy(), ops_golden[tag], rtol=1e-4, atol=2e-4)
    assert (buf[:, :16] == -7.0).all() and (buf[:, 16 + C:] == -7.0).all()


@pytest.mark.parametrize("scale,tag,base,hw,first", [("n", "yolov13n_dysample_64x96", "yolov13n_64x96", (64, 96), 10),
                                                     ("l", "yolov13l_dysample_64", "yolov13l_64", (64, 64), 10)])
def test_layers_vs_reference_golden(E, golden_dir, scale, tag, base, hw, first):
    """Each layer runs on the reference's captured inputs (the goldens of the layers it reads), so a layer's error is its own.  Layers
    0-9, 11, 12 and 14 are yolov13's with yolov13's weights: their goldens are those of `base` (make_golden_dysample.py checks that they
    repeat bit for bit and leaves them out), and test_gpu_yolov13.py already runs them; here they serve as inputs."""
    g, gb = np.load(os.path.join(golden_dir, tag + ".npz")), np.load(os.path.join(golden_dir, base + ".npz"))
    from edge_yolo_amd.nn import _ops
    m = _build(NAME.format(scale), torch.float32)

    def gin(j):  # golden output of layer j
        for f in (g, gb):
            if f"layer{j}" in f and (f is g or j in (4, 5, 6, 7, 8, 9, 11, 12, 14)):
                return torch.from_numpy(f[f"layer{j}"]).cuda()
        src = m.model[j]
        ins = [gin(j - 1 if f == -1 else f) for f in ([src.f] if isinstance(src.f, int) else src.f)]
        if type(src).__name__ == "Concat":  # left out of the l file: a copy of its inputs
            return torch.cat(ins, 1)
        assert type(src).__name__ == "FullPAD_Tunnel"  # layer 13 of the l file: x0 + gate * x1 of two stored maps, in float64
        return (ins[0].double() + float(src.gate.detach()) * ins[1].double()).float()

    seen = []
    for layer in m.model[first:-1]:
        i = layer.i
        if f"layer{i}" not in g:
            continue
        x = gin(i - 1 if layer.f == -1 else layer.f) if isinstance(layer.f, int) else [gin(i - 1 if j == -1 else j) for j in layer.f]
        t = _ops.as_tensor(layer(x))
        np.testing.assert_allclose(t.float().cpu().numpy(), g[f"layer{i}"], rtol=1e-4, atol=2e-4, err_msg=f"layer {i} {layer.type}")
        seen.append(i)
    assert set(dysample_synth.DYSAMPLE_LAYERS) <= set(seen)
    if scale == "n":
        yy, _ = m(synth.synth_images(1, *hw).cuda())
        np.testing.assert_allclose(yy.cpu().numpy(), g["y"], rtol=1e-4, atol=1e-3)


@pytest.mark.parametrize("scale,tag,hw", [("n", "yolov13n_dysample_96x160", (96, 160)), ("l", "yolov13l_dysample_64", (64, 64))])
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
    print(f"yolov13n-DySample f16 vs fp32 at 320^2: scores {es:.3e} (bound 2e-2), boxes {eb:.3f} px (bound {0.015 * 320})")
    assert es < 2e-2
    assert eb < 0.015 * 320


def test_predict_graph_batches_save_load(E, tmp_path):
    model = E.YOLO(NAME.format("n"))
    model.model.load_state_dict(dysample_synth.state_dict(model.model.state_dict()))
    x = synth.synth_images(2, 128, 160)
    r1 = model.predict(x, conf=0.25, iou=0.7, device="cuda:0", graph=False)
    r2 = model.predict(x, conf=0.25, iou=0.7, device="cuda:0", graph=True)
    r3 = model.predict(x, conf=0.25, iou=0.7, device="cuda:0", graph=True)  # replay
    assert sum(len(a.boxes.data) for a in r1) > 0
    for a, b, c in zip(r1, r2, r3):
        assert torch.equal(a.boxes.data.cpu(), b.boxes.data.cpu()) and torch.equal(a.boxes.data.cpu(), c.boxes.data.cpu())
    xs = [torch.rand(2, 3, 128, 160, generator=torch.Generator().manual_seed(i)) for i in range(4)]
    outs = list(model.predict_batches(xs, conf=0.25, half=True))
    assert len(outs) == len(xs)
    for xi, res in zip(xs, outs):
        ref = model.predict(xi, conf=0.25, half=True)
        for a, b in zip(res, ref):
            assert torch.equal(a.boxes.data.cpu(), b.boxes.data.cpu())
    f = str(tmp_path / "dysample.pt")
    model.save(f)
    again = E.YOLO(f)
    for i in dysample_synth.DYSAMPLE_LAYERS:
        assert type(again.model.model[i]).__name__ == "DySample" and again.model.model[i].init_pos.abs().eq(0.25).all()
    r4 = again.predict(x, conf=0.25, iou=0.7, device="cuda:0", graph=False)
    r5 = model.predict(x, conf=0.25, iou=0.7, device="cuda:0", graph=False)
    for a, b in zip(r4, r5):
        assert torch.equal(a.boxes.data.cpu(), b.boxes.data.cpu())


def test_640_f16_kernels(E):
    """A batch-2 640^2 f16 forward: one dysample launch per DySample layer on 128 / 256 / 128 channels at 40^2 / 20^2 / 40^2, no
    upsampling copy, no conv_direct launch."""
    from edge_yolo_amd import profiling
    m = _build(NAME.format("n"), torch.float16)
    x = synth.synth_images(2, 640, 640).cuda().half()
    m(x)
    with profiling.trace() as t:
        y, _ = m(x)
    torch.cuda.synchronize()
    assert torch.isfinite(y).all()
    labels = [r[0] for r in t.records]
    assert not any("conv_direct" in k for k in labels), sorted(set(labels))
    assert [r[5] for r in t.records if r[0] == "dysample_kernel"] == ["C128 G4 40x40", "C256 G4 20x20", "C128 G4 40x40"]


def test_yolov13n_unchanged_in_the_same_process(E, golden_dir):
    """yolov13n.yaml built beside the DySample model still gives its own golden (the nearest upsample path is untouched)."""
    from edge_yolo_amd.nn.tasks import DetectionModel
    _build(NAME.format("n"), torch.float32)(synth.synth_images(1, 96, 160).cuda())
    g = np.load(os.path.join(golden_dir, "yolov13n_96x160.npz"))
    m = DetectionModel("yolov13n.yaml")
    m.load_state_dict(synth.synth_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, gain=0.5))
    m = m.to("cuda").fuse().float().eval()
    assert any(type(l).__name__ == "Upsample" for l in m.model)
    y, raw = m(synth.synth_images(1, 96, 160).cuda())
    np.testing.assert_allclose(y.cpu().numpy(), g["y"], rtol=1e-4, atol=1e-3)
    for i, r in enumerate(raw):
        np.testing.assert_allclose(r.float().cpu().numpy(), g[f"raw{i}"], rtol=1e-4, atol=2e-4)
