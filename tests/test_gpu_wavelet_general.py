"""-m gpu: general PyWavelets filter banks (wave=) and use_ds=True (reference block.py:3582-3788).  ey_dwt against an fp64
restatement for every wavelet of the table; the DWT, enhancer, block and whole-model paths against the reference's own outputs
(tests/golden/wavelets_*.npz, tests/golden/make_golden_wavelets.py); db1 == haar bytes; predict() / predict_batches() with graphs."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import synthdata as synth
from gpu_util import _traced, check, load_synth, to_dev

pytestmark = pytest.mark.gpu
DT = [torch.float32, torch.float16]


@pytest.fixture(scope="module")
def M():
    import edge_yolo_amd  # noqa: F401
    from edge_yolo_amd.nn.modules import block
    return block


@pytest.fixture(scope="module")
def G(golden_dir):
    return np.load(os.path.join(golden_dir, "wavelets_ops.npz"))


def _dwt64(x, taps, k):
    """fp64 restatement of _PywtDWT2D.forward: reflect pad k/2-1, depthwise k x k conv, stride 2 -> (B, 4C, Ho, Wo) as LL|LH|HL|HH."""
    B, C, H, W = x.shape
    p = k // 2 - 1
    xp = F.pad(x.double(), (p, p, p, p), mode="reflect") if p else x.double()
    y = F.conv2d(xp, taps.double().reshape(4, 1, k, k).repeat(C, 1, 1, 1), stride=2, groups=C)  # (B, C*4, Ho, Wo): per channel 4 bands
    return y.view(B, C, 4, *y.shape[-2:]).transpose(1, 2).reshape(B, 4 * C, *y.shape[-2:])


def _run_dwt(d, x):
    from edge_yolo_amd import _lib as L
    return L.as_nhwc(d.subbands(x))


@pytest.mark.parametrize("dtype", DT)
def test_ey_dwt_every_wavelet_vs_fp64(M, dtype):
    """Every wavelet of the table at the smallest legal map (pad = H - 1), an odd and an even map; c = 8 (vector path) and c = 3."""
    table, _ = M.wavelet_filters()
    for name in sorted(table):
        d = M._PywtDWT2D(name)
        k, p = d.k, d.pad
        for (b, c, h, w) in ((2, 8, max(p + 1, 2), max(p + 2, 3)), (1, 3, 2 * p + 5, 2 * p + 4), (2, 8, 2 * p + 6, 2 * p + 7)):
            x = (synth.synth_images(b, h, w, c=c) * 2 - 1).to(dtype)  # (representable in dtype)
            got = _run_dwt(d, x.cuda()).float().cpu().double()
            taps = d.taps32.to(dtype)
            want = _dwt64(x, taps, k)
            assert got.shape == want.shape, (name, got.shape, want.shape)
            if dtype == torch.float32:
                err = (got - want).abs().max()
                assert float(err) <= 2e-4, (name, (b, c, h, w), float(err))
            else:  # fp32 accumulation of k*k products, one f16 rounding: |err| <= 2^-11 |y| + (k*k + 1) 2^-24 sum|t x| + 2^-24
                s = _dwt64(x.abs(), taps.abs(), k)
                bound = 2.0 ** -11 * want.abs() + (k * k + 1) * 2.0 ** -24 * s + 2.0 ** -24
                assert bool(((got - want).abs() <= bound).all()), (name, (b, c, h, w), float(((got - want).abs() - bound).max()))


def test_ey_dwt_refuses_small_maps(M):
    from edge_yolo_amd import _lib as L
    x = torch.zeros(1, 8, 30, 40, device="cuda")
    with pytest.raises(ValueError):
        M._PywtDWT2D("dmey")(x)  # pad 30 >= H
    xn = L.as_nhwc(x)
    y = torch.zeros(1, 15, 20, 32, device="cuda")
    taps = M._PywtDWT2D("dmey").taps(xn)
    assert L.lib().ey_dwt(L.dtype_code(x.dtype), 1, 30, 40, 8, 62, taps.data_ptr(), xn.data_ptr(), 8, y.data_ptr(), 32, L.stream()) == -1
    assert bool((y == 0).all())


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("name", ["haar", "db2", "sym4", "coif1", "bior2.2", "rbio3.3", "db10", "dmey"])
def test_dwt_vs_reference_golden(M, G, dtype, name):
    d = M._PywtDWT2D(name)
    for tag in ("even", "odd", "min"):
        x = torch.from_numpy(G[f"dwt_{name}_{tag}_x"])
        check(torch.cat(d(x.cuda().to(dtype)), 1), torch.from_numpy(G[f"dwt_{name}_{tag}"]), dtype, what=f"{name} {tag}")
    if int(G[f"dwt_{name}_raises_at_pad"]):
        with pytest.raises(ValueError):
            d(torch.zeros(1, 8, max(d.pad, 1), d.pad + 4, device="cuda", dtype=dtype))


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("c", [16, 32])
@pytest.mark.parametrize("use_ds", [False, True])
@pytest.mark.parametrize("name", ["db2", "sym4", "coif1"])
def test_enhancer_vs_reference_golden(M, G, dtype, c, use_ds, name):
    tag = f"enh{c}_{name}_{'ds' if use_ds else 'conv'}"
    m = M._WaveletEnhancer(c, use_ds=use_ds, wave=name)
    load_synth(m, tag)
    m = to_dev(m, dtype)
    for sfx, (b, h, w) in (("even", (2, 10, 14)), ("odd", (1, 9, 13))):
        x = synth.synth_images(b, h, w, c=c) - 0.5
        got, kernels = _traced(lambda: m(x.cuda().to(dtype)))
        if dtype == torch.float16:  # the fused half-resolution kernel, then the tail conv
            assert kernels[0] == f"wavelet_z_kernel<k{m.dwt.k}{',ds' if use_ds else ''}>" and len(kernels) == 2, kernels
        else:
            assert any(k.startswith("dwt_general_kernel") for k in kernels), kernels
            if use_ds:
                assert sum(k.startswith("dsconv") for k in kernels) == 3 or sum(k.startswith("dw") for k in kernels) == 4, kernels  # f_h on LH, HL, HH
        check(got, torch.from_numpy(G[f"{tag}_{sfx}"]), dtype, what=f"{tag} {sfx}")


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("dsc3k", [False, True])
def test_dsc3k2_wavelet_sym4_ds_vs_reference_golden(M, G, dtype, dsc3k):
    tag = f"dsc3k2w_sym4_ds_{int(dsc3k)}"
    m = M.DSC3K2_Wavelet(32, 64, 2, dsc3k, wave="sym4", use_ds=True)
    load_synth(m, tag)
    x = synth.synth_images(2, 12, 16, c=32) - 0.5
    check(to_dev(m, dtype)(x.cuda().to(dtype)), torch.from_numpy(G[tag]), dtype, scale=2, what=tag)


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("hw", [(10, 14), (9, 13), (2, 3)])
def test_db1_is_haar_bytes(M, dtype, hw):
    x = (synth.synth_images(2, *hw, c=16) - 0.5).cuda().to(dtype)
    outs = []
    for name in ("haar", "db1"):
        m = M._WaveletEnhancer(16, wave=name)
        load_synth(m, "enh")
        m = to_dev(m, dtype)
        outs.append((torch.cat(m.dwt(x), 1).clone(), m(x).clone()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def _model(wave):
    import edge_yolo_amd as E
    from edge_yolo_amd.nn.tasks import yaml_model_load
    d = dict(yaml_model_load("yolo11n-test.yaml"))
    d["backbone"] = [list(r) for r in d["backbone"]]
    d["head"] = [list(r) for r in d["head"]]
    for r in d["backbone"] + d["head"]:
        if r[2] == "DSC3K2_Wavelet":
            r[3] = list(r[3]) + [{"wave": wave, "use_ds": True}]
    y = E.YOLO(d)
    y.model.load_state_dict(synth.synth_state_dict({k: tuple(v.shape) for k, v in y.model.state_dict().items()}))
    return y, d


@pytest.mark.parametrize("wave,tag,b,hw", [("db2", "wavelets_n_64", 2, 64), ("sym4", "wavelets_n_256", 1, 256)])
def test_whole_model_fp32_vs_reference_golden(golden_dir, wave, tag, b, hw):
    """EdgeLine-n with every enhancer _WaveletEnhancer(c, use_ds=True, wave=...): raw head outputs within the 1e-3 north-star bar; f16
    decoded outputs against this fp32 model within the f16 model bars of tests/test_gpu_model.py::test_fp16_vs_oracle (scores 2e-2, boxes
    1.5% of the image size)."""
    g = np.load(os.path.join(golden_dir, tag + ".npz"))
    y, _ = _model(wave)
    m = y.model.to("cuda")
    m.fuse()
    m = m.float().eval()
    for j in g["wave_layers"]:
        assert m.model[int(j)].wave.dwt.wave_name == wave
    x = synth.synth_images(b, hw, hw).cuda()
    out, raw = m(x)
    for i, r in enumerate(raw):
        np.testing.assert_allclose(r.float().cpu().numpy(), g[f"raw{i}"], rtol=1e-4, atol=1e-3, err_msg=f"raw{i}")
    out = out.cpu()
    yh, _ = m.half()(x.half())
    yh = yh.float().cpu()
    assert float((yh[:, 4:] - out[:, 4:]).abs().max()) < 2e-2
    assert float((yh[:, :4] - out[:, :4]).abs().max()) < 0.015 * hw


def test_sym4_model_refuses_64(M):
    y, _ = _model("sym4")
    m = y.model.to("cuda").float().eval()
    with pytest.raises(ValueError, match="reflect padding 3"):
        m(synth.synth_images(1, 64, 64).cuda())  # P5 maps are 2x2: the reference refuses them too


@pytest.mark.parametrize("half", [False, True])
def test_predict_db2_ds_640_graph(half):
    """predict() with graph capture == eager, replay included; predict_batches returns what predict returns."""
    y, _ = _model("db2")
    x = synth.synth_images(2, 640, 640)
    r1 = y.predict(x, conf=0.25, iou=0.7, device="cuda:0", half=half, graph=False)
    r2 = y.predict(x, conf=0.25, iou=0.7, device="cuda:0", half=half, graph=True)
    r3 = y.predict(x, conf=0.25, iou=0.7, device="cuda:0", half=half, graph=True)
    assert sum(len(r.boxes.data) for r in r1) > 0
    for a, b, c in zip(r1, r2, r3):
        assert torch.equal(a.boxes.data.cpu(), b.boxes.data.cpu()) and torch.equal(a.boxes.data.cpu(), c.boxes.data.cpu())
    outs = list(y.predict_batches([x, x], conf=0.25, iou=0.7, half=half))
    assert len(outs) == 2
    for res in outs:
        for a, b in zip(res, r2):
            assert torch.equal(a.boxes.data.cpu(), b.boxes.data.cpu())


# ---- the fused half-resolution kernel (ey_wavelet_z2) against the unfused f16 form: k in {4, 6, 8} (db2, db3, db4) x use_ds x c, at the
# benchmarked model's enhancer shapes (c / map = 16/160, 32/80, 64/40, 128/20), an odd map and the smallest legal map (pad = H - 1)
_WZ_SHAPES = [(16, 160, 160, 2), (32, 80, 80, 2), (64, 40, 40, 2), (128, 20, 20, 2), (64, 21, 37, 2), (32, 9, 13, 1)]


@pytest.mark.parametrize("name", ["haar", "db2", "db3", "db4"])
@pytest.mark.parametrize("use_ds", [False, True])
@pytest.mark.parametrize("c,h,w,b", _WZ_SHAPES + [(16, 4, 5, 1), (128, 4, 6, 2)])
def test_fused_wavelet_z_vs_unfused_f16(M, name, use_ds, c, h, w, b):
    """Same rounding points as the unfused f16 launches (sub-bands, depthwise output and P stored as f16), so the results agree to the
    f16 rounding of the MFMA sums: the bar of the Haar kernel's own test (tests/test_gpu_ops.py::test_wavelet_z_kernel_vs_oracle_and_unfused).
    Every filter length keeps the smallest legal map (pad = H - 1 for db4 at 4x5) inside the fused kernel."""
    m = M._WaveletEnhancer(c, use_ds=use_ds, wave=name)
    load_synth(m, f"enh{c}")
    mh = to_dev(m, torch.float16)
    x = (synth.synth_images(b, h, w, c=c) - 0.5).cuda().half()
    got, kernels = _traced(lambda: mh(x))
    assert kernels[0].startswith("wavelet_z_kernel") and len(kernels) == 2, kernels
    mh.fused_z = False
    ref = mh(x)
    torch.cuda.synchronize()
    scale = float(ref.float().abs().max())
    assert float((got.float() - ref.float()).abs().max()) <= 3e-3 * scale

