"""-m gpu: the fused wavelet kernel (wavelet_z_kernel, csrc/wavelet.hip: 32 instantiations = c in {16, 32, 64, 128} x filter length
{2, 4, 6, 8} x dense / DSConv f_h) and the Haar dwt_kernel against fp64 (tests/fp64_wavelet_ref.py; the reference and the gates are
proved on the CPU in tests/test_wavelet_ref_cpu.py).

* Bounded: general data, every instantiation at a ragged multi-tile odd map, the smallest legal map and the model's own map; the
  input is a channel slice of a wider buffer whose other channels are NaN.  Per-element bound + mean-ulp gate (fp64_ref.report).
* Impulse locality: one non-zero pixel per image at corners, tile seams, borders; outside the fp64 footprint Z keeps the bits of the
  zero-input constant.
* Schedule (xcd_map = 0) and repeatability: the same bits.
* Haar dwt_kernel: bit-exact on integers, bounded on general data, both dtypes, vector and scalar paths, output into a channel slice.
* The step: every wavelet / dwt launch of a batch-32 and a batch-1 forward at 640x640 is covered here by (label, c), and every distinct
  ops.wavelet_z call is replayed at its exact shape and view (the batch-32 fp64 references are the cost of this file).

Measured on an MI355X, fp64_ref.report's `max err/bound / mean ulp` per instantiation at the ragged, smallest and model map.  Every
Haar case but one has its mean-ulp gate from the unfused path (fp64_wavelet_ref.UNFUSED_MEAN_ULP says why and holds the figures); the
fused kernel measured 0.999 .. 1.002 x the unfused path there.  All other cases are held to 0.5.

                  ragged          smallest        model
  haar conv C16   0.030 / 1.968   0.011 / 0.309   0.047 / 2.376
  haar conv C32   0.025 / 2.090   0.021 / 1.436   0.018 / 2.140
  haar conv C64   0.007 / 2.512   0.008 / 1.141   0.007 / 2.602
  haar conv C128  0.004 / 2.605   0.004 / 3.156   0.004 / 2.834
  haar ds   C16   0.033 / 2.392   0.036 / 6.179   0.035 / 2.950
  haar ds   C32   0.016 / 3.939   0.013 / 0.771   0.014 / 2.786
  haar ds   C64   0.007 / 3.318   0.006 / 1.330   0.006 / 3.004
  haar ds   C128  0.003 / 3.262   0.005 / 1.737   0.003 / 2.622
   db2 conv C16   0.026 / 0.260   0.026 / 0.247   0.021 / 0.262
   db2 conv C32   0.012 / 0.262   0.012 / 0.254   0.012 / 0.262
   db2 conv C64   0.006 / 0.272   0.007 / 0.245   0.008 / 0.287
   db2 conv C128  0.003 / 0.353   0.005 / 0.249   0.003 / 0.297
   db2 ds   C16   0.017 / 0.256   0.024 / 0.293   0.019 / 0.258
   db2 ds   C32   0.009 / 0.261   0.011 / 0.255   0.009 / 0.276
   db2 ds   C64   0.005 / 0.267   0.005 / 0.259   0.005 / 0.287
   db2 ds   C128  0.003 / 0.288   0.002 / 0.247   0.003 / 0.385
   db3 conv C16   0.023 / 0.268   0.014 / 0.250   0.020 / 0.265
   db3 conv C32   0.012 / 0.272   0.014 / 0.254   0.014 / 0.279
   db3 conv C64   0.006 / 0.294   0.007 / 0.251   0.008 / 0.382
   db3 conv C128  0.003 / 0.329   0.002 / 0.252   0.003 / 0.281
   db3 ds   C16   0.018 / 0.260   0.014 / 0.231   0.021 / 0.259
   db3 ds   C32   0.010 / 0.266   0.010 / 0.255   0.010 / 0.278
   db3 ds   C64   0.005 / 0.266   0.005 / 0.251   0.005 / 0.301
   db3 ds   C128  0.002 / 0.303   0.002 / 0.271   0.003 / 0.408
   db4 conv C16   0.018 / 0.269   0.022 / 0.246   0.023 / 0.265
   db4 conv C32   0.012 / 0.284   0.009 / 0.256   0.011 / 0.287
   db4 conv C64   0.006 / 0.354   0.005 / 0.294   0.005 / 0.298
   db4 conv C128  0.003 / 0.401   0.003 / 0.370   0.003 / 0.315
   db4 ds   C16   0.019 / 0.262   0.015 / 0.259   0.020 / 0.269
   db4 ds   C32   0.009 / 0.272   0.007 / 0.266   0.011 / 0.276
   db4 ds   C64   0.005 / 0.296   0.004 / 0.247   0.004 / 0.322
   db4 ds   C128  0.003 / 0.326   0.003 / 0.339   0.003 / 0.340
"""
import zlib

import pytest
import torch

pytestmark = pytest.mark.gpu

import fp64_ref as R  # noqa: E402
import fp64_wavelet_ref as WR  # noqa: E402
from gpu_util import _traced, tuned  # noqa: E402
from test_gpu_conv_exact import _holder, _nhwc  # noqa: E402

F16 = torch.float16
NAMES = list(WR.NAMES)
INST = [(n, ds, c) for n in NAMES for ds in (False, True) for c in WR.CS]
INST_IDS = [f"{n}-{'ds' if ds else 'conv'}-C{c}" for n, ds, c in INST]


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _label(name, use_ds):
    k = WR.NAMES[name]
    return "wavelet_z_kernel" if k == 2 and not use_ds else f"wavelet_z_kernel<k{k}{',ds' if use_ds else ''}>"


COVERED = {(_label(n, ds), c) for n, ds, c in INST}
DWT_CS = (3, 8, 16, 32, 64, 128)
COVERED |= {("dwt_kernel", c) for c in DWT_CS}


def _dwt(name):
    from edge_yolo_amd.nn.modules import block
    return block._PywtDWT2D(name)


def _fns(w, c):
    """sets_fn / z_fn / dw_fn of nn._ops.wavelet_z from the natural weights: f_ll and (use_ds) f_h's pointwise as centre-tap 3x3 sets."""
    h = c // 2

    def centre(w1):
        w3 = torch.zeros((h, c, 3, 3))
        w3[:, :, 1:2, 1:2] = w1.float()
        return w3

    wh3 = centre(w["wh"]) if w["wdw"] is not None else w["wh"].float()
    sets_fn = lambda: ((centre(w["wl"]), w["bl"]), (wh3, w["bh"]))  # noqa: E731
    z_fn = lambda: (w["wz"].float(), None)  # noqa: E731
    dw_fn = (lambda: w["wdw"].float()) if w["wdw"] is not None else None
    return sets_fn, z_fn, dw_fn


def _view(x, cs=None, off=8):
    """the kernel's input as the model passes it: a channel slice [off, off + c) of a cs-channel NHWC buffer, NaN elsewhere"""
    from edge_yolo_amd import _lib as L
    B, c, H, W = x.shape
    if cs is None:
        return _nhwc(B, c, H, W, F16, x, pad=16)
    buf = L.empty_nhwc(B, cs, H, W, F16, "cuda")
    buf.fill_(float("nan"))
    t = buf[:, off:off + c]
    t.copy_(x)
    return t


def _fused(name, use_ds, xd, w, tune=None):
    from edge_yolo_amd.nn import _ops
    sets_fn, z_fn, dw_fn = _fns(w, xd.shape[1])
    with tuned(**(tune or {})):
        z, labels = _traced(lambda: _ops.wavelet_z(_holder(), xd, sets_fn, z_fn, dwt=_dwt(name), dw_fn=dw_fn))
    assert z is not None, "ops.wavelet_z declined the call"
    assert labels == [_label(name, use_ds)], f"{name} ds={use_ds}: launched {labels}, expected one {_label(name, use_ds)}"
    return z, labels[0]


def _unfused(name, use_ds, xd, w):
    """_WaveletEnhancer's three-launch f16 form (fused_z = False) up to Z, on the same weights: dwt_kernel / dwt_general_kernel, the
    4-group conv or f_ll + three DSConvs, the 1x1 -- the path the mean-ulp gates are measured on."""
    from edge_yolo_amd import _lib as L
    from edge_yolo_amd.nn import _ops
    B, c, H, W = xd.shape
    h = c // 2
    sets_fn, z_fn, dw_fn = _fns(w, c)
    sub = _dwt(name).subbands(xd)
    P = L.empty_nhwc(B, 2 * c, H // 2, W // 2, F16, "cuda")
    if use_ds:
        _ops.conv2d(_holder(), [sub[:, :c]], lambda: (w["wl"].float(), w["bl"]), 1, 1, 0, L.ACT_SILU, out=P[:, :h])
        for i in (1, 2, 3):
            src, dst = sub[:, i * c:(i + 1) * c], P[:, i * h:(i + 1) * h]
            hold = _holder()
            y = _ops.dsconv(hold, src, lambda: (w["wdw"].float(), None), lambda: (w["wh"].float(), w["bh"]), 3, L.ACT_SILU, out=dst)
            if y is None:
                t = _ops.dwconv(hold, src, lambda: (w["wdw"].float(), None), 3, L.ACT_NONE, tag="dw")
                _ops.conv2d(hold, [t], lambda: (w["wh"].float(), w["bh"]), 1, 1, 0, L.ACT_SILU, out=dst, tag="pw")
    else:
        _ops.conv2d(_holder(), [sub[:, :c]], lambda: list(sets_fn()), 3, 1, 1, L.ACT_SILU, out=P[:, :h], ngroup=4, src_gstride=c, y_gstride=h, w_sets=2)
    z = _ops.conv2d(_holder(), [P], z_fn, 1, 1, 0, L.ACT_NONE)
    torch.cuda.synchronize()
    return z


def _ref(name, x, w):
    taps = _dwt(name).taps32.to(F16)
    return WR.wavelet_z_ref(x.cuda(), taps, w["wl"].cuda(), w["bl"], w["wh"].cuda(), w["bh"], w["wz"].cuda(), w["wdw"].cuda() if w["wdw"] is not None else None)


def _bounded(name, use_ds, c, B, H, W, cid, cs=None, off=8, unfused=False):
    """one bounded case; returns the (max err/bound, mean ulp) of the fused kernel (and of the unfused path, unasserted, when asked)"""
    w = WR.weights(c, use_ds, _gen("w", name, use_ds, c))
    x = WR.general_input(B, c, H, W, _gen("x", cid, B, H, W))
    xd = _view(x, cs, off)
    z, bz, _, _ = _ref(name, x, w)
    got, label = _fused(name, use_ds, xd, w)
    out = [None, None]
    if unfused:  # measurement only (the figures of fp64_wavelet_ref.UNFUSED_MEAN_ULP): printed, gated by nothing
        g = _unfused(name, use_ds, xd, w).double()
        out[1] = (float(((g - z).abs() / bz).max()), float(((g - z).abs() / R.ulp16(z)).mean()))
        print(f"[unfused] {cid} max err/bound {out[1][0]:.3f}  mean ulp {out[1][1]:.4f}")
    out[0] = R.report(f"{cid} {B}x{H}x{W}", f"{label} C{c}", got, z, bz, WR.mean_ulp_gate(cid))
    return out


# ------------------------------------------------------------------------------------------------------------------------ bounded
@pytest.mark.parametrize("kind", ["ragged", "min", "model"])
@pytest.mark.parametrize("name,use_ds,c", INST, ids=INST_IDS)
def test_wavelet_z_within_fp64_bound(name, use_ds, c, kind):
    B, H, W = WR.bounded_shapes(name, c)[kind]
    _bounded(name, use_ds, c, B, H, W, WR.case_id(name, use_ds, c, kind))


def test_recorded_unfused_mean_ulp():
    """every gate above 0.5 is 1.25 x a figure of the unfused path: re-measure each one (the kernels are deterministic)"""
    for cid, want in WR.UNFUSED_MEAN_ULP.items():
        name, form, cc, kind = cid.split("-")
        c, use_ds = int(cc[1:]), form == "ds"
        if kind.startswith("step"):
            continue  # re-measured by test_step_wavelet_calls_replay_within_bound (the view comes from the forward)
        B, H, W = WR.bounded_shapes(name, c)[kind]
        _, (_, mu) = _bounded(name, use_ds, c, B, H, W, cid, unfused=True)
        assert abs(mu - want) <= 0.02 * want + 1e-3, f"{cid}: the unfused path measures {mu:.4f} mean ulp, the table says {want}"


# ------------------------------------------------------------------------------------------------------------------------ impulse locality
@pytest.mark.parametrize("name,use_ds,c", INST, ids=INST_IDS)
def test_wavelet_z_impulse_locality(name, use_ds, c):
    w = WR.weights(c, use_ds, _gen("w", name, use_ds, c))
    for H, W in WR.IMPULSE_HWS:
        spots = WR.impulse_spots(H, W, WR.tile_h(c))
        assert len(spots) >= 18
        x = torch.cat([torch.zeros((1, c, H, W), dtype=torch.float64), WR.impulse_input(c, H, W, spots, _gen("imp", name, use_ds, c, H))])
        got, label = _fused(name, use_ds, _view(x), w)
        z, bz, _, _ = _ref(name, x, w)
        WR.check_impulse(f"{name}{' ds' if use_ds else ''} C{c} {H}x{W}", label, got[:1], got[1:], z[:1], bz[:1], z[1:], bz[1:], spots, H, W, WR.NAMES[name])


# ------------------------------------------------------------------------------------------------------------------------ schedule
@pytest.mark.parametrize("name,use_ds,c", INST, ids=INST_IDS)
def test_wavelet_z_schedule_and_repeat_same_bits(name, use_ds, c):
    """the XCD-contiguous tile order (xcd_map bit 2) off, and a second launch: the same bits on a ragged multi-tile map"""
    B, H, W = WR.bounded_shapes(name, c)["ragged"]
    w = WR.weights(c, use_ds, _gen("w", name, use_ds, c))
    xd = _view(WR.general_input(B, c, H, W, _gen("sched", name, use_ds, c)))
    a, _ = _fused(name, use_ds, xd, w)
    b, _ = _fused(name, use_ds, xd, w)
    s, _ = _fused(name, use_ds, xd, w, tune=dict(xcd_map=0))
    assert torch.isfinite(a).all()
    assert torch.equal(a, b), "two launches on the same input differ"
    assert torch.equal(a, s), "xcd_map = 0 changes the result"


# ------------------------------------------------------------------------------------------------------------------------ Haar dwt_kernel
def _dwt_case(c, path, B, H, W, dtype, exact):
    """ey_dwt_haar through nn._ops.dwt_haar: input = a channel slice of a NaN buffer (aligned: 16-byte offset, vector path when
    c % 8 == 0; misaligned: offset of 2 channels, scalar path), output = the slice [8, 8 + 4c) of a wider buffer filled with 5."""
    from edge_yolo_amd import _lib as L
    from edge_yolo_amd.nn import _ops
    gen = _gen("dwt", c, path, B, H, W, str(dtype), exact)
    x = R.ex_input((B, c, H, W), gen) if exact else torch.randn((B, c, H, W), generator=gen).to(dtype).double()
    off = 8 if path == "aligned" else 2
    buf = L.empty_nhwc(B, c + 16, H, W, dtype, "cuda")
    buf.fill_(float("nan"))
    xd = buf[:, off:off + c]
    xd.copy_(x)
    obuf = L.empty_nhwc(B, 4 * c + 16, H // 2, W // 2, dtype, "cuda")
    obuf.fill_(5.0)
    out = obuf[:, 8:8 + 4 * c]
    _, labels = _traced(lambda: _ops.dwt_haar(xd, out=out))
    assert labels == ["dwt_kernel"], labels
    assert bool((obuf[:, :8] == 5.0).all()) and bool((obuf[:, 8 + 4 * c:] == 5.0).all()), "dwt_kernel wrote outside its output channel slice"
    taps = _dwt("haar").taps32.to(dtype).double().cuda()
    ys, bs = [], []
    for band in range(4):
        y, A, Y = R.conv_ref([x.cuda()], R._dense(taps[band].expand(c, 1, 2, 2)), None, 2, 2, 0)
        ys.append(y)
        bs.append(R.bound(y, A, Y, 4, f16_out=dtype == F16))
    return out, torch.cat(ys, 1), torch.cat(bs, 1)


_DWT_SHAPES = [(2, 10, 14), (3, 9, 13), (2, 2, 2), (1, 3, 2)]
_DWT_PATHS = [(c, "aligned") for c in DWT_CS] + [(8, "misaligned"), (16, "misaligned")]


@pytest.mark.parametrize("c,path", _DWT_PATHS, ids=[f"C{c}-{p}" for c, p in _DWT_PATHS])
def test_dwt_haar_exact_f16(c, path):
    """integers in [-2, 2]: every sub-band is a multiple of 1/2 below 8, and the kernel's fp32 taps 0.49999997 round to it"""
    for B, H, W in _DWT_SHAPES:
        got, y, _ = _dwt_case(c, path, B, H, W, F16, True)
        R.assert_exact(f"dwt C{c} {path} {B}x{H}x{W}", "dwt_kernel", got, y)


@pytest.mark.parametrize("dtype", [F16, torch.float32], ids=["f16", "f32"])
@pytest.mark.parametrize("c,path", _DWT_PATHS, ids=[f"C{c}-{p}" for c, p in _DWT_PATHS])
def test_dwt_haar_within_fp64_bound(c, path, dtype):
    for B, H, W in _DWT_SHAPES:
        got, y, bnd = _dwt_case(c, path, B, H, W, dtype, False)
        R.report(f"dwt C{c} {path} {B}x{H}x{W} {str(dtype)[6:]}", "dwt_kernel", got, y, bnd)


# ------------------------------------------------------------------------------------------------------------------------ the step
_WZ_STEP = {}


def _step(batch):
    """test_gpu_conv_exact._step_forward with nn._ops.wavelet_z / dwt_haar / dwt recorded: (traced labels, wavelet_z calls, dwt calls)"""
    if batch in _WZ_STEP:
        return _WZ_STEP[batch]
    import test_gpu_conv_exact as CE
    from edge_yolo_amd import _lib as L
    from edge_yolo_amd.nn import _ops
    wz_calls, dwt_calls = [], []
    orig = (_ops.wavelet_z, _ops.dwt_haar, _ops.dwt)

    def last_label(n0):
        return _ops.TRACE.records[-1][0] if _ops.TRACE is not None and len(_ops.TRACE.records) > n0 else None

    def view(t):
        t = L.as_nhwc(t)
        base = t.untyped_storage().data_ptr()
        return (tuple(t.shape), L.cstride(t), (t.data_ptr() - base) // t.element_size() % L.cstride(t))

    def rec_wz(mod, b, sets_fn, z_fn, dwt=None, dw_fn=None):
        n0 = len(_ops.TRACE.records) if _ops.TRACE is not None else 0
        z = orig[0](mod, b, sets_fn, z_fn, dwt=dwt, dw_fn=dw_fn)
        if z is not None:
            wz_calls.append(dict(view=view(b), wave=dwt.wave_name if dwt is not None else "haar", use_ds=dw_fn is not None, label=last_label(n0)))
        return z

    def rec_dwt(i):
        def f(x, *a, **k):
            n0 = len(_ops.TRACE.records) if _ops.TRACE is not None else 0
            y = orig[i](x, *a, **k)
            dwt_calls.append((last_label(n0), x.shape[1]))
            return y
        return f

    CE._STEP.pop(batch, None)  # a forward cached before the recorders were in place saw no wavelet call
    _ops.wavelet_z, _ops.dwt_haar, _ops.dwt = rec_wz, rec_dwt(1), rec_dwt(2)
    try:
        labels, _ = CE._step_forward(batch)
    finally:
        _ops.wavelet_z, _ops.dwt_haar, _ops.dwt = orig
    _WZ_STEP[batch] = (labels, wz_calls, dwt_calls)
    return _WZ_STEP[batch]


@pytest.mark.parametrize("batch", [32, 1])
def test_step_wavelet_kernels_are_covered(batch):
    labels, wz_calls, dwt_calls = _step(batch)
    fam = [lab for lab in labels if lab.startswith(("wavelet_z_kernel", "dwt"))]
    seen = [(c["label"], c["view"][0][1]) for c in wz_calls] + list(dwt_calls)
    print(f"[step] batch {batch} at 640x640: {len(fam)} wavelet / dwt launches: {sorted(set(seen))}")
    assert fam, "no wavelet launch traced"
    assert sorted(fam) == sorted(lab for lab, _ in seen), f"wavelet / dwt launches outside the recorded entry points: {sorted(set(fam))} vs {sorted(set(seen))}"
    missing = sorted(set(seen) - COVERED)
    assert not missing, f"batch {batch}: wavelet kernels of the step that no case of this file covers (label, c): {missing}"


@pytest.mark.parametrize("batch", [32, 1])
def test_step_wavelet_calls_replay_within_bound(batch):
    """every distinct ops.wavelet_z call of the step at its exact shape, channel stride and channel offset, general data, against the
    bound.  The fp64 reference of batch 32 at c = 16, 160x160 is chunked by image (fp64_ref.conv_ref) and is the cost of this file."""
    _, wz_calls, _ = _step(batch)
    seen = {}
    for c in wz_calls:
        seen.setdefault(repr({k: v for k, v in c.items() if k != "label"}), c)
    assert seen, "no ops.wavelet_z call recorded"
    print(f"[replay] batch {batch}: {len(wz_calls)} wavelet_z calls, {len(seen)} distinct")
    for call in seen.values():
        (B, c, H, W), cs, off = call["view"]
        assert B == batch
        name, use_ds = call["wave"], call["use_ds"]
        assert call["label"] == _label(name, use_ds) and (call["label"], c) in COVERED
        cid = WR.case_id(name, use_ds, c, f"step{batch}")
        _, unf = _bounded(name, use_ds, c, B, H, W, cid, cs=cs, off=off, unfused=cid in WR.UNFUSED_MEAN_ULP)
        if unf is not None:  # a gate above 0.5 is 1.25 x a figure of the unfused path: re-measured here
            want = WR.UNFUSED_MEAN_ULP[cid]
            assert abs(unf[1] - want) <= 0.02 * want + 1e-3, f"{cid}: the unfused path measures {unf[1]:.4f} mean ulp, the table says {want}"
        torch.cuda.empty_cache()
