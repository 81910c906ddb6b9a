"""-m gpu: ey_process_mask (csrc/segment.hip) against the float64 restatement tests/fp64_mask_ref.py.

Criterion (derived, not measured): the bits equal the fp64 bits at every pixel where |v| > E,
    E = 1.05 * [(nm + 2) u blend(sum|coef proto|) + 8 u max|corner v|],  u = 2^-24;
pixels with |v| <= E may go either way, and their share of the in-box pixels is capped at 1e-3 per case (a cap, not a tolerance).  The
dyadic probe allows no exclusions: its sums are exact in any order.  proto and the coefficient maps are channel windows of wider NaN-filled
buffers, the output a slice of a sentinel-filled buffer; nothing outside the slice may change and every byte inside is 0 or 1."""
import zlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import fp64_mask_ref as f64  # noqa: E402
import seg_synth  # noqa: E402

SENT = 0xAB
LEVELS = {1: [(3, 5)], 3: [(4, 6), (2, 3), (1, 2)], 4: [(4, 6), (2, 3), (1, 2), (1, 1)]}
# (mh, mw, s, nm, N, levels, byte offset of the output slice in its buffer)
CASES = [(1, 1, 4, 8, 17, 1, 16), (1, 1, 1, 32, 1, 1, 5), (2, 3, 2, 40, 17, 3, 16), (5, 7, 8, 32, 17, 4, 32), (16, 24, 4, 32, 301, 3, 16),
         (17, 33, 2, 8, 17, 1, 16), (40, 24, 4, 40, 17, 4, 64), (17, 33, 1, 32, 17, 3, 7), (40, 24, 8, 8, 1, 1, 16), (5, 7, 4, 32, 0, 3, 16),
         (16, 24, 1, 40, 301, 1, 16), (2, 3, 8, 32, 17, 3, 16), (40, 80, 4, 32, 17, 3, 16), (16, 24, 4, 32, 17, 3, 3)]
DTYPES = [torch.float32, torch.float16]


def _draw(r, shape, dt, dyadic):
    if dyadic:
        return r.integers(-8, 9, shape).astype(np.float32) * np.float32(0.125)
    a = r.normal(0.0, 1.0, shape).astype(np.float32)
    return a.astype(np.float16).astype(np.float32) if dt == torch.float16 else a


def _window(a_nhwc, dt, lead=8, trail=8):
    """numpy [.., C] -> a channel window [lead, lead + C) of a NaN-filled device buffer, as a logical-NCHW NHWC view."""
    *d, c = a_nhwc.shape
    buf = torch.full((*d, lead + c + trail), float("nan"), dtype=dt, device="cuda")
    buf[..., lead:lead + c] = torch.tensor(a_nhwc).to(dt)
    return buf[..., lead:lead + c].permute(0, 3, 1, 2), buf


def build(case, dt, dyadic=False, B=2, seed=0):
    mh, mw, s, nm, N, nl, lead = case
    r = np.random.default_rng([zlib.crc32(repr((case, str(dt), dyadic)).encode()), seed])
    proto = _draw(r, (B, mh, mw, nm), dt, dyadic)
    maps = [_draw(r, (B, h, w, nm), dt, dyadic) for h, w in LEVELS[nl]]
    A = sum(h * w for h, w in LEVELS[nl])
    anchors, off = [], 0
    for h, w in LEVELS[nl]:  # first and last anchor of every level, then random ones
        anchors += [off, off + h * w - 1]
        off += h * w
    anchors = (anchors + r.integers(0, A, max(N, 1)).tolist())[:N] if N else []
    k = zlib.crc32(repr(case).encode()) % 2
    imgs = np.ones(N, np.int32) if k else (np.arange(N) >= (2 * N + 2) // 3).astype(np.int32)  # all in image 1 (image 0 has none) / uneven
    rows = np.stack([imgs, np.array(anchors, np.int32)], 1).astype(np.int32) if N else np.zeros((0, 2), np.int32)
    boxes = seg_synth.boxes_for(r, N, mh * s, mw * s, s)
    return dict(proto=proto, maps=maps, rows=rows, boxes=boxes, case=case, dt=dt)


def reference(c):
    mh, mw, s, nm, N, nl, _ = c["case"]
    flat = np.concatenate([m.reshape(m.shape[0], -1, nm) for m in c["maps"]], 1)  # [B, A, nm] in concatenated anchor order
    out = dict(v=np.zeros((N, mh * s, mw * s)), mag=np.zeros((N, mh * s, mw * s)), corner=np.zeros((N, mh * s, mw * s)), bits=np.zeros((N, mh * s, mw * s), np.uint8))
    for b in range(c["proto"].shape[0]):
        sel = np.nonzero(c["rows"][:, 0] == b)[0]
        if len(sel):
            ref = f64.process_mask64(c["proto"][b].transpose(2, 0, 1), flat[b, c["rows"][sel, 1]], c["boxes"][sel], s)
            for k in out:
                out[k][sel] = ref[k]
    return out


def launch(c, extra_rows=3):
    from edge_yolo_amd.nn import _ops
    mh, mw, s, nm, N, nl, lead = c["case"]
    dt = c["dt"]
    proto, _ = _window(c["proto"], dt)
    maps = [_window(m, dt)[0] for m in c["maps"]]
    rows = torch.tensor(np.concatenate([c["rows"], np.full((extra_rows, 2), 0, np.int32)])).cuda()  # rows beyond N are never read into the output
    boxes = torch.tensor(np.concatenate([c["boxes"], np.tile(np.array([[0, 0, 1e4, 1e4]], np.float32), (extra_rows, 1))])).cuda()
    size = N * mh * s * mw * s
    buf = torch.full((lead + size + 64,), SENT, dtype=torch.uint8, device="cuda")
    out = buf[lead:lead + size].view(N, mh * s, mw * s)
    got = _ops.process_mask(proto, maps, rows, boxes, s, n=N, out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    b = buf.cpu().numpy()
    assert (b[:lead] == SENT).all() and (b[lead + size:] == SENT).all(), "bytes around the output slice changed"
    g = b[lead:lead + size].reshape(N, mh * s, mw * s)
    assert ((g == 0) | (g == 1)).all(), "a byte inside the slice is neither 0 nor 1"
    return g


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f16"])
@pytest.mark.parametrize("case", CASES, ids=[f"{c[0]}x{c[1]}_s{c[2]}_nm{c[3]}_N{c[4]}_L{c[5]}_o{c[6]}" for c in CASES])
def test_bits_against_fp64(case, dt):
    c = build(case, dt)
    got = launch(c)
    ref = reference(c)
    und, tot = f64.check_bits(got, ref, case[3])
    print(f"undecided {und} of {tot} in-box pixels; set bits {int(got.sum())}")
    if case[4] >= 17:
        assert tot > 0 and got.any()


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f16"])
@pytest.mark.parametrize("case", [CASES[3], CASES[4], CASES[6], CASES[7], CASES[11]], ids=lambda c: f"{c[0]}x{c[1]}_s{c[2]}_nm{c[3]}")
def test_dyadic_probe_is_bit_exact(case, dt):
    """Coefficients and protos are small integers / 8: every partial sum and every blend is exact in fp32 in any order -> no exclusions."""
    c = build(case, dt, dyadic=True)
    got = launch(c)
    ref = reference(c)
    np.testing.assert_array_equal(got, ref["bits"])
    assert got.any() and not got.all()


@pytest.mark.parametrize("kw", [dict(s=3), dict(nm=12), dict(nl=5)], ids=["s3", "nm12", "5levels"])
def test_refusals_leave_the_output_untouched(kw):
    from edge_yolo_amd.nn import _ops
    s, nm, nl = kw.get("s", 4), kw.get("nm", 8), kw.get("nl", 1)
    proto = torch.zeros(1, 4, 4, nm, device="cuda").permute(0, 3, 1, 2)
    maps = [torch.zeros(1, 2, 2, nm, device="cuda").permute(0, 3, 1, 2) for _ in range(nl)]
    rows = torch.zeros(2, 2, dtype=torch.int32, device="cuda")
    boxes = torch.tensor([[0.0, 0.0, 8.0, 8.0]] * 2, device="cuda")
    out = torch.full((2, 4 * s, 4 * s), SENT, dtype=torch.uint8, device="cuda")
    with pytest.raises(NotImplementedError):
        _ops.process_mask(proto, maps, rows, boxes, s, out=out)
    torch.cuda.synchronize()
    assert bool((out == SENT).all())


def test_out_of_range_rows_give_zero_masks():
    from edge_yolo_amd.nn import _ops
    c = build((5, 7, 4, 32, 17, 3, 16), torch.float32)
    A = sum(h * w for h, w in LEVELS[3])
    bad = {0: (2, 0), 3: (-1, 1), 5: (0, A), 8: (1, -1), 11: (0, 2 ** 31 - 1)}
    for i, rw in bad.items():
        c["rows"][i] = rw
    c["boxes"][:] = (-10.0, -10.0, 100.0, 100.0)  # every valid row has a full-image box
    got = launch(c)
    keep = np.array([i not in bad for i in range(17)])
    assert not got[~keep].any()
    c["rows"][~keep] = (0, 0)
    ref = reference(c)
    f64.check_bits(got[keep], {k: v[keep] for k, v in ref.items()}, 32)
    assert got[keep].any()


def test_utils_process_mask_reference_signature(golden_dir):
    """utils.ops.process_mask(protos, masks_in, bboxes, shape, upsample) on the reference's own cases (tests/golden/seg_ops.npz)."""
    import os
    from edge_yolo_amd.utils import ops as uops
    g = np.load(os.path.join(golden_dir, "seg_ops.npz"))
    for case in seg_synth.PM_GOLDEN:
        tag, s, half, nm = case[:4]
        protos, coef, boxes, shape = seg_synth.pm_golden_case(*case)
        dt = torch.float16 if half else torch.float32
        got = uops.process_mask(torch.tensor(protos).cuda().to(dt), torch.tensor(coef).cuda(), torch.tensor(boxes).cuda(), shape, upsample=True)
        assert got.dtype == torch.uint8 and tuple(got.shape) == g[tag + "_bits"].shape
        ref = f64.process_mask64(protos, coef, boxes, s)
        f64.check_bits(got.cpu().numpy(), ref, nm)
        f64.check_bits(g[tag + "_bits"], ref, nm)  # (the reference's bits meet the same criterion: tests/test_seg_cpu.py)
        if s > 1:
            low = uops.process_mask(torch.tensor(protos).cuda().to(dt), torch.tensor(coef).cuda(), torch.tensor(boxes).cuda(), shape, upsample=False)
            f64.check_bits(low.cpu().numpy(), f64.process_mask64(protos, coef, boxes * np.float32(1.0 / s), 1), nm)
    assert uops.process_mask(torch.zeros(8, 4, 4).cuda(), torch.zeros(0, 8).cuda(), torch.zeros(0, 4).cuda(), (16, 16), upsample=True).shape == (0, 16, 16)
