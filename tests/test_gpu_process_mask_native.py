"""-m gpu: ey_process_mask_native (csrc/segment.hip) against the float64 restatement tests/fp64_mask_native_ref.py.

Criterion (derived, not measured): every byte outside the box is 0; inside, the bits equal the fp64 bits wherever |V| > E,
    E = 1.05 * [(nm + 2) u blend(sum|coef proto|) + 8 u max|corner v| + 2 (ex + ey) max|corner v|],  u = 2^-24, e = 4 u max(source coordinate, 1);
pixels with |V| <= E may go either way, and their share of the in-box pixels is capped at 1e-3 per case (a cap, not a tolerance).  The
dyadic probe (identity and power-of-two ratios only: the blend weights are dyadic only there) allows no exclusions.  proto and the
coefficient maps are channel windows of wider NaN-filled buffers, the output a slice of a sentinel-filled buffer at aligned and unaligned
byte offsets; nothing outside the slice may change and every byte inside is 0 or 1."""
import os
import zlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import fp64_mask_native_ref as f64  # noqa: E402
import retina_synth as rs  # noqa: E402

SENT = 0xAB
LEVELS = {1: [(3, 5)], 3: [(4, 6), (2, 3), (1, 2)], 4: [(4, 6), (2, 3), (1, 2), (1, 1)]}
DTYPES = [torch.float32, torch.float16]


def _geo(mh, mw, shape):
    from edge_yolo_amd.nn._ops import mask_geometry
    return mask_geometry((mh, mw), shape)


def _draw(r, shape, dt, dyadic):
    if dyadic:
        return r.integers(-8, 9, shape).astype(np.float32) * np.float32(0.125)
    return rs.gauss(r, shape, dt == torch.float16)


def _window(a_nhwc, dt, lead=8, trail=8):
    """numpy [.., C] -> a channel window [lead, lead + C) of a NaN-filled device buffer, as a logical-NCHW NHWC view."""
    *d, c = a_nhwc.shape
    buf = torch.full((*d, lead + c + trail), float("nan"), dtype=dt, device="cuda")
    buf[..., lead:lead + c] = torch.tensor(a_nhwc).to(dt)
    return buf[..., lead:lead + c].permute(0, 3, 1, 2)


def build(mh, mw, shapes, counts, nm, nl, dt, dyadic=False, seed=0):
    """A batch of len(shapes) images over one proto grid: image b has counts[b] rows and the original shapes[b]."""
    B = len(shapes)
    r = np.random.default_rng([zlib.crc32(repr((mh, mw, shapes, counts, nm, nl, str(dt), dyadic)).encode()), seed])
    proto = _draw(r, (B, mh, mw, nm), dt, dyadic)
    maps = [_draw(r, (B, h, w, nm), dt, dyadic) for h, w in LEVELS[nl]]
    A = sum(h * w for h, w in LEVELS[nl])
    rows, boxes = [], []
    for b, (k, shape) in enumerate(zip(counts, shapes)):
        anchors, off = [], 0
        for h, w in LEVELS[nl]:  # first and last anchor of every level, then random ones
            anchors += [off, off + h * w - 1]
            off += h * w
        anchors = (anchors + r.integers(0, A, max(k, 1)).tolist())[:k]
        rows += [(b, a) for a in anchors]
        boxes.append(rs.boxes_for(r, k, *shape))
    rows = np.array(rows, np.int32).reshape(-1, 2)
    return dict(proto=proto, maps=maps, rows=rows, boxes=np.concatenate(boxes).astype(np.float32).reshape(-1, 4), shapes=list(shapes), counts=list(counts), nm=nm, dt=dt)


def reference(c):
    """-> per image the fp64 result dict (None where the image has no rows)."""
    nm = c["nm"]
    flat = np.concatenate([m.reshape(m.shape[0], -1, nm) for m in c["maps"]], 1)  # [B, A, nm] in concatenated anchor order
    mh, mw = c["proto"].shape[1:3]
    out, o = [], 0
    for b, (k, shape) in enumerate(zip(c["counts"], c["shapes"])):
        sel = slice(o, o + k)
        o += k
        out.append(f64.process_mask_native64(c["proto"][b].transpose(2, 0, 1), flat[b, c["rows"][sel, 1]], c["boxes"][sel], _geo(mh, mw, shape)) if k else None)
    return out


def launch(c, lead=16, extra_rows=3):
    """-> per image the (n_b, H0_b, W0_b) bytes; checks the bytes around the slice and the 0 / 1 range."""
    from edge_yolo_amd.nn import _ops
    dt = c["dt"]
    proto = _window(c["proto"], dt)
    maps = [_window(m, dt) for m in c["maps"]]
    rows = torch.tensor(np.concatenate([c["rows"], np.zeros((extra_rows, 2), np.int32)])).cuda()  # rows beyond N are never read into the output
    boxes = torch.tensor(np.concatenate([c["boxes"], np.tile(np.array([[0, 0, 1e4, 1e4]], np.float32), (extra_rows, 1))])).cuda()
    off = np.concatenate([[0], np.cumsum(c["counts"])]).tolist()
    size = sum(k * h * w for k, (h, w) in zip(c["counts"], c["shapes"]))
    buf = torch.full((lead + size + 64,), SENT, dtype=torch.uint8, device="cuda")
    flat, views = _ops.process_mask_native(proto, maps, rows, boxes, off, c["shapes"], out=buf[lead:lead + size])
    torch.cuda.synchronize()
    assert (size == 0 or flat.data_ptr() == buf.data_ptr() + lead) and len(views) == len(c["shapes"])  # (an empty slice has no address)
    b = buf.cpu().numpy()
    assert (b[:lead] == SENT).all() and (b[lead + size:] == SENT).all(), "bytes around the output slice changed"
    g = b[lead:lead + size]
    assert ((g == 0) | (g == 1)).all(), "a byte inside the slice is neither 0 nor 1"
    got, o = [], 0
    for v, k, (h, w) in zip(views, c["counts"], c["shapes"]):
        assert tuple(v.shape) == (k, h, w) and (k == 0 or v.data_ptr() == buf.data_ptr() + lead + o)
        got.append(g[o:o + k * h * w].reshape(k, h, w))
        o += k * h * w
    return got


def _case_batch(case, dt, dyadic=False):
    """An op case as a batch of two images of its shape: all rows in image 1 (image 0 has none), or split unevenly."""
    mh, mw, h0, w0, nm, N, nl, lead = case
    k = zlib.crc32(repr(case).encode()) % 2
    counts = [0, N] if k else [(2 * N + 2) // 3, N - (2 * N + 2) // 3]
    return build(mh, mw, [(h0, w0), (h0, w0)], counts, nm, nl, dt, dyadic), lead


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f16"])
@pytest.mark.parametrize("case", rs.OP_CASES, ids=rs.case_id)
def test_bits_against_fp64(case, dt):
    c, lead = _case_batch(case, dt)
    got = launch(c, lead)
    und = tot = 0
    for g, ref in zip(got, reference(c)):
        if ref is not None:
            u, t = f64.check_bits(g, ref, case[4], cap=1.0)
            und, tot = und + u, tot + t
    print(f"undecided {und} of {tot} in-box pixels; set bits {sum(int(g.sum()) for g in got)}")
    assert und <= 1e-3 * max(tot, 1)  # the cap of the whole case
    if case[5] >= 17:
        assert tot > 0 and any(g.any() for g in got)


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f16"])
@pytest.mark.parametrize("case", [c for c in rs.OP_CASES if c[:4] in rs.DYADIC], ids=rs.case_id)
def test_dyadic_probe_is_bit_exact(case, dt):
    """Coefficients and protos are small integers / 8 and the blend weights multiples of 1/8: every sum is exact in fp32 in any order."""
    c, lead = _case_batch(case, dt, dyadic=True)
    got = launch(c, lead)
    for g, ref in zip(got, reference(c)):
        if ref is not None:
            np.testing.assert_array_equal(g, ref["bits"])
    assert any(g.any() for g in got) and not all(g.all() for g in got if g.size)


@pytest.mark.parametrize("lead", [16, 3], ids=["aligned", "unaligned"])
def test_ragged_batch_in_one_launch(lead):
    """Three images of different original sizes over one proto grid, the middle one without rows: an upscale, nothing, a downscale."""
    c = build(16, 24, [(37, 91), (50, 50), (9, 13)], [9, 0, 8], 32, 3, torch.float16)
    got = launch(c, lead)
    for g, ref, k in zip(got, reference(c), c["counts"]):
        assert len(g) == k
        if k:
            f64.check_bits(g, ref, 32)
            assert g.any()


def test_out_of_range_rows_give_zero_masks():
    c = build(5, 7, [(23, 31), (23, 31)], [9, 8], 32, 3, torch.float32)
    A = sum(h * w for h, w in LEVELS[3])
    bad = {0: (2, 0), 3: (-1, 1), 5: (0, A), 8: (1, 0), 11: (1, -1), 14: (1, 2 ** 31 - 1), 16: (0, 0)}  # (8: image 1's anchor among image 0's rows; 16: the reverse)
    for i, rw in bad.items():
        c["rows"][i] = rw
    c["boxes"][:] = (-10.0, -10.0, 100.0, 100.0)  # every valid row has a full-image box
    got = np.concatenate(launch(c))
    keep = np.array([i not in bad for i in range(17)])
    assert not got[~keep].any()
    c["rows"][~keep] = [(0 if i < 9 else 1, 0) for i in np.nonzero(~keep)[0]]
    ref = reference(c)
    o = 0
    for r, k in zip(ref, c["counts"]):
        kk = keep[o:o + k]
        f64.check_bits(got[o:o + k][kk], {n: (v[kk] if n != "eps" else v) for n, v in r.items()}, 32)
        o += k
    assert got[keep].any()


def test_nan_box_gives_an_empty_mask():
    c = build(5, 7, [(23, 31)], [4], 8, 1, torch.float32)
    c["boxes"][:] = (-10.0, -10.0, 100.0, 100.0)
    for i in range(3):
        c["boxes"][i, i] = np.nan
    got = launch(c)[0]
    assert not got[:3].any() and got[3].any()


REFUSALS = [(dict(nm=12), NotImplementedError), (dict(nl=5), NotImplementedError), (dict(B=65), NotImplementedError), (dict(mh=1, mw=1, shape=(5, 3)), ValueError),
            (dict(shape=(0, 4)), ValueError), (dict(off=[0, 2, 1]), ValueError), (dict(off=[1, 1, 2]), ValueError)]


@pytest.mark.parametrize("kw,err", REFUSALS, ids=["nm12", "5levels", "B65", "empty_crop", "H0_0", "decreasing", "first_not_0"])
def test_refusals_leave_the_output_untouched(kw, err):
    """Refused before anything is launched: nm, level count and B outside what is built; an empty crop (a 1x1 proto onto 5x3 gives right = 0),
    a target below 1x1, offsets that do not group the N rows by image."""
    from edge_yolo_amd.nn import _ops
    nm, nl, B, mh, mw = kw.get("nm", 8), kw.get("nl", 1), kw.get("B", 2), kw.get("mh", 4), kw.get("mw", 4)
    shape = kw.get("shape", (9, 9))
    proto = torch.zeros(B, mh, mw, nm, device="cuda").permute(0, 3, 1, 2)
    maps = [torch.zeros(B, 2, 2, nm, device="cuda").permute(0, 3, 1, 2) for _ in range(nl)]
    rows = torch.zeros(2, 2, dtype=torch.int32, device="cuda")
    boxes = torch.tensor([[0.0, 0.0, 8.0, 8.0]] * 2, device="cuda")
    off = kw.get("off", [0, 2] + [2] * (B - 1))
    out = torch.full((4096,), SENT, dtype=torch.uint8, device="cuda")
    with pytest.raises(err):
        _ops.process_mask_native(proto, maps, rows, boxes, off, [shape] * B, out=out)
    torch.cuda.synchronize()
    assert bool((out == SENT).all())


def test_out_is_checked():
    from edge_yolo_amd.nn import _ops
    proto = torch.zeros(1, 4, 4, 8, device="cuda").permute(0, 3, 1, 2)
    maps = [torch.zeros(1, 2, 2, 8, device="cuda").permute(0, 3, 1, 2)]
    rows = torch.zeros(2, 2, dtype=torch.int32, device="cuda")
    boxes = torch.tensor([[0.0, 0.0, 8.0, 8.0]] * 2, device="cuda")
    for bad in (torch.zeros(2 * 81 - 1, dtype=torch.uint8, device="cuda"), torch.zeros(2 * 81, dtype=torch.int8, device="cuda"),
                torch.zeros(2, 81, dtype=torch.uint8, device="cuda"), torch.zeros(4 * 81, dtype=torch.uint8, device="cuda")[::2], torch.zeros(2 * 81, dtype=torch.uint8)):
        with pytest.raises(ValueError, match="out="):
            _ops.process_mask_native(proto, maps, rows, boxes, [0, 2], [(9, 9)], out=bad)
    assert _ops.process_mask_native(proto, maps, rows[:0], boxes[:0], [0, 0], [(9, 9)])[0].numel() == 0  # N == 0: nothing is launched


@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
def test_utils_process_mask_native_reference_signature(golden_dir, half):
    """utils.ops.process_mask_native(protos, masks_in, bboxes, shape) on the reference's own cases (tests/golden/retina_ops.npz)."""
    from edge_yolo_amd.utils import ops as uops
    gold = np.load(os.path.join(golden_dir, "retina_ops.npz"))
    dt = torch.float16 if half else torch.float32
    for case in rs.OP_CASES:
        if case[5] == 0:
            continue
        protos, coef, boxes, shape = rs.golden_case(case, half)
        tag = rs.golden_tag(case, half)
        want = rs.unpack(gold[tag + "_bits"], gold[tag + "_shape"])
        got = uops.process_mask_native(torch.tensor(protos).cuda().to(dt), torch.tensor(coef).cuda(), torch.tensor(boxes).cuda(), shape)
        assert got.dtype == torch.uint8 and tuple(got.shape) == want.shape
        got = got.cpu().numpy()
        ref = f64.process_mask_native64(protos, coef, boxes, _geo(*protos.shape[1:], shape))
        f64.check_bits(got, ref, case[4])
        decided = np.abs(ref["v"]) > f64.mask_bound(ref, case[4])
        np.testing.assert_array_equal(got[decided], want[decided], err_msg=tag)  # (the reference's bits meet the same criterion: tests/test_retina_cpu.py)
    assert tuple(uops.process_mask_native(torch.zeros(8, 4, 4).cuda(), torch.zeros(0, 8).cuda(), torch.zeros(0, 4).cuda(), (16, 9)).shape) == (0, 16, 9)
