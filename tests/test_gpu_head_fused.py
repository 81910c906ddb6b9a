"""-m gpu: head_tail_decode_kernel (ey_head_tail_decode_levels_nms: the towers' closing 1x1 convs inside the decode) against the
launches it replaces, and the lean best-class search of both decode kernels (candidates without pred, f16, vec staging;
csrc/head_nms.hip, hd_best_lean) against the kernels' own full loop.

* ey_sigmoid is non-decreasing over all 63 488 finite f16 values in ascending order on the hardware -- the fact the lean search
  stands on (best score = score of the largest logit).
* Lean call (pred = NULL) == keep_pred call (which still scores every class) == lean call with the tunable head_lean = 0, byte for
  byte over keys, class ids and boxes: crafted rows (repeated maxima, neighbouring f16 values around the maximum, saturated
  plateaus, +0 / -0 mixes, subnormals, NaN, +-Inf) and random rows at three scales, with q from the quality head free and pinned
  to either clamp, with and without a class mask, nc 80 and 8.
* Fused == unfused, byte for byte: the same features and weights through ey_conv2d (box tail) + ey_conv_pw_chain (class chain) +
  ey_head_decode_levels_nms and through the fused entry at head_fuse levels 1 and 2; keys, class ids, boxes and (when asked for)
  pred.  Ragged 512-anchor blocks, three levels in one launch, a level of several blocks, channel-offset views of NaN-filled
  buffers, nc 80 / 72, quality head on / off, class mask, saturating weights, all-equal class logits, NaN / Inf features.
* Shapes outside the gate are refused before anything is launched."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

import test_gpu_head_decode_exact as HX  # noqa: E402  (helpers only: direct C-ABI call, NaN-padded NHWC views, candidate views)

F16 = torch.float16


def _finite_f16_ascending():
    neg = torch.arange(0xFBFF, 0x7FFF, -1, dtype=torch.int32)  # -65504 ... -0
    pos = torch.arange(0x0000, 0x7C00, dtype=torch.int32)      # +0 ... 65504
    bits = torch.cat([neg, pos])
    assert bits.numel() == 63488
    return (bits - (bits >= 0x8000).int() * 0x10000).to(torch.int16).view(F16)


def test_sigmoid_monotone_over_f16():
    """Scores of ey_head_decode_levels (quality off: score = ey_sigmoid(logit)) for every finite f16 logit, in logit order."""
    vals = _finite_f16_ascending()
    assert bool((vals.float()[1:] >= vals.float()[:-1]).all())
    nc, H, W = 8, 64, 124
    A = H * W
    assert A * nc == vals.numel()
    cls = vals.view(A, nc).t().reshape(1, nc, H, W)
    box = torch.zeros(1, 64, H, W)
    levels = [(HX._nhwc(box, F16), HX._nhwc(cls, F16), 8, None, 0)]
    assert torch.equal(levels[0][1].permute(0, 2, 3, 1).reshape(-1).cpu(), vals), "logits not laid out in ascending order"
    pred = torch.full((1, 4 + nc, A), float("nan"), device="cuda")
    rc, v = HX._decode(F16, levels, nc, A, pred)
    assert rc == 0 and v == HX.VEC, (rc, v)
    s = pred[0, 4:].t().reshape(-1).cpu()
    assert bool(torch.isfinite(s).all()) and float(s[0]) == 0.0 and float(s[-1]) == 1.0
    d = s[1:] - s[:-1]
    bad = torch.nonzero(d < 0).flatten()
    print(f"[lean] ey_sigmoid over 63488 finite f16 logits: {int((d == 0).sum())} equal neighbours, {bad.numel()} descents")
    assert bad.numel() == 0, f"ey_sigmoid descends at logits {[float(vals[i]) for i in bad[:8]]}"


def _prev16(x):
    """Next lower f16 of each (finite, non-zero) value."""
    b = x.to(F16).view(torch.int16).to(torch.int32) & 0xFFFF
    b = torch.where(b >= 0x8000, b + 1, b - 1)
    return (b - (b >= 0x8000).int() * 0x10000).to(torch.int16).view(F16).float()


def _rows(nc, gen):
    """(N, nc) fp32 class logits (all f16-representable or rounded later)."""
    rows = []
    base = torch.randn(nc, generator=gen) * 2 - 4

    def row(fill=None):
        return base.clone() if fill is None else torch.full((nc,), float(fill))

    idx3 = [2, 5, 7] if nc == 8 else [3, 41, 79]
    for top in (-6.0, -1.25, 0.75, 5.0, 11.0):  # maxima repeated at several indices (first one wins)
        for first in (0, 1):
            r = row()
            r[[first * idx3[0]] + idx3[1:]] = top
            rows.append(r)
    for v in (-9.0, -2.5, -0.001, 6e-8, 6e-5, 0.5, 3.0, 9.0, 12.0, 15.5, 16.5, 17.0, 24.0, 1000.0):  # neighbours of the maximum
        vv = torch.tensor([v]).to(F16).float()
        lo, vv = float(_prev16(vv)), float(vv)
        for order in range(3):
            r = row(-30000.0)
            if order == 0:
                r[1], r[nc - 2] = lo, vv     # the lower neighbour first
            elif order == 1:
                r[1], r[nc - 2] = vv, lo
            else:
                r[0], r[3], r[nc - 1] = lo, vv, vv
            rows.append(r)
            rows.append(-r.flip(0))
    for v in (17.0, -17.0, 30.0, -30.0, 65504.0, -65504.0, 0.0, -0.0):  # plateaus: every class equal
        rows.append(row(v))
    r = row(-65504.0); r[nc - 3] = -65000.0; rows.append(r)
    r = row(20.0); r[2], r[5] = 65504.0, 18.0; rows.append(r)             # different logits, one saturated score
    r = row(-0.0); r[4] = 0.0; rows.append(r)                             # +0 / -0 mixes
    r = row(0.0); r[0] = -0.0; rows.append(r)
    r = row(-3.0); r[3], r[6] = -0.0, 0.0; rows.append(r)
    r = row(-3.0); r[3], r[6] = 0.0, -0.0; rows.append(r)
    r = row(-1.0); r[2], r[6] = 6e-8, -6e-8; rows.append(r)               # subnormals around zero
    for pos in (0, nc // 2, nc - 1):
        for bad in (float("nan"), float("inf"), -float("inf")):
            r = row(); r[pos] = bad; rows.append(r)
            r = row(2.0); r[pos] = bad; r[1] = 7.0; rows.append(r)
    r = row(float("nan")); rows.append(r)
    r = row(float("inf")); rows.append(r)
    r = row(-float("inf")); rows.append(r)
    for scale in (0.5, 4.0, 30.0):
        x = torch.randn(4096, nc, generator=gen) * scale
        tie = torch.rand(4096, generator=gen) < 0.25  # a quarter of the rows: the maximum again at a random index
        j = torch.randint(0, nc, (4096,), generator=gen)
        x[tie, j[tie]] = x.amax(1)[tie]
        rows.extend(x)
    return torch.stack(rows)


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("quality", [None, "rand", "hi", "lo"])
@pytest.mark.parametrize("nc", [80, 8])
def test_lean_best_class_equals_full_loop(nc, quality, masked):
    L = HX._lib()
    gen = HX._gen("lean", nc, quality, masked)
    rows = _rows(nc, gen)
    W = 64
    H = (rows.shape[0] + W - 1) // W
    A = H * W
    rows = torch.cat([rows, torch.randn(A - rows.shape[0], nc, generator=gen) * 3])
    cls = rows.t().reshape(1, nc, H, W)
    box = torch.randn(1, 64, H, W, generator=gen) * 2.5
    q = None if quality is None else HX._quality(gen, {"rand": None, "hi": 40.0, "lo": -40.0}[quality])
    conf = 0.0 if quality == "lo" else 0.25  # (q = 1e-6: nothing passes 0.25)
    levels = [(HX._nhwc(box, F16), HX._nhwc(cls, F16), 8, q, 0)]
    mask = (torch.rand(nc, generator=gen) < 0.6).to(torch.uint8).cuda() if masked else None
    want_v = HX._variant_of(True, q is not None, True)

    def run(pred):
        buf = HX._cand_buf(1, A)
        rc, v = HX._decode(F16, levels, nc, A, pred, nms=(conf, mask, buf))
        assert rc == 0 and v == want_v, (rc, v, L.lib().ey_last_error())
        return HX._cand_views(buf, 1, A)

    lean = run(None)
    full = run(torch.empty((1, 4 + nc, A), device="cuda"))
    assert L.lib().ey_tune_get(b"head_lean") == 1
    try:
        L.check(L.lib().ey_tune_set(b"head_lean", 0), "ey_tune_set")
        off = run(None)
    finally:
        L.check(L.lib().ey_tune_set(b"head_lean", 1), "ey_tune_set")
    for name, a, b, c in zip(("keys", "cls_id", "box4"), lean, full, off):
        for other, t in (("keep_pred", b), ("head_lean=0", c)):
            same = a.contiguous().view(torch.uint8) == t.contiguous().view(torch.uint8)
            assert bool(same.all()), f"nc={nc} q={quality}: {name} of the lean call differ from the {other} call in {int((~same).sum())} bytes"
    print(f"[lean] nc={nc} q={quality} mask={masked}: {A} anchors, {int((lean[0] != 0).sum())} keys, byte-equal to the full loop")


# ------------------------------------------------------------------------------------------------------ fused == unfused
TAIL_BOX, TAIL_BOX_CLS = 3, 4  # EY_HD_TAIL_BOX, EY_HD_TAIL_BOX_CLS


def _tail_decode(dtype, levels, tails, nc, A, pred, nms, fuse_cls, box_cin=64, box_cout=64, cmid=80):
    """Direct call of ey_head_tail_decode_levels_nms: levels = [(box_feat, cls_in, stride, q or None, a_off)], tails = [(box_wp, box_b,
    (w1p, b1, w2p, b2) or None)], nms = (conf, mask or None, candidate buffer).  Returns (return code, variant)."""
    L = HX._lib()
    lib = L.lib()
    n, B = len(levels), levels[0][0].shape[0]
    IA, FA, PA = ctypes.c_int * n, ctypes.c_float * n, ctypes.c_void_p * n
    Hs, Ws = IA(*[lv[0].shape[2] for lv in levels]), IA(*[lv[0].shape[3] for lv in levels])
    st = FA(*[float(lv[2]) for lv in levels])
    boxp, clsp = PA(*[lv[0].data_ptr() for lv in levels]), PA(*[lv[1].data_ptr() for lv in levels])
    boxcs, clscs = IA(*[L.cstride(lv[0]) for lv in levels]), IA(*[L.cstride(lv[1]) for lv in levels])
    ccin = IA(*[lv[1].shape[1] for lv in levels])
    offs = IA(*[int(lv[4]) for lv in levels])
    qa = [PA(*[(lv[3][j].data_ptr() if lv[3] is not None else None) for lv in levels]) for j in range(4)]
    hid = levels[0][3][0].shape[0] if levels[0][3] is not None else 0
    bw, bb = PA(*[t[0].data_ptr() for t in tails]), PA(*[t[1].data_ptr() for t in tails])
    ch = [PA(*[(t[2][j].data_ptr() if t[2] is not None else None) for t in tails]) for j in range(4)]
    conf, mask, buf = nms
    rc = lib.ey_head_tail_decode_levels_nms(L.dtype_code(dtype), B, n, Hs, Ws, st, boxp, boxcs, box_cin, box_cout, bw, bb, clsp, clscs, int(fuse_cls), ccin, cmid,
                                            ch[0], ch[1], ch[2], ch[3], nc, qa[0], qa[1], qa[2], qa[3], hid, pred.data_ptr() if pred is not None else None, A, offs,
                                            float(conf), mask.data_ptr() if mask is not None else None, buf.data_ptr(), buf.numel(), L.stream())
    v = lib.ey_head_decode_last_variant()
    torch.cuda.synchronize()
    return rc, v


class _Level:
    """One pyramid level: features (channel-offset views of NaN-filled wider buffers), the three 1x1 convs' weights, and the logits the
    separate launches (ey_conv2d, ey_conv_pw_chain) compute from them."""

    def __init__(self, B, H, W, nc, data, gen):
        from edge_yolo_amd import _lib as L
        from edge_yolo_amd.nn import _ops as ops
        from edge_yolo_amd.nn.modules.conv import _Packed
        scale = 50.0 if data == "sat" else 1.0
        bf, cf = torch.randn(B, 64, H, W, generator=gen), torch.randn(B, 80, H, W, generator=gen)
        if data == "naninf":
            bf[0, 5, H // 2, 1], bf[B - 1, 40, 0, W - 1] = float("nan"), float("inf")
            cf[0, 7, 0, 0], cf[B - 1, 70, H - 1, W // 2] = float("inf"), float("nan")
        self.bf, self.cf = HX._nhwc(bf, F16, 8, 16), HX._nhwc(cf, F16, 16, 24)
        wb, bb = torch.randn(64, 64, 1, 1, generator=gen) * (0.3 * scale), torch.randn(64, generator=gen)
        w1, b1 = torch.randn(80, 80, 1, 1, generator=gen) * (0.15 * scale), torch.randn(80, generator=gen) * 0.5
        w2, b2 = torch.randn(nc, 80, 1, 1, generator=gen) * (0.25 * scale), torch.randn(nc, generator=gen) - 1.0
        if data == "zero":  # every class logit = the same bias: all classes tie, the first index wins
            w2, b2 = torch.zeros_like(w2), torch.full((nc,), 0.3)
        m1, m2 = _Packed(), _Packed()
        self.box_logits = ops.conv2d(m1, [self.bf], lambda: (wb, bb), 1, 1, 0, L.ACT_NONE)
        assert L.lib().ey_conv_last_variant() >= 3000
        self.cls_logits = L.empty_nhwc(B, nc, H, W, F16, "cuda")
        assert ops.conv_pw_chain(m2, self.cf, lambda: (w1, b1), L.ACT_SILU, lambda: (w2, b2), L.ACT_NONE, self.cls_logits) is not None
        wp, bias, _, _ = ops.packed_conv1x1(m1, self.bf, None)  # (cached by the conv2d above)
        self.tail_box = (wp, bias)
        self.chain = ops.pw_chain_packed(m2, self.cf, None, None)[:4]
        self.keep = (m1, m2)


SHAPES = {"ragged3": (2, [(9, 11, 8), (5, 6, 16), (3, 3, 32)]), "blocks": (3, [(17, 16, 8)])}
FUSED = [(sh, nc, data, quality, with_pred, masked)
         for k, (sh, nc, data) in enumerate((sh, nc, data) for sh in SHAPES for nc in (80, 72) for data in ("normal", "sat", "zero", "naninf"))
         for quality, with_pred, masked in [(("rand", None)[k % 2], bool((k // 2) % 2), bool((k // 4 + k) % 2))]]
assert {q for _, _, _, q, _, _ in FUSED} == {"rand", None} and {p for _, _, _, _, p, _ in FUSED} == {True, False} and {m for *_, m in FUSED} == {True, False}


@pytest.mark.parametrize("shape,nc,data,quality,with_pred,masked", FUSED)
def test_fused_equals_unfused(shape, nc, data, quality, with_pred, masked):
    B, shapes = SHAPES[shape]
    gen = HX._gen("fused", shape, nc, data)
    lv = [_Level(B, H, W, nc, data, gen) for H, W, _ in shapes]
    qs = [HX._quality(gen) if quality else None for _ in shapes]
    offs, A = [], 0
    for H, W, _ in shapes:
        offs.append(A)
        A += H * W
    mask = (torch.rand(nc, generator=gen) < 0.6).to(torch.uint8).cuda() if masked else None
    conf = 0.25

    def run(fuse):
        buf = HX._cand_buf(B, A)
        pred = torch.full((B, 4 + nc, A), float("nan"), device="cuda") if with_pred else None
        if fuse == 0:
            levels = [(l.box_logits, l.cls_logits, s[2], q, o) for l, s, q, o in zip(lv, shapes, qs, offs)]
            rc, v = HX._decode(F16, levels, nc, A, pred, nms=(conf, mask, buf))
            want_v = HX._variant_of(True, quality, True)
        else:
            levels = [(l.bf, l.cf if fuse == 2 else l.cls_logits, s[2], q, o) for l, s, q, o in zip(lv, shapes, qs, offs)]
            tails = [(l.tail_box[0], l.tail_box[1], l.chain if fuse == 2 else None) for l in lv]
            rc, v = _tail_decode(F16, levels, tails, nc, A, pred, (conf, mask, buf), fuse == 2)
            want_v = (TAIL_BOX_CLS if fuse == 2 else TAIL_BOX) + (HX.QUAL if quality else 0) + HX.NMS
        assert rc == 0 and v == want_v, (fuse, rc, v, HX._lib().lib().ey_last_error())
        return HX._cand_views(buf, B, A) + ((pred,) if with_pred else ())

    want = run(0)
    if data in ("normal", "sat"):
        big = max(float(l.cls_logits.float().abs().max()) for l in lv)
        assert (1.0 < big < 40.0) if data == "normal" else big > 100.0, f"{data}: class logits up to {big}"
    if data == "zero":
        assert bool((want[1] == 0).all()), "all-equal class logits: the first class must win"
    for fuse in (1, 2):
        got = run(fuse)
        for name, a, b in zip(("keys", "cls_id", "box4", "pred"), got, want):
            same = a.contiguous().view(torch.uint8) == b.contiguous().view(torch.uint8)
            assert bool(same.all()), f"{shape} nc={nc} {data} head_fuse={fuse}: {name} differ from the unfused launches in {int((~same).sum())} bytes"
    print(f"[fused] {shape} nc={nc} {data} q={quality} pred={with_pred} mask={masked}: {B * A} anchors, {int((want[0] != 0).sum())} keys, levels 1 and 2 byte-equal")


@pytest.mark.parametrize("case", ["nc10", "box32", "misaligned", "levels5", "f32"])
def test_fused_refusals(case):
    """Outside the shape gate the call returns EY_EUNSUPPORTED (or EY_EINVAL) before anything is launched."""
    gen = HX._gen("refuse", case)
    nc = 10 if case == "nc10" else 80
    n = 5 if case == "levels5" else 1
    B, H, W = 1, 4, 5
    lv = _Level(B, H, W, 80, "normal", gen)
    cls_in, fuse_cls = lv.cf, True
    if case == "nc10":
        cls_in, fuse_cls = HX._nhwc(torch.randn(B, 10, H, W, generator=gen), F16, 0, 6), False
    if case == "misaligned":
        cls_in = HX._nhwc(torch.randn(B, 80, H, W, generator=gen), F16, 1, 9)
    A = n * H * W
    levels = [(lv.bf, cls_in, 8, None, i * H * W) for i in range(n)]
    tails = [(lv.tail_box[0], lv.tail_box[1], lv.chain if fuse_cls else None)] * n
    buf = HX._cand_buf(B, A)
    rc, v = _tail_decode(torch.float32 if case == "f32" else F16, levels, tails, nc, A, None, (0.25, None, buf), fuse_cls, box_cin=32 if case == "box32" else 64)
    assert rc in (-1, -2) and v == 0, (case, rc, v)
    assert bool((buf == 0xFF).all()), f"{case}: a refused call wrote the candidate buffer"
    print(f"[fused] {case}: refused ({rc}): {HX._lib().lib().ey_last_error().decode()}")
