"""-m gpu: head_decode_kernel (ey_head_decode_levels, _xyxy and _nms: DFL softmax + expectation, DGQP quality MLP, anchor decode,
sigmoid scores, fused NMS candidate rows) against the fp64 reference of tests/fp64_attn_ref.py; each case asserts the form that ran
(ey_head_decode_last_variant).

* Bit-exact probe: one-hot DFL logits (every other exp underflows to 0) make each side an integer bin, so with strides 8..64 the
  box rows are exact; class logits in {-65504, 0, 65504} give scores exactly {0, 0.5, 1} with ties (cls_id = first maximal index).
  This pins level, anchor, batch and a_off indexing bit for bit on the vec and scalar staging paths and the fused candidates.
* Bounded checks on general data: per-element fp64 bound and a mean-ulp32 gate (outputs are fp32 in both dtypes), over dtype,
  vec / scalar staging (nc 1, 3, 10, a misaligned nc = 80 view), quality on / off (and clamped), xywh / xyxy, 1-4 levels with
  a_off gaps (columns no level covers stay NaN), LDS above 64 KiB, and the refusal past 160 KiB.
* Fused candidates (with and without pred, with a class mask): boxes, class ids, keys (score_bits << 32 | 0xFFFFFFFF - anchor,
  non-zero exactly when best > conf and the class passes), every slot of the A anchors written."""
import ctypes
import struct
import zlib

import pytest
import torch

pytestmark = pytest.mark.gpu

import fp64_attn_ref as AR  # noqa: E402

VEC, SCALAR, QUAL, NMS = 1, 2, 10, 100
ALL_VARIANTS = {p + q + n for p in (VEC, SCALAR) for q in (0, QUAL) for n in (0, NMS)}
MEAN_ULP32 = 4.0  # gate on the mean |err| / ulp32(magnitude) (fp64_attn_ref.report32)
WORST = {}
F16, F32 = torch.float16, torch.float32
LEVELS = [(9, 11, 8), (5, 6, 16), (3, 3, 32), (1, 2, 64)]  # B = 2: 198, 60, 18 and 4 anchors -- ragged 128-anchor blocks


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _lib():
    from edge_yolo_amd import _lib as L
    return L


def _nhwc(vals, dtype, off=0, pad=0):
    L = _lib()
    B, C, H, W = vals.shape
    buf = L.empty_nhwc(B, C + pad, H, W, dtype, "cuda")
    buf.fill_(float("nan"))
    t = buf[:, off:off + C]
    t.copy_(vals.to(dtype))
    return t


def _decode(dtype, levels, nc, A, pred, xyxy=False, nms=None):
    """Direct call: levels = [(box, cls, stride, q or None, a_off)]; nms = (conf, mask uint8 tensor or None, candidate buffer).
    Returns (return code, variant)."""
    L = _lib()
    lib = L.lib()
    n, B = len(levels), levels[0][0].shape[0]
    IA, FA, PA = ctypes.c_int * n, ctypes.c_float * n, ctypes.c_void_p * n
    Hs, Ws = IA(*[lv[0].shape[2] for lv in levels]), IA(*[lv[0].shape[3] for lv in levels])
    st = FA(*[float(lv[2]) for lv in levels])
    boxp, clsp = PA(*[lv[0].data_ptr() for lv in levels]), PA(*[lv[1].data_ptr() for lv in levels])
    boxcs, clscs = IA(*[L.cstride(lv[0]) for lv in levels]), IA(*[L.cstride(lv[1]) for lv in levels])
    offs = IA(*[int(lv[4]) for lv in levels])
    qa = [PA(*[(lv[3][j].data_ptr() if lv[3] is not None else None) for lv in levels]) for j in range(4)]
    hid = levels[0][3][0].shape[0] if levels[0][3] is not None else 0
    dt = L.dtype_code(dtype)
    if nms is not None:
        conf, mask, buf = nms
        rc = lib.ey_head_decode_levels_nms(dt, B, n, Hs, Ws, st, boxp, boxcs, clsp, clscs, nc, qa[0], qa[1], qa[2], qa[3], hid,
                                           pred.data_ptr() if pred is not None else None, A, offs, float(conf),
                                           mask.data_ptr() if mask is not None else None, buf.data_ptr(), buf.numel(), L.stream())
    else:
        fn = lib.ey_head_decode_levels_xyxy if xyxy else lib.ey_head_decode_levels
        rc = fn(dt, B, n, Hs, Ws, st, boxp, boxcs, clsp, clscs, nc, qa[0], qa[1], qa[2], qa[3], hid, pred.data_ptr(), A, offs, L.stream())
    v = lib.ey_head_decode_last_variant()
    torch.cuda.synchronize()
    return rc, v


def _quality(gen, b2=None):
    w1 = torch.randn(64, 20, generator=gen) * 0.3
    b1 = torch.randn(64, generator=gen) * 0.1
    w2 = torch.randn(64, generator=gen) * 0.3
    b2 = torch.randn(1, generator=gen) * 0.5 if b2 is None else torch.tensor([float(b2)])
    return tuple(t.float().cuda() for t in (w1, b1, w2, b2))


def _levels(dtype, B, nc, shapes, gen, quality=None, cls_off=0, box_vals=None, cls_vals=None, gaps=True, order=None):
    """Level tensors for `shapes` [(H, W, stride)]; quality None / "rand" / "clamp" (b2 = +40 on even levels, -40 on odd ones: q
    pinned to both clamps).  a_off: levels laid out in `order` (default: reversed) with gaps of 3 anchors when `gaps`.
    Returns (levels, A_total, covered column index)."""
    n = len(shapes)
    order = order or list(range(n))[::-1]
    offs, a = [0] * n, 3 if gaps else 0
    for l in order:
        offs[l] = a
        a += shapes[l][0] * shapes[l][1] + (3 if gaps else 0)
    levels = []
    for l, (H, W, s) in enumerate(shapes):
        bv = box_vals[l] if box_vals is not None else torch.randn(B, 64, H, W, generator=gen) * 2.5
        cv = cls_vals[l] if cls_vals is not None else torch.randn(B, nc, H, W, generator=gen) * 3
        q = None
        if quality == "rand":
            q = _quality(gen)
        elif quality == "clamp":
            q = _quality(gen, 40.0 if l % 2 == 0 else -40.0)
        levels.append((_nhwc(bv, dtype), _nhwc(cv, dtype, cls_off, 9 if cls_off else 0), s, q, offs[l]))
    cols = torch.cat([torch.arange(lv[4], lv[4] + lv[0].shape[2] * lv[0].shape[3]) for lv in levels])
    return levels, a, cols


def _note(family, case, rb, mu):
    w = WORST.setdefault(family, [(0.0, ""), (0.0, "")])
    if rb > w[0][0]:
        w[0] = (rb, case)
    if mu > w[1][0]:
        w[1] = (mu, case)


def _check_pred(case, v, pred, levels, nc, A, cols, xyxy):
    y, E, Y = AR.head_decode_ref(levels, nc, A, xyxy)
    gap = torch.ones(A, dtype=torch.bool)
    gap[cols] = False
    assert torch.isnan(pred[:, :, gap.cuda()]).all(), f"{case}: columns no level covers were written"
    c = cols.cuda()
    g, yy, EE, YY = pred[:, :, c], y[:, :, c], E[:, :, c], Y[:, :, c]
    bnd = EE + AR.ulp32(yy)  # the kernel's fp32 arithmetic + one final fp32 rounding (already within E: belt and braces)
    rb, mu = AR.report32(case, v, g, yy, bnd, YY, MEAN_ULP32)
    _note("head decode", case, rb, mu)
    return y, E, Y


def _variant_of(vec, quality, nms):
    return (VEC if vec else SCALAR) + (QUAL if quality else 0) + (NMS if nms else 0)


# ------------------------------------------------------------------------------------------------------------------ bounded
PATHS = [("vec80", 80, 0, True), ("nc1", 1, 0, False), ("nc3", 3, 0, False), ("nc10", 10, 0, False), ("mis80", 80, 1, False)]
BOUNDED = [(dt, p, q, xy, 3) for dt in (F16, F32) for p in PATHS for q in (None, "rand") for xy in (False, True)]
BOUNDED += [(dt, PATHS[i], q, False, nl) for dt in (F16, F32) for i, q, nl in ((0, "rand", 1), (3, None, 2), (0, None, 4), (4, "rand", 4))]
BOUNDED += [(dt, PATHS[i], "clamp", False, 4) for dt in (F16, F32) for i in (0, 2)]
# LDS above 64 KiB (vec: f16 nc 272, f32 nc 136; scalar: f16 nc 250, f32 nc 130)
BOUNDED += [(F16, ("vec272", 272, 0, True), "rand", False, 2), (F32, ("vec136", 136, 0, True), None, False, 2),
            (F16, ("nc250", 250, 0, False), None, True, 2), (F32, ("nc130", 130, 0, False), "rand", False, 2)]


@pytest.mark.parametrize("dtype,path,quality,xyxy,nl", BOUNDED, ids=lambda x: getattr(x, "__name__", None) or str(x))
def test_head_decode_bounded(dtype, path, quality, xyxy, nl):
    name, nc, cls_off, vec = path
    case = f"head decode {str(dtype)[6:]} {name} q={quality} {'xyxy' if xyxy else 'xywh'} levels={nl}"
    gen = _gen("hd", str(dtype), name, quality, xyxy, nl)
    levels, A, cols = _levels(dtype, 2, nc, LEVELS[:nl], gen, quality, cls_off)
    pred = torch.full((2, 4 + nc, A), float("nan"), device="cuda")
    rc, v = _decode(dtype, levels, nc, A, pred, xyxy)
    assert rc == 0, _lib().lib().ey_last_error()
    assert v == _variant_of(vec, quality, False), f"{case}: ran variant {v}"
    y, _, _ = _check_pred(case, v, pred, levels, nc, A, cols, xyxy)
    if quality == "clamp":  # scores = sigmoid(cls) * q with q pinned to 1 - 1e-6f (even levels) and 1e-6f (odd levels)
        for l, lv in enumerate(levels):
            s = torch.sigmoid(AR._rows(lv[1])).transpose(1, 2)
            c = slice(lv[4], lv[4] + lv[0].shape[2] * lv[0].shape[3])
            qv = AR.Q_HI if l % 2 == 0 else AR.Q_LO
            assert torch.allclose(y[:, 4:, c], s * qv, rtol=0, atol=0), f"{case}: reference not clamped"


@pytest.mark.parametrize("dtype,nc", [(F16, 648), (F32, 328)])
def test_head_decode_lds_refusal(dtype, nc):
    """Past 160 KiB of staged class logits the call is refused before anything is launched."""
    levels, A, _ = _levels(dtype, 1, nc, LEVELS[2:3], _gen("hdref", nc))
    pred = torch.full((1, 4 + nc, A), float("nan"), device="cuda")
    rc, v = _decode(dtype, levels, nc, A, pred)
    assert rc == -1 and v == 0 and b"LDS" in _lib().lib().ey_last_error(), (rc, v)
    assert torch.isnan(pred).all(), "refused head decode wrote pred"
    print(f"[exact] head decode {str(dtype)[6:]} nc={nc}: refused, nothing launched")


# --------------------------------------------------------------------------------------------------------- fused candidates
def _cand_views(buf, B, A):
    P = (A + 255) // 256 * 256
    keys = buf[:B * P * 8].view(torch.int64).view(B, P)[:, :A]
    cls_id = buf[B * P * 8:B * P * 12].view(torch.int32).view(B, P)[:, :A]
    box4 = buf[B * P * 12:B * P * 12 + B * 4 * A * 4].view(torch.float32).view(B, 4, A)
    return keys, cls_id, box4


def _cand_buf(B, A):
    nb = _lib().lib().ey_nms_candidates_bytes(B, A)
    return torch.full((nb,), 0xFF, dtype=torch.uint8, device="cuda")


@pytest.mark.parametrize("dtype,path,quality,with_pred,masked", [
    (F16, PATHS[0], "rand", True, True), (F32, PATHS[0], None, False, False), (F16, PATHS[3], "rand", False, True),
    (F32, PATHS[2], "rand", True, False), (F16, PATHS[4], None, True, True), (F32, PATHS[4], "rand", False, True)])
def test_head_decode_candidates(dtype, path, quality, with_pred, masked):
    name, nc, cls_off, vec = path
    B, conf = 2, 0.25
    case = f"head decode nms {str(dtype)[6:]} {name} q={quality} pred={with_pred} mask={masked}"
    gen = _gen("hdnms", str(dtype), name, quality, with_pred, masked)
    levels, A, cols = _levels(dtype, B, nc, LEVELS[:3], gen, quality, cls_off, gaps=False, order=[1, 0, 2])
    mask = (torch.rand(nc, generator=gen) < 0.6).to(torch.uint8).cuda() if masked else None
    pred = torch.full((B, 4 + nc, A), float("nan"), device="cuda") if with_pred else None
    buf = _cand_buf(B, A)
    rc, v = _decode(dtype, levels, nc, A, pred, nms=(conf, mask, buf))
    assert rc == 0, _lib().lib().ey_last_error()
    assert v == _variant_of(vec, quality, True), f"{case}: ran variant {v}"
    if with_pred:
        y, E, Y = _check_pred(case, v, pred, levels, nc, A, cols, False)
    else:
        y, E, Y = AR.head_decode_ref(levels, nc, A, False)
    keys, cls_id, box4 = _cand_views(buf, B, A)
    rb, mu = AR.report32(f"{case} box4", v, box4, y[:, :4], E[:, :4] + AR.ulp32(y[:, :4]), Y[:, :4], MEAN_ULP32)
    _note("head decode", case, rb, mu)
    sc, Esc = y[:, 4:], E[:, 4:] + AR.ulp32(y[:, 4:])
    top2 = sc.topk(min(2, nc), dim=1).values
    best = top2[:, 0]
    arg = sc.argmax(1)                                                     # first maximal index
    ebest = Esc.amax(1)
    assert bool(((cls_id >= 0) & (cls_id < nc)).all()), f"{case}: class id slots not written"
    sure = (top2[:, 0] - top2[:, 1] > 2 * ebest) if nc > 1 else torch.ones_like(best, dtype=torch.bool)
    assert torch.equal(cls_id.long()[sure], arg[sure]), f"{case}: class ids differ where the top-2 gap exceeds twice the bound"
    allowed = mask.bool()[arg] if mask is not None else torch.ones_like(sure)
    want_key = (best > conf) & allowed
    decided = sure & ((best - conf).abs() > ebest)
    nz = keys != 0
    assert torch.equal(nz[decided], want_key[decided]), f"{case}: {int((nz[decided] != want_key[decided]).sum())} keys disagree with best > conf"
    anchor = torch.arange(A, device="cuda").expand(B, A)
    low = keys & 0xFFFFFFFF
    assert torch.equal(low[nz], (0xFFFFFFFF - anchor)[nz]), f"{case}: key low word is not 0xFFFFFFFF - anchor"
    hi = (keys >> 32).to(torch.int32).view(torch.float32).double()
    assert bool(((hi[nz] - best[nz]).abs() <= ebest[nz]).all()), f"{case}: key score bits differ from the best score"
    assert bool((hi[nz] > conf).all()), f"{case}: key for a score <= conf"
    print(f"[fp64] {case} [{v}] keys: {int(nz.sum())} candidates, {int(decided.sum())} of {B * A} anchors decided")


# --------------------------------------------------------------------------------------------------------------- exact probe
def _probe_data(B, nc, shapes, gen):
    """One-hot DFL logits (200 at bin k, 0 elsewhere) and class logits in {-65504, 0, 65504}; some anchors all -65504."""
    box_vals, cls_vals, bins = [], [], []
    for H, W, _ in shapes:
        k = torch.randint(0, 16, (B, 4, H, W), generator=gen)
        bv = torch.zeros(B, 4, 16, H, W)
        bv.scatter_(2, k.unsqueeze(2), 200.0)
        box_vals.append(bv.view(B, 64, H, W))
        bins.append(k)
        c = (torch.randint(-1, 2, (B, nc, H, W), generator=gen) * 65504.0)
        c[:, :, 0, 0] = -65504.0
        cls_vals.append(c)
    return box_vals, cls_vals, bins


def _f32bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


@pytest.mark.parametrize("dtype,nc,cls_off,vec,xyxy", [
    (F16, 80, 0, True, False), (F16, 80, 0, True, True), (F32, 80, 0, True, False), (F16, 10, 0, False, False),
    (F32, 3, 0, False, True), (F16, 80, 1, False, False), (F32, 80, 1, False, True)])
def test_head_decode_exact_probe(dtype, nc, cls_off, vec, xyxy):
    B = 2
    case = f"head decode probe {str(dtype)[6:]} nc={nc} {'vec' if vec else 'scalar'} {'xyxy' if xyxy else 'xywh'}"
    gen = _gen("hdprobe", str(dtype), nc, cls_off, xyxy)
    box_vals, cls_vals, bins = _probe_data(B, nc, LEVELS, gen)
    levels, A, cols = _levels(dtype, B, nc, LEVELS, gen, None, cls_off, box_vals, cls_vals, order=[2, 0, 3, 1])
    want = torch.full((B, 4 + nc, A), float("nan"), dtype=torch.float64)
    for (H, W, s), k, c, lv in zip(LEVELS, bins, cls_vals, levels):
        ax = torch.arange(W).double().view(1, W) + 0.5
        ay = torch.arange(H).double().view(H, 1) + 0.5
        d = k.double()
        x1, y1, x2, y2 = ax - d[:, 0], ay - d[:, 1], ax + d[:, 2], ay + d[:, 3]
        rows = [x1, y1, x2, y2] if xyxy else [(x1 + x2) / 2, (y1 + y2) / 2, x2 - x1, y2 - y1]
        cs = slice(lv[4], lv[4] + H * W)
        for r in range(4):
            want[:, r, cs] = (rows[r] * s).reshape(B, H * W)
        want[:, 4:, cs] = ((c.sign() + 1) / 2).reshape(B, nc, H * W)
    pred = torch.full((B, 4 + nc, A), float("nan"), device="cuda")
    rc, v = _decode(dtype, levels, nc, A, pred, xyxy)
    assert rc == 0 and v == _variant_of(vec, False, False), (rc, v)
    got = pred.cpu().double()
    same = (got == want) | (torch.isnan(got) & torch.isnan(want))
    if not bool(same.all()):
        i = int(torch.nonzero(~same.flatten())[0])
        idx = [int(t) for t in torch.unravel_index(torch.tensor(i), tuple(want.shape))]
        raise AssertionError(f"{case}: {int((~same).sum())} elements differ; first at (b,row,anchor)={idx}: got {float(got.flatten()[i])} "
                             f"want {float(want.flatten()[i])}")
    print(f"[exact] {case} [{v}] pred bit-exact, {int(cols.numel()) * B * (4 + nc)} elements")
    if xyxy:
        return
    # fused candidates on the same data (no gaps: the levels must cover every anchor)
    levels, A, _ = _levels(dtype, B, nc, LEVELS, gen, None, cls_off, box_vals, cls_vals, gaps=False, order=[2, 0, 3, 1])
    want = torch.full((B, 4 + nc, A), float("nan"), dtype=torch.float64)
    for (H, W, s), k, c, lv in zip(LEVELS, bins, cls_vals, levels):
        ax = torch.arange(W).double().view(1, W) + 0.5
        ay = torch.arange(H).double().view(H, 1) + 0.5
        d = k.double()
        rows = [ax + (d[:, 2] - d[:, 0]) / 2, ay + (d[:, 3] - d[:, 1]) / 2, d[:, 0] + d[:, 2], d[:, 1] + d[:, 3]]
        cs = slice(lv[4], lv[4] + H * W)
        for r in range(4):
            want[:, r, cs] = (rows[r] * s).reshape(B, H * W)
        want[:, 4:, cs] = ((c.sign() + 1) / 2).reshape(B, nc, H * W)
    buf = _cand_buf(B, A)
    rc, v = _decode(dtype, levels, nc, A, None, nms=(0.25, None, buf))
    assert rc == 0 and v == _variant_of(vec, False, True), (rc, v)
    keys, cls_id, box4 = (t.cpu() for t in _cand_views(buf, B, A))
    assert torch.equal(box4.double(), want[:, :4]), f"{case}: candidate boxes differ"
    sc = want[:, 4:]
    best, arg = sc.max(1).values, sc.argmax(1)
    assert torch.equal(cls_id.long(), arg), f"{case}: class ids are not the first maximal index"
    wk = torch.zeros(B, A, dtype=torch.int64)
    for b in range(B):
        for a in range(A):
            if best[b, a] > 0.25:
                wk[b, a] = (_f32bits(float(best[b, a])) << 32) | (0xFFFFFFFF - a)
    assert torch.equal(keys, wk), f"{case}: {int((keys != wk).sum())} candidate keys differ"
    print(f"[exact] {case} [{v}] candidates bit-exact, {int((wk != 0).sum())} keys")


def test_variant_coverage():
    """Every variant code is asserted by at least one case of this file (each case asserts its own at run time)."""
    got = {_variant_of(p[3], q, False) for _, p, q, _, _ in BOUNDED}
    got |= {_variant_of(True, False, True), _variant_of(False, False, True), _variant_of(True, True, True), _variant_of(False, True, True)}
    assert got == ALL_VARIANTS, sorted(got ^ ALL_VARIANTS)
    for fam, ((rb, c1), (mu, c2)) in sorted(WORST.items()):
        print(f"[fp64] worst {fam}: err/bound {rb:.3f} ({c1}); mean ulp32 {mu:.3f} ({c2})")
