"""-m gpu: ey_mask_prompt and ey_scale_masks against the float64 restatement (tests/fp64_fastsam_ref.py), per element, with bounds
derived from the kernels' summation order (f64.area_bound, f64.iou_bound), not measured.  Areas are sums of non-negative terms, so the
bound is relative; with original == mask size every weight is 1 and the areas are exact integers.  `best` must be the float64 argmax
(the generator guarantees a gap of 1e-3, far above the propagated bound, which is asserted here too); exact ties go to the lower index;
`hit` is exact at the robust points the cases use.  Outputs sit inside sentinel-filled wider buffers; nothing outside may be written,
a second run gives the same bits, and refusals leave everything untouched."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import fastsam_synth as fs  # noqa: E402
import fp64_fastsam_ref as f64  # noqa: E402

PAD = 3  # sentinel elements around / behind every output


def _buffers(B, N, P, Q, dev):
    """-> (out dict of views for _ops.mask_prompt, the flat sentinel-filled buffers behind them)."""
    ld = N + PAD
    flat = {"full": torch.full((N + 2 * PAD,), float("nan"), device=dev), "keep": torch.full((N + 2 * PAD,), 0xAB, dtype=torch.uint8, device=dev),
            "inter": torch.full((P * ld + 2 * PAD,), float("nan"), device=dev), "iou": torch.full((P * ld + 2 * PAD,), float("nan"), device=dev),
            "best": torch.full((B * P + 2 * PAD,), -77, dtype=torch.int32, device=dev), "hit": torch.full((Q * ld + 2 * PAD,), 0xAB, dtype=torch.uint8, device=dev)}
    # (float32 / int32 views must stay 4-byte aligned: their offset PAD counts elements)
    out = {"full": flat["full"][PAD:PAD + N], "keep": flat["keep"][PAD:PAD + N]}
    if P:
        out.update(inter=flat["inter"][PAD:PAD + P * ld].view(P, ld), iou=flat["iou"][PAD:PAD + P * ld].view(P, ld), best=flat["best"][PAD:PAD + B * P].view(B, P))
    if Q:
        out["hit"] = flat["hit"][PAD:PAD + Q * ld].view(Q, ld)
    return out, flat


def _untouched(flat, out, N, P, Q):
    for k, t in flat.items():
        t = t.cpu()
        edge = torch.cat([t[:PAD], t[len(t) - PAD:]])
        assert bool(torch.isnan(edge).all()) if t.is_floating_point() else bool((edge == (0xAB if t.dtype == torch.uint8 else -77)).all()), k
    for k in ("inter", "iou", "hit"):
        if k in out:
            tail = out[k][:, N:].cpu()
            assert bool(torch.isnan(tail).all()) if tail.is_floating_point() else bool((tail == 0xAB).all()), k


@pytest.mark.parametrize("tag", list(fs.OP_CASES))
def test_mask_prompt_vs_fp64(tag):
    from edge_yolo_amd.nn import _ops
    c = fs.op_case(tag)
    B, P, Q = len(c["shapes"]), len(c["boxes"]), len(c["points"])
    off = np.concatenate([[0], np.cumsum(c["counts"])]).tolist()
    N = off[-1]
    masks = torch.tensor(np.concatenate(c["masks"]) * 255 if tag.startswith("same") else np.concatenate(c["masks"])).cuda()  # (any non-zero byte is set)
    kw = dict(bboxes=c["boxes"] if P else None, points=c["points"] if Q else None, labels=c["labels"] if Q else None)
    out, flat = _buffers(B, N, P, Q, masks.device)
    _ops.mask_prompt(masks, off, c["shapes"], out=out, **kw)
    torch.cuda.synchronize()
    _untouched(flat, out, N, P, Q)
    first = {k: v.clone() for k, v in flat.items()}
    ref = f64.prompt64(c["masks"], c["shapes"], c["boxes"], c["points"], c["labels"])
    got = {k: v.cpu().numpy() for k, v in out.items()}
    for b, r in enumerate(ref):
        lo, hi = off[b], off[b + 1]
        if r is None:
            assert hi == lo and (not P or (got["best"][b] == -1).all())
            continue
        exact = tuple(c["shapes"][b]) == tuple(c["mask_hw"])
        e = 0.0 if exact else f64.area_bound(c["mask_hw"], c["shapes"][b])
        full = got["full"][lo:hi].astype(np.float64)
        print(f"{tag} image {b}: bound {e:.3e}, full max rel err {float((np.abs(full - r['full']) / r['full']).max()):.3e}")
        assert (np.abs(full - r["full"]) <= e * r["full"]).all()
        if P:
            inter, iou = got["inter"][:, lo:hi].astype(np.float64), got["iou"][:, lo:hi].astype(np.float64)
            print(f"   inter max rel err {float((np.abs(inter - r['inter']) / np.maximum(r['inter'], 1e-300)).max()):.3e}, iou max abs err {float(np.abs(iou - r['iou']).max()):.3e}")
            assert (np.abs(inter - r["inter"]) <= e * r["inter"]).all()
            ib = f64.iou_bound(r["inter"], r["full"][None], r["area"][:, None], e)
            assert (np.abs(iou - r["iou"]) <= ib).all()
            if c["dup"] and b == 0:  # the twins get the same bits, the lower index wins
                a, d = c["dup"]
                assert got["iou"][0, lo + a] == got["iou"][0, lo + d] and got["inter"][0, lo + a] == got["inter"][0, lo + d] and got["best"][b, 0] == a
            else:
                assert (r["gap"] > 2 * ib.max(1)).all()  # decidable: the argmax cannot depend on the rounding
                np.testing.assert_array_equal(got["best"][b], r["best"])
        if Q:
            np.testing.assert_array_equal(got["hit"][:, lo:hi].astype(bool), r["hit"])
            assert set(np.unique(got["hit"][:, lo:hi])) <= {0, 1}
        np.testing.assert_array_equal(got["keep"][lo:hi].astype(bool), r["keep"])
        assert set(np.unique(got["keep"][lo:hi])) <= {0, 1}
        if exact:
            assert (full == np.round(full)).all()
    _ops.mask_prompt(masks, off, c["shapes"], out=out, **kw)  # the same bits again
    torch.cuda.synchronize()
    for k, v in flat.items():
        assert torch.equal(v.view(torch.uint8), first[k].view(torch.uint8)), k
    plain = _ops.mask_prompt(masks, off, c["shapes"], **kw)  # the wrapper's own buffers: the same values
    for k, v in plain.items():
        assert torch.equal(v.view(torch.uint8), (out[k][:, :N] if k in ("inter", "iou", "hit") else out[k]).contiguous().view(torch.uint8)), k


def test_mask_position_does_not_change_the_bits():
    """A mask scores the same wherever it lies in memory: 37 x 53 masks start at every byte alignment."""
    from edge_yolo_amd.nn import _ops
    c = fs.op_case("odd_37x53")
    m = torch.tensor(c["masks"][0]).cuda()
    a = _ops.mask_prompt(m, [0, 12], c["shapes"][:1], c["boxes"], c["points"], c["labels"])
    rolled = torch.cat([m[5:], m[:5]])
    b = _ops.mask_prompt(rolled, [0, 12], c["shapes"][:1], c["boxes"], c["points"], c["labels"])
    assert torch.equal(torch.cat([a["full"][5:], a["full"][:5]]).view(torch.int32), b["full"].view(torch.int32))
    assert torch.equal(torch.cat([a["inter"][:, 5:], a["inter"][:, :5]], 1).view(torch.int32), b["inter"].view(torch.int32))


def test_mask_prompt_refusals_leave_the_outputs_untouched():
    from edge_yolo_amd import _lib as L
    from edge_yolo_amd.nn import _ops
    c = fs.op_case("same_64x96")
    masks = torch.tensor(c["masks"][0]).cuda()
    bad = [dict(bboxes=[[5, 5, 5, 9]]), dict(bboxes=[[5, 9, 8, 9]]), dict(bboxes=[[-1, 0, 4, 4]]), dict(points=[[96, 3]], labels=[1]), dict(points=[[3, 64]], labels=[1]),
           dict(points=[[-1, 3]], labels=[1]), dict()]
    for kw in bad:
        P, Q = len(kw.get("bboxes", [])), len(kw.get("points", []))
        out, flat = _buffers(1, 12, P, Q, masks.device)
        before = {k: v.clone() for k, v in flat.items()}
        with pytest.raises(L.HipLibraryError):
            _ops.mask_prompt(masks, [0, 12], [(64, 96)], out=out, **kw)
        torch.cuda.synchronize()
        for k, v in flat.items():
            assert torch.equal(v.view(torch.uint8), before[k].view(torch.uint8)), (kw, k)
    for kw in (dict(bboxes=[[0, 0, 4, 4]] * 33), dict(points=[[1, 1]] * 33, labels=[1] * 33), dict(bboxes=[[0, 0, 40000, 4]])):
        P, Q = len(kw.get("bboxes", [])), len(kw.get("points", []))
        out, flat = _buffers(1, 12, P, Q, masks.device)
        before = {k: v.clone() for k, v in flat.items()}
        with pytest.raises(NotImplementedError):
            _ops.mask_prompt(masks, [0, 12], [(64, 96)], out=out, **kw)
        torch.cuda.synchronize()
        for k, v in flat.items():
            assert torch.equal(v.view(torch.uint8), before[k].view(torch.uint8)), (kw, k)
    with pytest.raises(ValueError):
        _ops.mask_prompt(masks.float(), [0, 12], [(64, 96)], bboxes=[[0, 0, 4, 4]])
    with pytest.raises(ValueError):
        _ops.mask_prompt(masks, [0, 13], [(64, 96)], bboxes=[[0, 0, 4, 4]])


@pytest.mark.parametrize("kind", ["u8", "f32", "f16"])
@pytest.mark.parametrize("tag,shape,target,padding", fs.SCALE_CASES, ids=[c[0] for c in fs.SCALE_CASES])
def test_scale_masks_vs_fp64(tag, shape, target, padding, kind):
    """ey_scale_masks: four roundings on the longest path (product, sum, product, sum), each relative to the sum of the absolute terms;
    f16 output adds one rounding to half precision (2^-11 relative, 2^-25 absolute below the normal range)."""
    from edge_yolo_amd.utils import ops as uops
    x = fs.scale_input(tag, shape, kind)
    dt = {"u8": torch.uint8, "f32": torch.float32, "f16": torch.float16}[kind]
    got = uops.scale_masks(torch.tensor(x).to(dt).cuda(), target, padding=padding)
    assert got.dtype == (torch.float32 if kind == "u8" else dt) and tuple(got.shape) == (*shape[:2], *target)
    want, mag = f64.scale_masks64(x, target, padding=padding), f64.scale_masks64(np.abs(x.astype(np.float64)), target, padding=padding)
    bound = 4 * f64.U * mag * 1.001
    if kind == "f16":
        bound = bound + (np.abs(want) + bound) * 2.0 ** -11 + 2.0 ** -25
    err = np.abs(got.float().cpu().numpy().astype(np.float64) - want)
    print(f"{tag} {kind}: max err {float(err.max()):.3e}, max bound {float(bound.max()):.3e}")
    assert (err <= bound).all()
    if tuple(shape[2:]) == tuple(target) and padding:
        np.testing.assert_array_equal(got.float().cpu().numpy(), x.astype(np.float32))  # identity: a copy


def test_scale_masks_matches_the_reference_and_bool(golden_dir):
    import os
    from edge_yolo_amd.utils import ops as uops
    g = np.load(os.path.join(golden_dir, "fastsam_ops.npz"))
    for tag, shape, target, padding in fs.SCALE_CASES:
        x = fs.scale_input(tag, shape, "f32")
        got = uops.scale_masks(torch.tensor(x).cuda(), target, padding=padding).cpu().numpy()
        step = int(g[tag + "_step"])
        mag = f64.scale_masks64(np.abs(x.astype(np.float64)), target, padding=padding)[..., ::step, ::step]
        assert (np.abs(got[..., ::step, ::step].astype(np.float64) - g[tag]) <= float(g[tag + "_err"]) + 4 * f64.U * mag * 1.001).all(), tag
    m = torch.tensor(fs.scale_input("sm_64x96_50x75", (2, 2, 64, 96), "u8")).cuda()
    assert torch.equal(uops.scale_masks(m.bool(), (50, 75)), uops.scale_masks(m, (50, 75)))
