"""-m gpu: ey_mask_contours through nn._ops.mask_contours equals the restatement of cv2.findContours (tests/contours_ref.py) exactly, as
integers, on every synthetic mask (tests/contours_synth.py): all masks of one size in one call, uint8 and bool, with and without boxes,
with the first launch's room forced down so that the second launch runs; 70 masks in one call; the input stays bit for bit what it was;
no masks work; and utils.ops.masks2segments and Masks.xy / xyn on the device equal the reference's own output (tests/golden/contours_ops.npz)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import contours_ref as ref  # noqa: E402
import contours_synth as cs  # noqa: E402

NAMES = [c[0] for c in cs.cases()]


def _boxes(idx):
    """xyxy with fractions around the set pixels, as process_mask crops: column r is kept where x1 <= r < x2."""
    out = []
    for i in idx:
        ys, xs = np.nonzero(cs.cases()[i][1])
        out.append([xs.min() - 0.5, ys.min() - 0.25, xs.max() + 0.5, ys.max() + 0.75] if len(ys) else [2.5, 1.5, 2.5, 1.5])
    return torch.tensor(out, dtype=torch.float32, device="cuda")


@pytest.mark.parametrize("room", [None, (16, 4), (1, 1024)], ids=["default", "4-vertices", "1-contour"])
@pytest.mark.parametrize("boxes", [False, True], ids=["whole", "boxes"])
@pytest.mark.parametrize("dtype", [torch.uint8, torch.bool], ids=["uint8", "bool"])
def test_every_mask_exactly(dtype, boxes, room):
    from edge_yolo_amd.nn import _ops
    kw = {} if room is None else {"_contour_capacity": room[0], "_vertex_capacity": room[1]}
    seen = 0
    for shape, idx in cs.by_shape().items():
        host = np.stack([cs.cases()[i][1] for i in idx])
        x = torch.tensor(host).cuda()
        x = (x != 0) if dtype == torch.bool else x
        before = x.clone()
        got = _ops.mask_contours(x, boxes=_boxes(idx) if boxes else None, **kw)
        assert torch.equal(x, before) and x.dtype == dtype
        assert len(got) == len(idx)
        for i, g in zip(idx, got):
            assert cs.same(g, cs.expected(i)), NAMES[i]
            seen += len(g)
    assert seen > 200


def test_seventy_masks_in_one_call():
    from edge_yolo_amd.nn import _ops
    rng = np.random.default_rng(11)
    host = (rng.random((70, 16, 19)) < rng.uniform(0.25, 0.9, (70, 1, 1))).astype(np.uint8)
    want = [ref.find_contours(m) for m in host]
    x = torch.tensor(host).cuda()
    for kw in ({}, {"_vertex_capacity": 4}):
        got = _ops.mask_contours(x, **kw)
        assert len(got) == 70 and all(cs.same(g, w) for g, w in zip(got, want))
    assert torch.equal(x.cpu(), torch.tensor(host))


def test_no_masks_and_refusals():
    from edge_yolo_amd import _lib
    from edge_yolo_amd.nn import _ops
    assert _ops.mask_contours(torch.zeros((0, 5, 7), dtype=torch.uint8, device="cuda")) == []
    assert _ops.mask_contours(torch.zeros((0, 5, 7), dtype=torch.bool, device="cuda"), boxes=torch.zeros((0, 4), device="cuda")) == []
    x = torch.ones((2, 6, 8), dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="contiguous"):
        _ops.mask_contours(x[:, :, ::2])
    with pytest.raises(ValueError, match="uint8 or bool"):
        _ops.mask_contours(x.float())
    with pytest.raises(ValueError, match="boxes"):
        _ops.mask_contours(x, boxes=torch.zeros((3, 4), device="cuda"))
    with pytest.raises(_lib.HipLibraryError):
        _ops.mask_contours(x.cpu())
    with pytest.raises(ValueError, match="out="):
        _ops.mask_contours(x, out=(torch.zeros(2, 4), torch.zeros(2, 4, 2), torch.zeros(2, 4)))
    out = (torch.empty((2, 2), dtype=torch.int32, device="cuda"), torch.empty((2, 8, 2), dtype=torch.int32, device="cuda"), torch.empty((2, 4), dtype=torch.int32, device="cuda"))
    got = _ops.mask_contours(x, out=out)
    assert [[c.tolist() for c in g] for g in got] == [[[[0, 0], [0, 5], [7, 5], [7, 0]]]] * 2
    assert out[2].cpu().tolist() == [[1, 4, 0, 0]] * 2 and out[0][:, 0].cpu().tolist() == [4, 4]


def test_segments_and_masks_equal_the_reference():
    from edge_yolo_amd.engine.results import Masks
    from edge_yolo_amd.utils import ops
    golden = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "contours_ops.npz"))
    for shape, idx in cs.by_shape().items():
        x = torch.tensor(np.stack([cs.cases()[i][1] for i in idx])).cuda()
        for strategy in ("all", "largest"):
            for data in (x, x.float() * 0.5 + (x != 0)):  # (a float mask is set where its integer part is not 0: 1.5 here)
                got = ops.masks2segments(data, strategy)
                assert len(got) == len(idx)
                for i, g in zip(idx, got):
                    want = golden[f"seg_{strategy}_{i}"]
                    assert g.dtype == np.float32 and g.shape == want.shape and np.array_equal(g, want), (NAMES[i], strategy)
    j = 0
    while f"masks{j}_idx" in golden:
        idx, orig = golden[f"masks{j}_idx"], tuple(int(v) for v in golden[f"masks{j}_orig"])
        m = Masks(torch.tensor(np.stack([cs.cases()[int(i)][1] for i in idx])).cuda(), orig)
        for key in ("xy", "xyn"):
            got = getattr(m, key)
            assert [len(g) for g in got] == golden[f"masks{j}_len"].tolist()
            cat = np.concatenate(got)
            assert cat.dtype == np.float32 and np.array_equal(cat, golden[f"masks{j}_{key}"]), (j, key)
        assert len(m[1:].xy) == len(idx) - 1 and np.array_equal(m[1:].xy[0], m.xy[1])
        j += 1
    assert j >= 5
