"""-m gpu: ey_mask_iou (csrc/maskiou.hip) against integer counts in numpy and the host restatement of the reference's fp32 expression
(utils/metrics.py::mask_iou on host arrays, itself pinned to the reference's bits by tests/test_segval_cpu.py).  The operands are 0/1
and the counts integers, so there is no tolerance anywhere: `inter` is compared exactly, `iou` as uint32 views.

Shapes are the smallest at which packing and tiling can go wrong (a wave packs 256 pixels into four 64-pixel words): one pixel, less than
a word, 64 pixels, one more (5x13), more than one block (16x24: 384 pixels, a partial second block), more words than one pack tile of 32
holds and a row length that is no multiple of 4 elsewhere (40x40: 28 words; 160x160: 400 words = 13 tiles, 7 groups of 64), with 0, 1, 63,
64, 65 and 300 predictions and 0, 1, 2, 64, 65 and 300 instances per image (300 in index mode: values above 255).  The operands start at odd
byte offsets (the byte path of the loads) and on 16-byte boundaries (the dword path)."""
import os

import numpy as np
import pytest
import torch

from edge_yolo_amd import _lib as L
from edge_yolo_amd.nn import _ops
from edge_yolo_amd.utils import metrics

pytestmark = pytest.mark.gpu

# (H, W, predictions per image, instances per image)
CASES = [
    (1, 1, [1, 0, 65], [2, 1, 1]),
    (3, 5, [63, 0, 64], [1, 2, 0]),
    (8, 8, [64, 65], [64, 2]),
    (5, 13, [65, 0, 1], [65, 0, 2]),
    (16, 24, [300], [300]),
    (40, 40, [300, 0, 63], [2, 0, 64]),
    (160, 160, [65, 1], [3, 1]),
]
IDS = [f"{h}x{w}-N{'_'.join(map(str, n))}-M{'_'.join(map(str, m))}" for h, w, n, m in CASES]


def make_case(H, W, Ns, Ms, index, seed):
    """-> pred [sum N, HW] uint8, gt stack [sum M, HW] uint8 (index mode: the expansion of the maps), maps [B, HW] int32.
    Rows cycle through sparse, half, full, all-zero and all-one; where an image has both sides, its first ground-truth row gets an
    identical prediction (the first) and its last one a disjoint, complementary one (the last).  Index mode loses one instance completely (area 0)."""
    r = np.random.default_rng(seed)
    HW = H * W
    dens = [0.03, 0.5, 0.97, 0.0, 1.0]
    preds, gts, maps = [], [], []
    for b, (N, M) in enumerate(zip(Ns, Ms)):
        p = np.stack([(r.random(HW) < dens[(i + b) % 5]) for i in range(N)]).astype(np.uint8) if N else np.zeros((0, HW), np.uint8)
        m = np.zeros(HW, np.int32)
        if index:
            m = r.integers(0, M + 1, HW).astype(np.int32) if M else m
            if M > 2:
                m[m == 2] = 3  # instance 2 is painted over completely
            if M and HW > 4:
                m[:2] = [M + 7, -3]  # values outside 1..M belong to no instance
            g = (m[None] == np.arange(1, M + 1)[:, None]).astype(np.uint8)
        else:
            g = np.stack([(r.random(HW) < dens[(i + 2 * b + 1) % 5]) for i in range(M)]).astype(np.uint8) if M else np.zeros((0, HW), np.uint8)
        if N and M:
            p[0] = g[0]
            if N > 1:
                p[N - 1] = 1 - g[M - 1]
        preds.append(p); gts.append(g); maps.append(m)
    return np.concatenate(preds), np.concatenate(gts), np.stack(maps)


def windowed(arr, fill, lead, tail=5):
    """arr as a contiguous view inside a wider flat device buffer filled with `fill`; -> (view, whole buffer, host copy of the buffer)."""
    a = torch.as_tensor(arr).contiguous()
    buf = torch.empty(lead + a.numel() + tail, dtype=a.dtype)
    buf.view(torch.uint8)[:] = fill
    buf[lead:lead + a.numel()] = a.flatten()
    dev = buf.cuda()
    return dev[lead:lead + a.numel()].view(a.shape), dev, buf.numpy().copy()


@pytest.mark.parametrize("aligned", [False, True], ids=["odd-start", "aligned"])
@pytest.mark.parametrize("index", [False, True], ids=["stack", "index"])
@pytest.mark.parametrize("H,W,Ns,Ms", CASES, ids=IDS)
def test_mask_iou_exact(H, W, Ns, Ms, index, aligned):
    """aligned: the byte operands start on a 16-byte boundary, so rows that are 4-byte aligned are read a dword per lane (with H * W a
    multiple of 4 all of them, with 5x13 and 3x5 every fourth); otherwise they start at an odd byte and every load is a byte load."""
    pred, gt, maps = make_case(H, W, Ns, Ms, index, seed=H * 1000 + W + len(Ns))
    B = len(Ns)
    pred_off, gt_off = np.concatenate([[0], np.cumsum(Ns)]), np.concatenate([[0], np.cumsum(Ms)])
    # ---- the expectation: integer counts, then the reference's fp32 expression on the host
    want_i, want = [], []
    for b in range(B):
        g, p = gt[gt_off[b]:gt_off[b + 1]], pred[pred_off[b]:pred_off[b + 1]]
        want_i.append(g.astype(np.int64) @ p.T.astype(np.int64))
        want.append(metrics.mask_iou(g, p) if len(g) and len(p) else np.zeros((len(g), len(p)), np.float32))
        if len(g) and len(p):
            assert want_i[b][0, 0] == g[0].sum() and (len(p) == 1 or want_i[b][-1, -1] == 0)  # the identical and the disjoint pair
    if index and max(Ms) > 2:
        assert any((gt[gt_off[b]:gt_off[b + 1]].sum(1) == 0).any() for b in range(B) if Ms[b] > 2)  # the painted-over instance
    # ---- operands inside wider 0xAB-filled buffers; outputs at odd offsets of sentinel-filled buffers, gaps between images
    dpred, pbuf, pbuf0 = windowed(pred.reshape(-1, H, W), 0xAB, lead=16 if aligned else 3)
    if index:
        dgt, gbuf, gbuf0 = windowed(maps.reshape(B, H, W), 0xAB, lead=3)
    else:
        dgt, gbuf, gbuf0 = windowed(gt.reshape(-1, H, W), 0xAB, lead=32 if aligned else 5)
    out_off, end = [], 1
    for b in range(B):
        out_off.append(end)
        end += Ns[b] * Ms[b] + 3 + 2 * b
    iou = torch.full((end + 4,), float("nan"), device="cuda")
    inter = torch.full((end + 4,), -77, dtype=torch.int32, device="cuda")
    nbytes = max(16, L.lib().ey_mask_iou_workspace_bytes(H, W, int(pred_off[-1]), int(gt_off[-1])))
    ws = torch.full((nbytes,), 0xAB, dtype=torch.uint8, device="cuda")
    _ops.mask_iou(dpred, pred_off, dgt, gt_off, index=index, out_off=out_off, iou=iou, inter=inter, workspace=ws)
    got, got_i = iou.cpu().numpy(), inter.cpu().numpy()
    touched = np.zeros(end + 4, bool)
    for b in range(B):
        n = Ns[b] * Ms[b]
        sl = slice(out_off[b], out_off[b] + n)
        touched[sl] = True
        np.testing.assert_array_equal(got_i[sl].reshape(Ms[b], Ns[b]), want_i[b], err_msg=f"inter, image {b}")
        np.testing.assert_array_equal(got[sl].view(np.uint32).reshape(Ms[b], Ns[b]), want[b].view(np.uint32), err_msg=f"iou bits, image {b}")
    assert np.isnan(got[~touched]).all() and (got_i[~touched] == -77).all(), "wrote outside the matrices"
    np.testing.assert_array_equal(pbuf.cpu().numpy(), pbuf0)
    np.testing.assert_array_equal(gbuf.cpu().numpy(), gbuf0)
    # ---- the same workspace again: identical bytes
    iou2 = torch.full((end + 4,), float("nan"), device="cuda")
    _ops.mask_iou(dpred, pred_off, dgt, gt_off, index=index, out_off=out_off, iou=iou2, workspace=ws)
    np.testing.assert_array_equal(iou2.cpu().numpy().view(np.uint32), got.view(np.uint32))
    # ---- default layout: matrices packed one after the other, no inter buffer
    iou3, off3, none = _ops.mask_iou(dpred, pred_off, dgt, gt_off, index=index)
    assert none is None and iou3.numel() == sum(n * m for n, m in zip(Ns, Ms))
    flat = np.concatenate([w.reshape(-1) for w in want]) if iou3.numel() else np.zeros(0, np.float32)
    np.testing.assert_array_equal(iou3.cpu().numpy().view(np.uint32), flat.view(np.uint32))


def test_reference_cases_on_the_device(golden_dir):
    """metrics.mask_iou on device tensors and ey_mask_iou's index mode: the reference's own bits (tests/golden/segval_ops.npz)."""
    g = np.load(os.path.join(golden_dir, "segval_ops.npz"))
    for tag in g["iou_tags"]:
        n = int(g[f"iou_{tag}_n"])
        a, b = np.unpackbits(g[f"iou_{tag}_gt"], axis=1)[:, :n], np.unpackbits(g[f"iou_{tag}_pred"], axis=1)[:, :n]
        want = g[f"iou_{tag}"]
        for dt in (torch.uint8, torch.float32):  # the reference hands over float masks
            got = metrics.mask_iou(torch.tensor(a).cuda().to(dt), torch.tensor(b).cuda().to(dt))
            assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == want.shape
            np.testing.assert_array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32), err_msg=str(tag))
    r = np.random.default_rng(4)
    for tag in g["ex_tags"]:
        m, nl = g[f"ex_{tag}_map"], int(g[f"ex_{tag}_nl"])
        ex = np.unpackbits(g[f"ex_{tag}"], axis=1)[:, :m.size]  # the reference's expansion
        pred = (r.random((7, m.size)) < 0.4).astype(np.uint8)
        pred[0] = ex[0]
        iou, _, inter = _ops.mask_iou(torch.tensor(pred.reshape(7, *m.shape)).cuda(), [0, 7], torch.tensor(m[None]).cuda(), [0, nl], index=True, inter=True)
        np.testing.assert_array_equal(inter.cpu().numpy().reshape(nl, 7), ex.astype(np.int64) @ pred.T.astype(np.int64))
        np.testing.assert_array_equal(iou.cpu().numpy().view(np.uint32).reshape(nl, 7), metrics.mask_iou(ex, pred).view(np.uint32))
    assert tuple(metrics.mask_iou(torch.zeros(0, 9).cuda(), torch.zeros(4, 9).cuda()).shape) == (0, 4)


def test_wrapper_refusals():
    p = torch.zeros(2, 4, 4, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError):
        _ops.mask_iou(p.float(), [0, 2], p, [0, 2])
    with pytest.raises(ValueError):
        _ops.mask_iou(p, [0, 2], p, [0, 2], index=True)  # the index form takes int32 maps
    with pytest.raises(ValueError):
        _ops.mask_iou(p, [0, 3], p, [0, 2])  # more rows than the tensor holds
    with pytest.raises(ValueError):
        _ops.mask_iou(p, [0, 2], p, [0, 2], iou=torch.zeros(3, device="cuda"))  # output too small
    with pytest.raises(ValueError):
        _ops.mask_iou(p, [0, 2], p, [0, 2], workspace=torch.zeros(8, dtype=torch.uint8, device="cuda"))
