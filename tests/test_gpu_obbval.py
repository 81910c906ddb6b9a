"""-m gpu: obb validation on the device.  ey_nms_rotated_ml against the reference's kept (anchor, class) lists and rows (tests/golden/
obbval_ops.npz: every column's float64 margin exceeds 1e-3 and the scores are distinct, so the comparison is bit for bit), ey_probiou_batch
against ey_probiou (bit for bit) and float64 (the 4 E + 2 ulp rule of tests/test_gpu_obb_exact.py), and yolo11n-obb through
`model.val(loader, validator=OBBValidator)` against the reference's OBBValidator on the same weights and batch (obbval_case.npz)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import fp64_obb_ref as f64  # noqa: E402
import fp64_obbval_ref as f64v  # noqa: E402
import obb_synth  # noqa: E402
import obbval_synth as S  # noqa: E402
import synthdata as synth  # noqa: E402

LAYER_TOL = dict(rtol=1e-4, atol=2e-4)  # tests/test_gpu_obb_model.py, fp32 layers


@pytest.fixture(scope="module")
def ops_g(golden_dir):
    return np.load(os.path.join(golden_dir, "obbval_ops.npz"))


@pytest.fixture(scope="module")
def case_g(golden_dir):
    return np.load(os.path.join(golden_dir, "obbval_case.npz"))


def _run(pred, case, max_det=None):
    from edge_yolo_amd.utils import ops as uops
    return uops.nms_rotated_multi_label(pred, case["conf"], case["iou"], case["classes"], case["agnostic"], max_det or case["max_det"], nc=case["nc"],
                                        max_nms=case["max_nms"])


# ------------------------------------------------------------------------------------------------------------------ ey_nms_rotated_ml
@pytest.mark.parametrize("case", S.NMS_CASES, ids=[c["tag"] for c in S.NMS_CASES])
def test_nms_rotated_ml_against_the_reference(ops_g, case):
    tag, A, nc = case["tag"], case["A"], case["nc"]
    assert float(ops_g[tag + "_margin"]) > S.MARGIN
    pred = S.nms_case(case, int(ops_g[tag + "_seed"]))
    dev = pred.cuda()
    rows, count, index = (t.cpu().numpy() for t in _run(dev, case))
    frows, fcount, findex = (t.cpu().numpy() for t in _run(dev, case, max_det=A * nc))  # every kept column
    B = pred.shape[0]
    assert rows.shape == (B, case["max_det"], 7) and count.shape == (B,) and index.shape == (B, case["max_det"]) and rows.dtype == np.float32
    for b in range(B):
        kept = ops_g[f"{tag}_kept{b}"]  # the reference's kept (anchor, class) pairs in its order
        nk, k = int(fcount[b]), int(count[b])
        print(f"{tag} image {b}: {int(ops_g[f'{tag}_total{b}'])} candidates, kept {nk}, reference {len(kept)}")
        assert nk == len(kept) and k == min(nk, case["max_det"])
        np.testing.assert_array_equal(findex[b, :nk], kept[:, 0], err_msg=f"{tag} image {b}: anchors")
        np.testing.assert_array_equal(frows[b, :nk, 5], kept[:, 1].astype(np.float32), err_msg=f"{tag} image {b}: classes")
        np.testing.assert_array_equal(index[b, :k], kept[:k, 0])
        np.testing.assert_array_equal(rows[b, :k], ops_g[f"{tag}_rows{b}"])  # bit for bit the reference's rows
        np.testing.assert_array_equal(rows[b, :k], frows[b, :k])
        assert (index[b, k:] == -1).all() and (rows[b, k:] == 0).all() and (findex[b, nk:] == -1).all() and (frows[b, nk:] == 0).all()
    if case["triple"]:  # one anchor, three classes: three rows that share the box, or the best class alone when agnostic
        same = index[0, :int(count[0])] == S.TRIPLE_ANCHOR
        assert int(same.sum()) == (1 if case["agnostic"] else 3)
        assert len({tuple(r[[0, 1, 2, 3, 6]]) for r in rows[0, :int(count[0])][same]}) == 1
    if case["classes"] is not None:
        assert set(rows[0, :int(count[0]), 5].astype(int)) <= set(case["classes"])


def test_nms_rotated_ml_cases_cover_the_kernel_paths(ops_g):
    """what the cases are there for: the 256-wide tile crossed, a cut inside an anchor's classes, exactly max_nms and one more, an empty
    image inside a batch, max_det below the kept count, and a select over thousands of keys."""
    t = S.NMS_BY_TAG
    assert int(ops_g["ml_all270_total0"]) == 270 > 256
    assert int(ops_g["ml_cut_total0"]) == 320 > t["ml_cut"]["max_nms"]
    assert int(ops_g["ml_exact_max_nms_total0"]) == t["ml_exact_max_nms"]["max_nms"] and int(ops_g["ml_max_nms_plus1_total0"]) == t["ml_max_nms_plus1"]["max_nms"] + 1
    assert int(ops_g["ml_b3_empty_total1"]) == 0 and int(ops_g["ml_b3_empty_total0"]) > 0 and int(ops_g["ml_b3_empty_total2"]) > 0
    assert len(ops_g["ml_max_det5_kept0"]) > t["ml_max_det5"]["max_det"] == 5
    assert int(ops_g["ml_large_total0"]) == 6000 > t["ml_large"]["max_nms"] == 4096
    assert any(int(ops_g[f"{c['tag']}_total0"]) > c["counts"][0] for c in S.NMS_CASES if c["mode"] == "hot")  # anchors with several classes


def test_nms_rotated_ml_graph_replay_and_rerun(ops_g):
    case = S.NMS_BY_TAG["ml_b3_empty"]
    pred = S.nms_case(case, int(ops_g["ml_b3_empty_seed"])).cuda()
    eager = [t.clone() for t in _run(pred, case)]
    again = _run(pred, case)
    for a, b in zip(eager, again):
        assert torch.equal(a, b)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _run(pred, case)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = _run(pred, case)
    for t in out:
        t.zero_()
    g.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager, out):
        assert torch.equal(a, b)
    assert int(out[1].sum()) > 0


def test_nms_rotated_ml_large_rerun_same_bytes(ops_g):
    case = S.NMS_BY_TAG["ml_large"]
    pred = S.nms_case(case, int(ops_g["ml_large_seed"])).cuda()
    a, b = _run(pred, case), _run(pred, case)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


@pytest.mark.parametrize("max_nms", [30000, 97])
def test_nms_rotated_ml_equal_scores(max_nms):
    """Equal scores are ordered by ascending anchor * nc + class, and a max_nms cut among equal scores takes the lower ones: the low 32 key
    bits of the select.  The goldens have no ties (the reference's argsort leaves them unspecified), so this is against the float64
    restatement, which implements the rule; a column within the ProbIoU bound of the threshold is left out of the comparison."""
    from edge_yolo_amd.utils import ops as uops
    case = dict(S.NMS_BY_TAG["ml_all270"], conf=0.25, iou=0.45)
    pred = S.nms_case(case, 0)
    A, nc = case["A"], case["nc"]
    pred[:, 4:4 + nc] = torch.round(pred[:, 4:4 + nc] * 8) / 8 + 0.26  # groups of equal scores, all above conf
    p = pred.numpy()
    assert len(np.unique(p[0, 4:4 + nc])) < 12
    ora = f64v.nms_rotated_ml64(p, case["conf"], case["iou"], None, False, A * nc, max_nms, S.MAX_WH)[0]
    if max_nms < A * nc:  # the cut falls inside a group of equal scores
        allc = f64v.candidates_ml(p[0], nc, case["conf"], None, A * nc)
        assert allc[2][max_nms - 1] == allc[2][max_nms]
    rows, count, index = (t.cpu().numpy() for t in uops.nms_rotated_multi_label(pred.cuda(), case["conf"], case["iou"], None, False, A * nc, nc=nc, max_nms=max_nms))
    k = int(count[0])
    got = list(zip(index[0, :k].tolist(), rows[0, :k, 5].astype(int).tolist()))
    order = list(zip(ora["anchor"].tolist(), ora["cls"].tolist()))
    pos = {ac: i for i, ac in enumerate(order)}
    assert set(got) <= set(order) and all(pos[got[i]] < pos[got[i + 1]] for i in range(k - 1))  # survivors only, in the rule's order
    decided = ora["margin"] > 4.0 * 5e-5 + 2.0 ** -23  # 4 E + 2 ulp with E = 5e-5: the generator measured E <= 2.1e-5 on these scenes
    assert (~decided).sum() <= 0.01 * len(order)
    gpu_keep = np.array([ac in set(got) for ac in order])
    np.testing.assert_array_equal(gpu_keep[decided], ora["keep"][decided])
    print(f"equal scores, max_nms {max_nms}: {len(order)} candidates, kept {k}, undecided {int((~decided).sum())}")


def test_single_label_rotated_nms_is_unchanged(golden_dir):
    """nms_device(rotated=True) on an existing case still gives the reference's rows, and with nc == 1 the two entry points agree."""
    from edge_yolo_amd.utils import ops as uops
    g = np.load(os.path.join(golden_dir, "obb_ops.npz"))
    case = obb_synth.NMS_BY_TAG["nms_b3"]
    pred = obb_synth.nms_case(case, int(g["nms_b3_seed"])).cuda()
    rows, count, index = uops.nms_device(pred, case["conf"], case["iou"], None, False, case["max_det"], nc=case["nc"], max_nms=case["max_nms"], rotated=True)
    for b in range(3):
        np.testing.assert_array_equal(rows[b, :int(count[b])].cpu().numpy(), g[f"nms_b3_rows{b}"])
    one = torch.cat([pred[:, :4], pred[:, 4:4 + case["nc"]].amax(1, keepdim=True), pred[:, -1:]], 1).contiguous()
    sl = uops.nms_device(one, case["conf"], case["iou"], None, False, case["max_det"], nc=1, max_nms=case["max_nms"], rotated=True)
    ml = uops.nms_rotated_multi_label(one, case["conf"], case["iou"], None, False, case["max_det"], nc=1, max_nms=case["max_nms"])
    for a, b in zip(sl, ml):
        assert torch.equal(a, b)
    with pytest.raises(NotImplementedError, match="nms_rotated_multi_label"):
        uops.nms_device(pred, 0.25, 0.45, nc=case["nc"], multi_label=True, rotated=True)


# ------------------------------------------------------------------------------------------------------------------ ey_probiou_batch
def test_probiou_batch(ops_g):
    from edge_yolo_amd.nn import _ops
    pred, gt, poff, goff = S.pair_case()
    assert [(poff[b + 1] - poff[b], goff[b + 1] - goff[b]) for b in range(4)] == S.PAIR_SIZES
    dp, dg = torch.tensor(pred).cuda(), torch.tensor(gt).cuda()
    out, off = _ops.probiou_batch(dp, poff, dg, goff)
    sizes = [n * m for n, m in S.PAIR_SIZES]
    assert out.numel() == sum(sizes) and list(off) == [0, 0, 0, 1]
    host = out.cpu().numpy()
    for b, (n, m) in enumerate(S.PAIR_SIZES):
        if not n * m:
            continue
        got = host[off[b]: off[b] + n * m].reshape(m, n)
        p, g = pred[poff[b]:poff[b + 1]], gt[goff[b]:goff[b + 1]]
        np.testing.assert_array_equal(got, _ops.probiou(torch.tensor(g).cuda(), torch.tensor(p).cuda()).cpu().numpy())  # bit for bit the single-problem call
        ref32, ref64 = ops_g[f"pb_{b}"].astype(np.float64), f64.probiou64(g, p)
        E = float(np.abs(ref32 - ref64).max())
        err = np.abs(got.astype(np.float64) - ref64)
        print(f"probiou_batch image {b} ({m}x{n}): E {E:.3e} achieved {float(err.max()):.3e}")
        assert (err <= f64.bound(E, ref64)).all()
    # explicit offsets in another order, into a caller's buffer that is larger than needed: nothing else is written
    buf = torch.full((sum(sizes) + 7,), -1.0, device="cuda")
    out2, off2 = _ops.probiou_batch(dp, poff, dg, goff, out_off=[5, 5, sizes[3] + 3, 2], out=buf)
    h2 = out2.cpu().numpy()
    np.testing.assert_array_equal(h2[2:2 + sizes[3]], host[1:])
    assert h2[sizes[3] + 3] == host[0] and (h2[:2] == -1).all() and h2[sizes[3] + 2] == -1 and (h2[sizes[3] + 4:] == -1).all()
    empty, _ = _ops.probiou_batch(dp[:0], [0, 0], dg[:3], [0, 3])
    assert empty.numel() == 0
    with pytest.raises(NotImplementedError):
        _ops.probiou_batch(dp, [0] * 130, dg, [0] * 130)


# ------------------------------------------------------------------------------------------------------------------ the validator
def _batch(g):
    B, H, W = (int(v) for v in g["image_shape"])
    return {"img": synth.synth_images(B, H, W, seed=int(g["image_seed"])), "cls": torch.tensor(g["cls"]), "bboxes": torch.tensor(g["bboxes"]),
            "batch_idx": torch.tensor(g["batch_idx"]), "ori_shape": [tuple(int(v) for v in s) for s in g["ori_shape"]],
            "ratio_pad": [((float(gn), float(gn)), (float(p[0]), float(p[1]))) for gn, p in zip(g["ratio_gain"], g["ratio_padwh"])]}


def test_val_end_to_end_against_the_reference(case_g):
    """yolo11n-obb at 64x96, fp32, the reference's weights and batch.  The forward agrees with the reference's to a few 1e-5 (the rows are
    held to the fp32 layer bar); the golden's margins, asserted here from the values the generator stored -- every NMS column > 1e-3 from
    the threshold, every class score > 1e-4 from conf, kept scores > 1e-4 apart within an image and, for one class, across the batch,
    every ProbIoU > 1e-4 from the ten thresholds -- make the kept rows, their order per class and the true-positive matrix the
    reference's, so the AP values must be the reference's.  Precision and recall are read off curves over the confidences; the generator
    asserted that the reference's own values do not move (1e-9) when every confidence moves by up to 5e-5, so they are held to 1e-6."""
    import edge_yolo_amd
    from edge_yolo_amd.engine.validator import OBBValidator
    g = case_g
    assert float(g["nms_margin"]) > S.MARGIN and float(g["margin"]) > S.IOU_MARGIN
    assert min(float(g["gap_conf"]), float(g["gap_kept"]), float(g["gap_class"])) > float(g["score_gap"]) == 1e-4 and float(g["metric_shift"]) < 1e-9
    model = edge_yolo_amd.YOLO("yolo11n-obb.yaml")
    model.model.load_state_dict(obb_synth.state_dict(model.model.state_dict()))
    batch = _batch(g)
    conf, iou = float(g["conf"]), float(g["iou"])
    res = model.val([batch], validator=OBBValidator, conf=conf, iou=iou, device="cuda:0")
    v = model.validator
    assert isinstance(v, OBBValidator) and list(res) == list(g["full_keys"]) and v.seen == int(g["full_seen"])
    # the kept rows of the same forward against the reference's
    pre = v.preprocess(batch)
    with torch.cuda.device(v.device):
        rows = v.postprocess(v.model(pre["img"]))
    for i, r in enumerate(rows):
        want = g[f"pred{i}"]
        got = r.cpu().numpy()
        print(f"image {i}: kept {len(got)}, reference {len(want)}, max abs err {float(np.abs(got - want).max()) if len(want) == len(got) and len(got) else 0:.3e}")
        assert got.shape == want.shape
        np.testing.assert_array_equal(got[:, 5], want[:, 5])
        np.testing.assert_allclose(got, want, **LAYER_TOL)
    tp = np.concatenate(v.stats["tp"], 0)
    np.testing.assert_array_equal(tp, g["full_tp"])
    np.testing.assert_allclose(np.concatenate(v.stats["conf"], 0), g["full_conf"], **LAYER_TOL)
    np.testing.assert_array_equal(v.nt_per_class, g["full_nt_per_class"])
    ref = dict(zip(g["full_keys"], g["full_values"]))
    means = g["full_means"]  # the reference's precision, recall, mAP50, mAP75, mAP50-95
    print("device", res, "reference", ref, "means", means)
    assert abs(res["metrics/mAP50(B)"] - ref["metrics/mAP50(B)"]) < 1e-9 and abs(res["metrics/mAP50-95(B)"] - means[4]) < 1e-9
    assert abs(res["fitness"] - ref["fitness"]) < 1e-9
    for k in ("metrics/precision(B)", "metrics/recall(B)"):
        assert abs(res[k] - ref[k]) < 1e-6, (k, res[k], ref[k])
    np.testing.assert_allclose(v.box.all_ap, g["full_ap"], rtol=0, atol=1e-9)
    # the host route on this run's own rows: the same statistics and metrics
    h = OBBValidator(model.model, conf=conf, iou=iou, device="cpu")
    h.update_metrics([r.cpu().numpy() for r in rows], batch)
    hres = h.get_stats()
    np.testing.assert_array_equal(np.concatenate(h.stats["tp"], 0), tp)
    for k in res:
        assert abs(res[k] - hres[k]) < 1e-12, k
    # the refusals that stay, and the options that are accepted by name only
    with pytest.raises(NotImplementedError, match="OBBValidator"):
        model.val([batch])
    with pytest.raises(NotImplementedError, match="save_json"):
        model.val([batch], validator=OBBValidator, save_json=True)
