"""CPU: the edge cases of tests/nms_edge_cases.py are what they claim to be -- the oracle's own answer (oracle/nms.py, topk_ref) satisfies
every condition the case states, so the -m gpu comparisons in test_gpu_nms_edges.py / test_gpu_e2e_topk_exact.py cannot become vacuous."""
import numpy as np
import pytest
import torch

import nms_edge_cases as ec
from oracle import model as om


@pytest.mark.parametrize("name", sorted(ec.NMS_CASES))
def test_nms_case_conditions(name):
    case, results = ec.nms_reference(name)
    assert len(results) == len(case.variants) > 0
    for v, (rows, idx) in zip(case.variants, results):
        kw = ec.full_kw(case, v)
        for r, i in zip(rows, idx):
            assert r.dtype == np.float32 and r.shape == (i.shape[0], 6) and r.shape[0] <= kw["max_det"]
    case.check(results)


def test_fast_path_eligibility_of_the_cases():
    """The cases meant for the fast path (and for its max_nms / max_det gates) are on the intended side of nms_select_launch's condition."""
    elig = {}
    for name in ec.NMS_CASES:
        case, _ = ec.nms_reference(name)
        elig[name] = [ec.fast_eligible(ec.full_kw(case, v), case.pred.shape[1] - 4) for v in case.variants]
    assert elig["max_nms_det1024"] == [m >= ec.NF_KMAX for m in ec.MAX_NMS_LIST] and not any(elig["max_nms_det1500"])
    assert elig["max_det"] == [m <= 1024 for m in ec.MAX_DET_LIST]
    assert not any(elig["max_nms_multi_label"]) and not any(elig["multi_label_filter"])
    for name in ("scalar_score_315", "scalar_score_1001", "scalar_score_8399", "degenerate_nc3", "degenerate_nc16", "iou_thres", "conf_thres", "mixed_batch", "nc252"):
        assert all(elig[name]), name


@pytest.mark.parametrize("name", sorted(ec.TOPK_CASES))
def test_topk_case_conditions(name):
    case, ref = ec.topk_reference(name)
    B, no, A = case.pred.shape
    for k in case.ks:
        rows, index = ref[k]
        assert rows.shape == (B, k, 6) and rows.dtype == np.float32 and index.shape == (B, k) and 1 <= k <= A
        assert (np.diff(rows[..., 4], axis=1) <= 0).all()
        np.testing.assert_array_equal(case.pred[np.arange(B)[:, None], :4, index], rows[..., :4])
        case.check(k, rows, index)


@pytest.mark.parametrize("name", ec.TIE_FREE)
def test_topk_ref_equals_e2e_postprocess_on_tie_free_input(name):
    """Without ties the two-pass torch.topk selection of Detect.postprocess has one answer, and topk_ref gives it bit for bit."""
    case, ref = ec.topk_reference(name)
    nc = case.pred.shape[1] - 4
    for k in case.ks:
        want = om.e2e_postprocess(torch.tensor(case.pred).permute(0, 2, 1), k, nc).numpy()
        np.testing.assert_array_equal(ref[k][0], want)
