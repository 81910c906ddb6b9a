"""-m gpu: ey_e2e_topk (the result path of every end2end head: nms_general_body in NMS_MODE_TOPK | NMS_MODE_XYXY, conf = -1, chunk cap
4096) vs topk_ref, the documented order -- score descending, equal scores by ascending (anchor, class) -- written down plainly
(tests/nms_edge_cases.py; the cases' conditions are asserted on the CPU in test_nms_edges_cpu.py).  Rows and anchor indices BIT-exact."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import nms_edge_cases as ec  # noqa: E402
from oracle import model as om  # noqa: E402

K_LDS = 1611  # the largest k the select workgroup's LDS holds (include/edgeyolo_hip.h); 1612 is refused


@pytest.fixture(scope="module")
def ops():
    import edge_yolo_amd  # noqa: F401
    from edge_yolo_amd.nn import _ops
    return _ops


def _check(ops, x, k, want_rows, want_index, what):
    rows, index = ops.e2e_topk(x, k, want_index=True)
    rows_only = ops.e2e_topk(x, k)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(index.cpu().numpy(), want_index, err_msg=f"{what}: anchor indices")
    np.testing.assert_array_equal(rows.cpu().numpy(), want_rows, err_msg=f"{what}: rows")
    np.testing.assert_array_equal(rows_only.cpu().numpy(), want_rows, err_msg=f"{what}: rows without the index output")


@pytest.mark.parametrize("name", sorted(ec.TOPK_CASES))
def test_topk_equals_reference(ops, name):
    """tie_free / nc1_*: distinct scores, k up to A, nc = 1 on the scalar (A = 333) and the vector (A = 1024) score kernel;
    heavy_*: > 4096 pairs in one top digit with k beyond the bins above it, so the descent opens the bin (one score: down to the index
    digits, the tie group in (anchor, class) order); all_equal: 9216 equal scores; zero_tail: scores of exactly 0.0 (key high word 0);
    mixed_batch: three of these regimes in one launch."""
    case, ref = ec.topk_reference(name)
    x = torch.tensor(case.pred).cuda()
    nc = case.pred.shape[1] - 4
    for k in case.ks:
        want_rows, want_index = ref[k]
        _check(ops, x, k, want_rows, want_index, f"{name} k={k}")
        if name in ec.TIE_FREE:  # ... and Detect.postprocess's two torch.topk passes, whose answer is unique here
            np.testing.assert_array_equal(want_rows, om.e2e_postprocess(torch.tensor(case.pred).permute(0, 2, 1), k, nc).numpy())


def test_topk_argument_errors_and_lds_bound(ops):
    """k outside 1..A: ValueError before anything is launched.  k beyond what the select workgroup's LDS holds: the library's error,
    naming LDS (a host-side check in front of the select launch), at 4096 and at the first refused value; the largest accepted k and the
    next ordinary call return the right rows."""
    from edge_yolo_amd import _lib
    rng = np.random.default_rng(3)
    A, nc = 4096, 2
    pred = np.zeros((1, 4 + nc, A), np.float32)
    pred[0, :4] = rng.uniform(0, 600, (4, A))
    pred[0, 4:] = rng.permutation(np.linspace(0.001, 0.999, nc * A, dtype=np.float32)).reshape(nc, A)
    x = torch.tensor(pred).cuda()
    small = x[:, :, :333].contiguous()
    for k in (0, 334):
        with pytest.raises(ValueError):
            ops.e2e_topk(small, k)
    for k in (4096, K_LDS + 1):
        with pytest.raises(_lib.HipLibraryError, match="LDS"):
            ops.e2e_topk(x, k)
    for k in (K_LDS, 300):
        _check(ops, x, k, *ec.topk_ref(pred, k), f"k={k} after the refusal")
