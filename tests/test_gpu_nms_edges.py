"""-m gpu: ey_nms at the edges tests/test_gpu_nms.py does not reach (cases and their conditions: tests/nms_edge_cases.py; the conditions
themselves are asserted on the CPU in test_nms_edges_cpu.py) vs oracle.nms.non_max_suppression.  Rows, counts and anchor indices are
BIT-exact, rows beyond the count are zero; where the predict-mode fast path is eligible every case runs with it switched off and on
(nms_fast_k 0 / 2048) and with the bit matrix covering 512 / 1536 candidates, and every setting gives the same answer."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import gpu_util  # noqa: E402
import nms_edge_cases as ec  # noqa: E402

SETTINGS = [(0, 512), (0, 1536), (2048, 512), (2048, 1536)]  # (nms_fast_k, nms_mask_k)
MAX_DET_LDS = 1611  # the largest max_det / k the select workgroup's LDS holds (include/edgeyolo_hip.h); 1612 is refused


@pytest.fixture(scope="module")
def E():
    import edge_yolo_amd  # noqa: F401
    from edge_yolo_amd import _lib
    from edge_yolo_amd.nn import _ops
    from edge_yolo_amd.utils import ops

    class NS:
        pass
    ns = NS()
    ns._ops, ns.ops, ns.lib = _ops, ops, _lib
    return ns


def _mask(classes, nc):
    if classes is None:
        return None
    m = torch.zeros(nc, dtype=torch.uint8)
    m[list(classes)] = 1
    return m.cuda()


def _run(E, x, kw, nc):
    boxes, count, index, ws = E._ops.nms(x, kw["conf_thres"], kw["iou_thres"], kw["max_det"], kw["max_nms"], float(kw["max_wh"]), kw["agnostic"],
                                         _mask(kw["classes"], nc), kw["multi_label"], return_workspace=True)
    torch.cuda.synchronize()
    return boxes.cpu().numpy(), count.cpu().numpy(), index.cpu().numpy(), ws.cpu().numpy()


def _assert_equals_oracle(got, want, widx, what):
    boxes, count, index = got[:3]
    for b in range(len(want)):
        n = int(count[b])
        assert n == want[b].shape[0], f"{what}: image {b}: kept {n}, oracle {want[b].shape[0]}"
        np.testing.assert_array_equal(index[b, :n], widx[b], err_msg=f"{what}: image {b}: anchor indices")
        np.testing.assert_array_equal(boxes[b, :n], want[b], err_msg=f"{what}: image {b}: rows")
        np.testing.assert_array_equal(boxes[b, n:], 0.0, err_msg=f"{what}: image {b}: rows beyond the count")
        np.testing.assert_array_equal(index[b, n:], -1, err_msg=f"{what}: image {b}: indices beyond the count")


def _check_case(E, name, meta_check=None):
    case, results = ec.nms_reference(name)
    nc = case.pred.shape[1] - 4
    x = torch.tensor(case.pred).cuda()
    for v, (want, widx) in zip(case.variants, results):
        kw = ec.full_kw(case, v)
        settings = SETTINGS if ec.fast_eligible(kw, nc) else [None]
        first = None
        for st in settings:
            what = f"{name} {v} (nms_fast_k, nms_mask_k)={st}"
            if st is None:
                got = _run(E, x, kw, nc)
            else:
                with gpu_util.tuned(nms_fast_k=st[0], nms_mask_k=st[1]):
                    got = _run(E, x, kw, nc)
            _assert_equals_oracle(got, want, widx, what)
            if first is None:
                first = got
            else:
                for a, r in zip(got[:3], first[:3]):
                    np.testing.assert_array_equal(a, r, err_msg=f"{what} differs from the first setting")
            if meta_check is not None and st is not None and st[0] == 2048:
                meta_check(ec.fast_meta(got[3], case.pred.shape[0], case.pred.shape[2]), got)


@pytest.mark.parametrize("name", ["max_nms_det1024", "max_nms_det1500"])
def test_max_nms_single_label(E, name):
    """max_nms in {1 .. 3000} on 4096 candidates: the general kernel's cut `processed + n > max_nms` (below 2048, and at max_det 1500),
    the fast path's gate `max_nms >= NF_KMAX` and its `nsel >= max_nms` completion test (2048, 2049, 3000 at max_det 1024)."""
    _check_case(E, name)


def test_max_nms_multi_label(E):
    _check_case(E, "max_nms_multi_label")


def test_multi_label_class_filter_agnostic_max_wh(E):
    _check_case(E, "multi_label_filter")


@pytest.mark.parametrize("A", [315, 1001, 8399])
def test_scalar_score_kernel(E, A):
    """A % 4 != 0: nms_score_kernel instead of nms_score4_kernel, B = 2, with and without a class filter."""
    _check_case(E, f"scalar_score_{A}")


@pytest.mark.parametrize("nc", [3, 16])
def test_degenerate_geometry(E, nc):
    """Zero / negative extents, areas that overflow, NaN and inf coordinates, duplicates with a denormal area: iou_gt's NaN branch, the
    mask kernel's `sane` ballot, the partitioned greedy's fallback (nc = 16: balanced owner waves and the non-finite boxes scored last, so
    the general kernel's first chunks are eligible for the class-partitioned greedy and its last chunk has to leave it)."""
    _check_case(E, f"degenerate_nc{nc}")


def test_iou_thres_0_tiny_1(E):
    _check_case(E, "iou_thres")


def test_conf_thres_0_and_1(E):
    _check_case(E, "conf_thres")


def test_mixed_batch_one_launch(E):
    """Nothing passes | more than max_det survive | five candidates | a tie group the fast path cannot split, in one launch: the `done`
    words of the workspace show that the fast path finished image 2 and left image 3 to the general kernel."""
    def meta_check(meta, got):
        assert [m[1] for m in meta] == [0, 4096, 5, 4096], meta
        assert meta[1][2] == 1 and meta[2] == (5, 5, 1), meta
        assert meta[3] == (100, 4096, 0), meta  # only the keys above the tie group could be selected
    _check_case(E, "mixed_batch", meta_check)


def test_max_det_switches(E):
    """max_det 1 | 512 / 513 (chunk cap 1024 -> 4096, class partition off) | 1024 / 1025 (fast path off) | 1500, every run cut by max_det."""
    _check_case(E, "max_det")


def test_nc252(E):
    _check_case(E, "nc252")


def test_max_det_beyond_the_lds_is_refused(E):
    """max_det whose kept-box lists do not fit the select workgroup's LDS: the library's error (naming LDS) from the host-side check in
    front of the select launch, at 4096 and at the first refused value; the largest accepted value and the next ordinary call are right."""
    from oracle import nms as onms
    case, results = ec.nms_reference("max_det")
    x = torch.tensor(case.pred).cuda()
    kw = ec.full_kw(case, dict())
    for bad in (4096, MAX_DET_LDS + 1):
        with pytest.raises(E.lib.HipLibraryError, match="LDS"):
            _run(E, x, {**kw, "max_det": bad}, 4)
    want, widx = onms.non_max_suppression(case.pred, **{**kw, "max_det": MAX_DET_LDS}, return_idx=True)
    _assert_equals_oracle(_run(E, x, {**kw, "max_det": MAX_DET_LDS}, 4), want, widx, f"max_det={MAX_DET_LDS}")
    _assert_equals_oracle(_run(E, x, {**kw, "max_det": 512}, 4), *results[ec.MAX_DET_LIST.index(512)], "max_det=512 after the refusal")


def test_nms_device_surface(E):
    """The same answers through utils.ops.nms_device (class list -> mask, keyword defaults)."""
    case, results = ec.nms_reference("scalar_score_1001")
    x = torch.tensor(case.pred).cuda()
    for v, (want, widx) in zip(case.variants, results):
        kw = ec.full_kw(case, v)
        boxes, count, index = E.ops.nms_device(x, kw["conf_thres"], kw["iou_thres"], classes=kw["classes"], max_det=kw["max_det"])
        _assert_equals_oracle((boxes.cpu().numpy(), count.cpu().numpy(), index.cpu().numpy()), want, widx, f"nms_device {v}")
