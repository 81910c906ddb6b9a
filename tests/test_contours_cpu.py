"""Mask polygons without a GPU: the restatement of cv2.findContours (tests/contours_ref.py) against hand-written expectations and against
properties that do not depend on it, on every synthetic mask (tests/contours_synth.py); merge_multi_segment, masks2segments' strategies
and the coordinates of Masks.xy / xyn against the reference's own output (tests/golden/contours_ops.npz); a Masks on the host raises; and
the host build of the kernel's own text (csrc/contours_core.inc.h through tests/contours_host_main.cpp, one lane, compiled with
AddressSanitizer and UBSan and run as a plain program) equals the restatement on every mask, with and without windows, and reports an
overflow instead of writing past a buffer that is too small."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import contours_ref as ref
import contours_synth as cs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = [c[0] for c in cs.cases()]


def _index(name):
    return NAMES.index(name)


def _pts(c):
    return [tuple(int(v) for v in p) for p in c]


def test_hand_written_expectations():
    (c,) = cs.expected(_index("rectangle"))  # OpenCV's well-known order: from the top-left corner down, counter-clockwise on the screen
    assert c.dtype == np.int32 and _pts(c) == [(3, 2), (3, 5), (7, 5), (7, 2)]
    assert cs.expected(_index("empty_5x9")) == [] and cs.expected(_index("empty_1x1")) == []
    for name, p in (("pixel_tl", (0, 0)), ("pixel_tr", (8, 0)), ("pixel_bl", (0, 4)), ("pixel_br", (8, 4)), ("pixel_interior", (4, 2)), ("ones_1x1", (0, 0))):
        (c,) = cs.expected(_index(name))
        assert _pts(c) == [p], name
    assert _pts(cs.expected(_index("ones_1x7"))[0]) == [(0, 0), (6, 0)] and _pts(cs.expected(_index("ones_7x1"))[0]) == [(0, 0), (0, 6)]
    assert _pts(cs.expected(_index("ones_5x9"))[0]) == [(0, 0), (0, 4), (8, 4), (8, 0)]
    assert _pts(cs.expected(_index("line_h"))[0]) == [(1, 2), (7, 2)] and _pts(cs.expected(_index("line_v"))[0]) == [(2, 1), (2, 7)]
    assert _pts(cs.expected(_index("line_diag"))[0]) == [(0, 0), (6, 6)] and _pts(cs.expected(_index("line_antidiag"))[0]) == [(6, 0), (0, 6)]
    counts = {"squares_touching": 1, "ring": 1, "ring_island": 1, "ring_thick_island": 1, "nested_twice": 1, "c_right_blob": 2, "c_left_blob": 2, "spur": 1,
              "spur_up": 1, "checkerboard_9x9": 1}
    for name, n in counts.items():
        assert len(cs.expected(_index(name))) == n, name
    # last found first: the blob in the bay starts below the C's first pixel
    for name in ("c_right_blob", "c_left_blob"):
        blob, c = cs.expected(_index(name))
        assert _pts(blob) == [(4 if name == "c_right_blob" else 2, 3), (4 if name == "c_right_blob" else 2, 4), (5 if name == "c_right_blob" else 3, 4),
                              (5 if name == "c_right_blob" else 3, 3)] and _pts(c)[0] == (1, 1)
    # the spur's pixels are passed twice: its tip is a vertex, and the pixel where it leaves the body appears on the way out and back
    spur = _pts(cs.expected(_index("spur"))[0])
    assert (6, 3) in spur and len(spur) == 9
    # the checkerboard is one 8-connected component whose border zigzags: the walk turns at every one of its 32 steps
    assert len(cs.expected(_index("checkerboard_9x9"))[0]) == 32


def test_label_of_an_unexamined_east_neighbour():
    m, (y, x) = cs.EAST_UNEXAMINED
    contours, lab = ref.find_contours(m, return_labels=True)
    assert m[y, x] == 1 and m[y, x + 1] == 0 and lab[y, x] == 2, lab
    assert lab[y, x + 3] == -2 and len(contours) == 1  # the right wall: east examined and 0


@pytest.mark.parametrize("i", range(len(NAMES)), ids=NAMES)
def test_restatement_properties(i):
    m = cs.cases()[i][1]
    before = m.copy()
    ref.check_properties(m, cs.expected(i))
    assert np.array_equal(m, before)


def test_more_random_masks_have_the_properties():
    rng = np.random.default_rng(7)
    for k in range(60):
        h, w = int(rng.integers(1, 20)), int(rng.integers(1, 24))
        m = (rng.random((h, w)) < rng.uniform(0.3, 0.9)).astype(np.uint8)
        ref.check_properties(m, ref.find_contours(m))


# ---------------------------------------------------------------------------------------------------------------------------------------
# post-processing against the reference's own output

@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "contours_ops.npz"))


def test_merge_multi_segment_equals_reference(golden):
    from edge_yolo_amd.data.converter import merge_multi_segment, min_index
    j = 0
    while f"merge{j}_n" in golden:
        segs = [golden[f"merge{j}_in{k}"] for k in range(int(golden[f"merge{j}_n"]))]
        got = np.concatenate(merge_multi_segment([s.copy() for s in segs]))
        assert got.dtype == golden[f"merge{j}_out"].dtype and np.array_equal(got, golden[f"merge{j}_out"])
        j += 1
    assert j >= 5
    a, b = np.array([[0, 0], [5, 5], [9, 9]]), np.array([[20, 20], [6, 5], [5, 6]])
    assert tuple(int(v) for v in min_index(a, b)) == (1, 1)  # the first of two equally near pairs


@pytest.mark.parametrize("strategy", ["all", "largest"])
def test_masks2segments_strategies_equal_reference(golden, strategy):
    from edge_yolo_amd.utils.ops import _contours2segment
    several = 0
    for i in range(len(NAMES)):
        got = _contours2segment(cs.expected(i), strategy)
        want = golden[f"seg_{strategy}_{i}"]
        assert got.dtype == np.float32 and got.shape == want.shape and np.array_equal(got, want), NAMES[i]
        several += len(cs.expected(i)) > 1
    assert several >= 8
    assert _contours2segment([], strategy).shape == (0, 2) and _contours2segment([], strategy).dtype == np.float32
    with pytest.raises(ValueError, match="strategy"):
        _contours2segment(cs.expected(0), "convex")


def test_largest_takes_the_first_of_equal_length():
    from edge_yolo_amd.utils.ops import _contours2segment
    a, b = np.array([[1, 1], [2, 2]], np.int32), np.array([[7, 7], [8, 8]], np.int32)
    assert np.array_equal(_contours2segment([a, b], "largest"), a.astype(np.float32))


def test_masks_coordinates_equal_reference(golden):
    """what Masks.xy / xyn do with the segments (scale_coords per segment), on the restatement's contours."""
    from edge_yolo_amd.utils import ops
    j = 0
    while f"masks{j}_idx" in golden:
        idx, orig = golden[f"masks{j}_idx"], tuple(int(v) for v in golden[f"masks{j}_orig"])
        shape = cs.cases()[int(idx[0])][1].shape
        for key, normalize in (("xy", False), ("xyn", True)):
            got = [ops.scale_coords(shape, ops._contours2segment(cs.expected(int(i))), orig, normalize=normalize) for i in idx]
            assert [len(g) for g in got] == golden[f"masks{j}_len"].tolist()
            cat = np.concatenate(got)
            assert cat.dtype == np.float32 and np.array_equal(cat, golden[f"masks{j}_{key}"]), (j, key)
        j += 1
    assert j >= 5


def test_masks_on_the_host_raise():
    from edge_yolo_amd.engine.results import Masks
    from edge_yolo_amd.utils import ops
    m = Masks(torch.zeros(2, 8, 8, dtype=torch.uint8), (8, 8))
    for holder in (m, m.cpu(), m.numpy()):
        for name in ("xy", "xyn"):
            with pytest.raises(NotImplementedError, match="device"):
                getattr(holder, name)
    with pytest.raises(NotImplementedError, match="device"):
        ops.masks2segments(torch.zeros(1, 4, 4))


def test_names_are_exported():
    import edge_yolo_amd.data.converter as conv
    from edge_yolo_amd import _lib
    from edge_yolo_amd.nn import _ops
    from edge_yolo_amd.utils import ops
    assert set(conv.__all__) == {"min_index", "merge_multi_segment"}
    assert callable(ops.masks2segments) and callable(_ops.mask_contours)
    assert "ey_mask_contours" in _lib.SIGNATURES and "ey_mask_contours_workspace_bytes" in _lib.SIGNATURES


# ---------------------------------------------------------------------------------------------------------------------------------------
# the kernel's own text, built for the host with one lane

@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a C++ compiler is needed for the host build of the contour core"
    exe = str(tmp_path_factory.mktemp("contours_host") / "contours_host_main")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "contours_host_main.cpp"), "-o", exe], check=True)
    return exe


def _run(exe, tmp_path, masks, ccap, vcap, windows=None):
    """-> [(info, lens, verts)] per mask; asserts that the masks come back untouched."""
    n, h, w = masks.shape
    src, dst = str(tmp_path / "case.bin"), str(tmp_path / "result.bin")
    with open(src, "wb") as f:
        f.write(np.asarray([n, h, w, ccap, vcap, int(windows is not None), 0, 0], np.int32).tobytes())
        f.write(np.ascontiguousarray(masks, np.uint8).tobytes())
        if windows is not None:
            f.write(np.ascontiguousarray(windows, np.int32).tobytes())
    subprocess.run([exe, src, dst], check=True)
    raw = np.fromfile(dst, np.uint8)
    per = 4 * (4 + ccap + 2 * vcap)
    assert raw.size == n * per + n * h * w
    assert np.array_equal(raw[n * per:].reshape(n, h, w), masks)
    out = []
    for b in range(n):
        a = raw[b * per:(b + 1) * per].view(np.int32)
        out.append((a[:4], a[4:4 + ccap], a[4 + ccap:].reshape(vcap, 2)))
    return out


def _tight_windows(idx):
    win = []
    for i in idx:
        ys, xs = np.nonzero(cs.cases()[i][1])
        win.append([xs.min(), ys.min(), xs.max() + 1, ys.max() + 1] if len(ys) else [3, 2, 1, 1])  # (an empty window for an empty mask)
    return np.asarray(win, np.int32)


@pytest.mark.parametrize("windows", [False, True], ids=["whole", "windows"])
def test_host_build_equals_restatement(host_exe, tmp_path, windows):
    for shape, idx in cs.by_shape().items():
        masks = np.stack([cs.cases()[i][1] for i in idx])
        res = _run(host_exe, tmp_path, masks, 128, 1024, _tight_windows(idx) if windows else None)
        for i, (info, lens, verts) in zip(idx, res):
            assert info[2] == 0 and info[3] == 0, NAMES[i]
            assert cs.same(cs.decode(info, lens, verts), cs.expected(i)), NAMES[i]
            assert (lens[info[0]:] == -7).all() and (verts[info[1]:] == -7).all()  # nothing beyond what the counts say


def test_host_build_window_that_cuts_a_mask(host_exe, tmp_path):
    """what lies outside the window counts as 0: the same contours as those of the mask with everything outside erased."""
    i = _index("blobs_64x96_1")
    m = cs.cases()[i][1]
    win = np.asarray([[10, 7, 61, 40], [-5, -5, 200, 200], [30, 30, 31, 31]], np.int32)
    res = _run(host_exe, tmp_path, np.stack([m] * 3), 128, 1024, win)
    for (x0, y0, x1, y1), (info, lens, verts) in zip(win, res):
        cut = np.zeros_like(m)
        cut[max(y0, 0):y1, max(x0, 0):x1] = m[max(y0, 0):y1, max(x0, 0):x1]
        assert info[2] == 0 and cs.same(cs.decode(info, lens, verts), ref.find_contours(cut))


@pytest.mark.parametrize("ccap,vcap", [(128, 4), (1, 1024), (1, 1)])
def test_host_build_small_buffers(host_exe, tmp_path, ccap, vcap):
    """a buffer that is too small: the counts are still complete, the overflow flag is set exactly when something did not fit, and nothing is
    written out of bounds (each buffer is an allocation of its own size under AddressSanitizer)."""
    flagged = 0
    for shape, idx in cs.by_shape().items():
        masks = np.stack([cs.cases()[i][1] for i in idx])
        for i, (info, lens, verts) in zip(idx, _run(host_exe, tmp_path, masks, ccap, vcap)):
            want = cs.expected(i)
            nc, nv = len(want), sum(len(c) for c in want)
            assert (int(info[0]), int(info[1])) == (nc, nv), NAMES[i]
            over = nc > ccap or nv > vcap
            assert int(info[2]) == int(over), NAMES[i]
            flagged += over
            if not over:
                assert cs.same(cs.decode(info, lens, verts), want), NAMES[i]
            else:  # what was written is the beginning of the whole result
                flat = np.concatenate(want[::-1]) if want else np.zeros((0, 2), np.int32)
                assert np.array_equal(verts[:min(nv, vcap)], flat[:vcap])
                assert lens[:min(nc, ccap)].tolist() == [len(c) for c in want[::-1]][:ccap]
    assert flagged >= 8
