"""Object tracking without a GPU: the case set takes every path of the frame step and keeps every decision 1e-4 away from flipping; the host
build of the kernels' own text (csrc/track_core.inc.h through tests/track_host_main.cpp, one lane, compiled with AddressSanitizer and UBSan
and run as a plain program) equals the float64 restatement on every case under the bars of the GPU test (tests/test_gpu_track.py), and
its solver equals scipy on the assignment cases; Boxes with 7 columns, the tracker settings and the refusals of track()."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import fp64_track_ref as ref
import track_synth as ts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_path_is_taken():
    total = {k: 0 for k in ref.PATHS}
    for i in range(len(ts.cases())):
        for k, v in ts.ref_run(i)[0].counters.items():
            total[k] += v
    print(total)
    assert all(v > 0 for v in total.values()), [k for k, v in total.items() if not v]


@pytest.mark.parametrize("i", range(len(ts.cases())), ids=[c["name"] for c in ts.cases()])
def test_decision_margins(i):
    m = ts.margins(ts.ref_run(i)[0])
    print(ts.cases()[i]["name"], m)
    assert all(v >= 1e-4 for v in m.values()), m


def test_occlusion_story():
    """B's lost track lands on A at frame 10 and is removed as its duplicate; B comes back as a third id at 18 and is output from 19."""
    _, frames = ts.ref_run(3)
    ids = [sorted(int(v) for v in rows[:, 4]) for rows, _ in frames]
    assert ids[8] == [1, 2] and ids[9] == [1] and ids[17] == [1] and ids[18] == [1, 3]
    assert ts.ref_run(3)[0].counters["dup_drop_lost"] == 1 and ts.ref_run(4)[0].counters["dup_drop_tracked"] == 1


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a C++ compiler is needed for the host build of the tracker core"
    exe = str(tmp_path_factory.mktemp("track_host") / "track_host_main")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "track_host_main.cpp"), "-o", exe], check=True)
    return exe


def _run(exe, tmp_path, head, thr, payload):
    src, dst = str(tmp_path / "case.bin"), str(tmp_path / "result.bin")
    with open(src, "wb") as f:
        f.write(np.asarray(head + [0] * (8 - len(head)), np.int32).tobytes())
        f.write(np.asarray(thr + [0.0] * (4 - len(thr)), np.float32).tobytes())
        for a in payload:
            f.write(a.tobytes())
    subprocess.run([exe, src, dst], check=True)
    with open(dst, "rb") as f:
        return f.read()


@pytest.fixture(scope="module")
def level():
    return ts.rounding_level()


@pytest.mark.parametrize("i", range(len(ts.cases())), ids=[c["name"] for c in ts.cases()])
def test_host_build_equals_restatement(i, host_exe, tmp_path, level):
    case = ts.cases()[i]
    a = {**ref.DEFAULTS, **case["args"]}
    T, cap = case["max_tracks"], max(len(r) for r in case["frames"]) + 3
    payload = []
    for rows in case["frames"]:
        buf = np.full((cap, 6), np.nan, np.float32)  # (rows past the count are never read as detections)
        buf[:len(rows)] = rows
        payload += [np.int32(len(rows)), buf]
    raw = _run(host_exe, tmp_path, [1, cap, T, len(case["frames"]), int(a["track_buffer"]), int(a["fuse_score"])],
               [a["track_high_thresh"], a["track_low_thresh"], a["new_track_thresh"], a["match_thresh"]], payload)
    off, worst = 0, 0.0

    def take(dt, *shape):
        nonlocal off
        arr = np.frombuffer(raw, dt, int(np.prod(shape)), off).reshape(shape)
        off += arr.nbytes
        return arr

    for f, (want, snap) in enumerate(ts.ref_run(i)[1]):
        cnt, rows, ids, hdr = int(take(np.int32, 1)[0]), take(np.float32, cap, 8), take(np.int32, cap), take(np.int32, 4)
        si, sf, kf = take(np.int32, T, 8), take(np.float32, T, 2), take(np.float64, T, 72)
        worst = max(worst, ts.compare_frame(f"{case['name']} frame {f}", want, snap, cnt, rows, ids, hdr, si, sf, kf, 32 * level))
    assert off == len(raw)
    print(f"{case['name']}: host build vs restatement {worst:.3e}, float64 vs longdouble d = {level:.3e}, bar 32 d = {32 * level:.3e}")


def _host_assign(exe, tmp_path, cost, thresh):
    n, m = cost.shape
    ld = m + 2
    buf = np.full((n, ld), np.nan, np.float32)
    buf[:, :m] = cost
    raw = _run(exe, tmp_path, [2, n, m, ld], [thresh], [buf])
    out = np.frombuffer(raw, np.int32)
    assert out.size == n + m
    return out[:n], out[n:]


def test_host_solver_equals_scipy(host_exe, tmp_path):
    for name, cost, thresh in ts.assignment_cases():
        ts.check_matching(name, cost, thresh, *_host_assign(host_exe, tmp_path, cost, thresh), exact=True)
    for name, cost, thresh in ts.tie_cases():
        ts.check_matching(name, cost, thresh, *_host_assign(host_exe, tmp_path, cost, thresh), exact=False)


def test_rectangular_form_equals_brute_force():
    """the definition itself: the restatement's solver against every partial matching of small random problems."""
    import itertools
    rng = np.random.default_rng(0)
    for _ in range(60):
        n, m = int(rng.integers(1, 5)), int(rng.integers(1, 5))
        cost, thresh = rng.random((n, m)), float(rng.uniform(0.3, 0.9))
        best = 0.0
        for k in range(1, min(n, m) + 1):
            for rows in itertools.combinations(range(n), k):
                for cols in itertools.permutations(range(m), k):
                    if all(cost[r, c] <= thresh for r, c in zip(rows, cols)):
                        best = min(best, sum(cost[r, c] - thresh for r, c in zip(rows, cols)))
        assert abs(ref.solve_rect(cost, thresh)[1] - best) < 1e-12


def test_boxes_with_track_ids():
    from edge_yolo_amd.engine.results import Boxes
    d = torch.tensor([[1., 2., 3., 4., 7., 0.5, 2.], [5., 6., 7., 8., 9., 0.25, 1.]])
    b = Boxes(d, (10, 10))
    assert b.is_track and b.id.tolist() == [7.0, 9.0] and b.conf.tolist() == [0.5, 0.25] and b.cls.tolist() == [2.0, 1.0]
    assert b.xyxy.tolist() == d[:, :4].tolist() and b[1].id.tolist() == [9.0] and b[1].is_track
    plain = Boxes(d[:, [0, 1, 2, 3, 5, 6]], (10, 10))
    assert plain.id is None and not plain.is_track and plain.conf.tolist() == [0.5, 0.25]
    with pytest.raises(AssertionError):
        Boxes(torch.zeros(1, 8), (10, 10))


def test_tracker_settings(tmp_path):
    from edge_yolo_amd.trackers import DEFAULT_SETTINGS, load_settings
    assert load_settings(None) == DEFAULT_SETTINGS == ref.DEFAULTS and load_settings(None) is not DEFAULT_SETTINGS
    assert load_settings({"track_buffer": 5, "fuse_score": 0}) == {**DEFAULT_SETTINGS, "track_buffer": 5, "fuse_score": False}
    f = tmp_path / "mine.yaml"
    f.write_text("tracker_type: bytetrack\ntrack_high_thresh: 0.5\nmatch_thresh: 0.9\n")
    assert load_settings(str(f)) == {**DEFAULT_SETTINGS, "track_high_thresh": 0.5, "match_thresh": 0.9}
    with pytest.raises(NotImplementedError, match="botsort"):
        load_settings({"tracker_type": "botsort", "gmc_method": "sparseOptFlow"})
    with pytest.raises(ValueError):
        load_settings({"tracker_type": "sort"})
    with pytest.raises(ValueError, match="gmc_method"):
        load_settings({"gmc_method": "none"})
    with pytest.raises(TypeError):
        load_settings(3)


def test_track_refusals():
    import edge_yolo_amd
    x = torch.zeros(1, 3, 64, 64)
    for name in ("yolo11n-obb.yaml", "yolo11n-cls.yaml"):
        with pytest.raises(NotImplementedError, match="not tracked"):
            edge_yolo_amd.YOLO(name).track(x)
    det = edge_yolo_amd.YOLO("yolo11n-test.yaml")
    with pytest.raises(NotImplementedError, match="botsort"):
        det.track(x, tracker={"tracker_type": "botsort"})
    with pytest.raises(ValueError):
        det.track(x, tracker={"no_such_setting": 1})
    with pytest.raises(ValueError, match="source"):
        det.track(None)
    with pytest.raises(TypeError, match="unsupported"):
        det.track(x, no_such_option=1)
