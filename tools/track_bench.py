"""Developer tool: time per frame of ey_bytetrack_update (one launch per frame for all streams) for B = 1, 8 and 32 streams of about 20, 100
and 300 detections per frame, over 60-frame synthetic sequences (tests/track_synth.scene: linear motion, jitter, misses, demoted scores,
clutter; at most 4 distinct scenes per configuration, dealt to the streams in turn), and of ey_linear_assignment on single problems of
128 x 128, 300 x 300 and 1024 x 300 dense random costs with thresh 0.8.

Device times are device events around whole sequences (60 launches each, the state reset between sequences included: four memsets) after one
warm-up sequence, repeated until a window lasts 0.2 s; five windows, the median with min and max.  Next to each tracker case stands the
float64 host restatement (tests/fp64_track_ref.py) fed by a device-to-host copy of the same rows, timed on ONE stream with a host clock
and multiplied by B (a host tracker walks its streams one after the other).  The restatement is the reference's algorithm -- per-object
Python, numpy, scipy's assignment -- but not the reference's code: its Kalman update is written out in Python loops and is slower than the
reference's vectorised numpy, so the ratio is a yardstick for "tracking on the host behind this predictor", not a claim about the reference.

One workgroup (256 lanes) works per stream: at B = 32 that is 32 of the card's 256 compute units, and inside a workgroup the solver is a
chain of dependent steps.  The figures say what that costs.  One JSON line per case, printed and written to profiles/track_bench.txt (or
--out PATH)."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
FRAMES, WINDOW_S, WINDOWS = 60, 0.2, 5
SCENES = {20: (20, 1280, 960), 100: (100, 2560, 1920), 300: (300, 3840, 2880)}  # detections per frame -> objects, width, height
CAP, MAX_TRACKS = 320, 1024
_HOST_MS = {}


def _windows(run_once, unit):
    """median / min / max time per `unit` of run_once() (which enqueues `unit` units of work), over WINDOWS windows of >= WINDOW_S."""
    import torch
    run_once()
    torch.cuda.synchronize()
    out = []
    for _ in range(WINDOWS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        reps, t0 = 0, time.perf_counter()
        a.record()
        while True:
            run_once()
            reps += 1
            if reps % 4 == 0 or reps == 1:
                torch.cuda.synchronize()
                if time.perf_counter() - t0 >= WINDOW_S:
                    break
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / (reps * unit))
    return statistics.median(out), min(out), max(out)


def tracker_case(B, ndet):
    import numpy as np
    import torch
    import fp64_track_ref as ref
    import track_synth as ts
    from edge_yolo_amd.trackers import BYTETracker
    nobj, w, h = SCENES[ndet]
    scenes = [ts.scene(100 + k, nobj, w, h, frames=FRAMES) for k in range(min(B, 4))]
    rows = np.zeros((FRAMES, B, CAP, 6), np.float32)
    count = np.zeros((FRAMES, B), np.int32)
    for b in range(B):
        for f, r in enumerate(scenes[b % len(scenes)]):
            k = min(len(r), CAP)
            rows[f, b, :k], count[f, b] = r[:k], k
    drows, dcount = torch.from_numpy(rows).cuda(), torch.from_numpy(count).cuda()
    tr = BYTETracker(streams=B, max_det=CAP, max_tracks=MAX_TRACKS, device="cuda:0")

    def sequence():
        tr.reset()
        for f in range(FRAMES):
            tr.update(drows[f], dcount[f])

    med, lo, hi = _windows(sequence, FRAMES)
    tracks = int((tr.state["slot_i"][:, :, 0] != 0).sum()) / B
    # the host: copy the rows of one stream back frame by frame and run the restatement on them
    if ndet not in _HOST_MS:  # (stream 0 sees the same scene at every B: timed once)
        host = ref.RefTracker(max_tracks=MAX_TRACKS)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for f in range(FRAMES):
            k = int(dcount[f, 0])
            host.update(drows[f, 0, :k].cpu().numpy())
        _HOST_MS[ndet] = (time.perf_counter() - t0) * 1e3 / FRAMES
    host_ms = _HOST_MS[ndet]
    return {"case": "bytetrack_update", "streams": B, "detections_per_frame": round(float(count.mean()), 1), "live_slots_per_stream_at_end": round(tracks, 1),
            "device_ms_per_frame": round(med, 4), "min": round(lo, 4), "max": round(hi, 4), "device_us_per_stream_frame": round(med * 1e3 / B, 2),
            "host_restatement_ms_per_frame_one_stream": round(host_ms, 3), "host_restatement_ms_per_frame_all_streams": round(host_ms * B, 3),
            "host_over_device": round(host_ms * B / med, 1)}


def assignment_case(n, m):
    import numpy as np
    import torch
    from scipy.optimize import linear_sum_assignment
    from edge_yolo_amd.nn import _ops
    c = np.random.default_rng([n, m]).random((n, m)).astype(np.float32)
    x = torch.from_numpy(c).cuda()
    out = (torch.empty((1, n), dtype=torch.int32, device="cuda"), torch.empty((1, m), dtype=torch.int32, device="cuda"))
    med, lo, hi = _windows(lambda: _ops.linear_assignment([x], 0.8, out=out), 1)
    t0 = time.perf_counter()
    for _ in range(5):
        linear_sum_assignment(c.astype(np.float64))
    scipy_ms = (time.perf_counter() - t0) * 1e3 / 5
    return {"case": "linear_assignment", "n": n, "m": m, "matched": int((out[0] >= 0).sum()), "device_ms": round(med, 4), "min": round(lo, 4), "max": round(hi, 4),
            "scipy_linear_sum_assignment_ms_host": round(scipy_ms, 4),
            "note": "the device time includes the wrapper's two small host-to-device copies (descriptor, threshold) and a workspace allocation"}


def main():
    out = os.path.join(ROOT, "profiles", "track_bench.txt")
    if "--out" in sys.argv:
        out = sys.argv[sys.argv.index("--out") + 1]
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("track_bench: no GPU; nothing is measured without one")
    lines = []
    for B in (1, 8, 32):
        for ndet in (20, 100, 300):
            lines.append(json.dumps(tracker_case(B, ndet)))
            print(lines[-1], flush=True)
    for n, m in ((128, 128), (300, 300), (1024, 300)):
        lines.append(json.dumps(assignment_case(n, m)))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
