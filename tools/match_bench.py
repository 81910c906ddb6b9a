"""Developer tool: what the validation matching costs on the host and on the device, at batch 32 with 300 kept rows per image and 7 / 20 / 60
labels per image (validation NMS at conf 0.001 fills max_det).  Per label count:
  * kernel_ms: one ey_match_batch launch giving the true positives at the ten thresholds AND the confusion matrix (boxes mode with xform),
    device events around windows of about 0.2 s of launches enqueued back to back (no host synchronisation inside a window; where the host
    cannot enqueue as fast as the kernel runs, the figure is the launch rate), five windows, the median with min and max;
  * update_off_ms / update_on_ms: DetectionValidator.update_metrics on the same device rows with both keywords off (the host route:
    per-image copies, numpy box_iou and match_predictions -- the baseline) and with confusion_matrix=True, device_match=True, by a host
    clock around calls that end synchronised, the median of 9 after a warm-up.
And once: val() images/s of yolo11n at 640 x 640, f16, over a synthetic loader of 4 batches of 32 with 20 labels per image, both ways.
One JSON line per measurement, printed and written to profiles/match_bench.txt (or --out PATH).
One workgroup per image leaves most of the card idle at batch 32 (32 of 256 CUs): the kernel time is a latency, not a throughput."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
WINDOW_S, WINDOWS, B, MAX_DET, IMG = 0.2, 5, 32, 300, 640


def _device_windows(run_once):
    """Kernel time: device events around `reps` launches enqueued back to back (no host synchronisation between them), reps sized so that a
    window lasts about WINDOW_S; -> [median, min, max] ms per launch over WINDOWS windows."""
    import torch
    for _ in range(3):
        run_once()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(20):
        run_once()
    torch.cuda.synchronize()
    reps = max(20, min(5000, int(WINDOW_S / ((time.perf_counter() - t0) / 20))))
    out = []
    for _ in range(WINDOWS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            run_once()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / reps)
    return [round(v, 4) for v in (statistics.median(out), min(out), max(out))]


def _host_median(run_once, n=9):
    import torch
    run_once()
    torch.cuda.synchronize()
    ts = []
    for _ in range(n):
        t0 = time.perf_counter()
        run_once()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return [round(v, 3) for v in (statistics.median(ts), min(ts), max(ts))]


def batch_of(labels, seed):
    """-> (rows per image on the host (300, 6) in the 640 x 640 input frame, the label part of a batch): jittered copies of the labels plus
    strays, as tests/confusion_synth.py draws them."""
    import numpy as np
    import confusion_synth as S
    rows, cls, box, bi = [], [], [], []
    for i in range(B):
        c = S.case((f"b{i}", MAX_DET, labels, 80, False), seed + i)
        k = IMG / np.array([S.IMGSZ[1], S.IMGSZ[0]] * 2, np.float32)
        d = c["det"].copy()
        d[:, :4] *= k
        d = d[np.argsort(-d[:, 4], kind="stable")]
        g = c["gt"] * k
        rows.append(d)
        cls.append(c["gt_cls"].reshape(-1, 1))
        box.append(np.stack([(g[:, 0] + g[:, 2]) / 2, (g[:, 1] + g[:, 3]) / 2, g[:, 2] - g[:, 0], g[:, 3] - g[:, 1]], 1) / IMG)
        bi.append(np.full(labels, i, np.float32))
    return rows, {"cls": np.concatenate(cls), "bboxes": np.concatenate(box).astype(np.float32), "batch_idx": np.concatenate(bi),
                  "ori_shape": [(IMG, IMG)] * B, "ratio_pad": None}


def main():
    import numpy as np
    import torch
    import edge_yolo_amd
    import synthdata as synth
    from edge_yolo_amd.engine.validator import DetectionValidator
    from edge_yolo_amd.nn import _ops
    from edge_yolo_amd.utils import metrics
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "match_bench.txt")
    lines = []

    def emit(d):
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)

    y = edge_yolo_amd.YOLO("yolo11n.yaml")
    y.model.load_state_dict(synth.synth_state_dict({k: tuple(t.shape) for k, t in y.model.state_dict().items()}))
    model = y._ready(torch.device("cuda:0"), True)
    img = torch.zeros(B, 3, IMG, IMG)
    for labels in (7, 20, 60):
        rows, batch = batch_of(labels, 1000 * labels)
        batch["img"] = img
        dev_rows = torch.from_numpy(np.stack(rows)).cuda()
        count = torch.full((B,), MAX_DET, dtype=torch.int32).cuda()
        off, on = DetectionValidator(model, half=True), DetectionValidator(model, half=True, confusion_matrix=True, device_match=True)
        pb = [on._prepare_batch(si, batch) for si in range(B)]
        gt = torch.from_numpy(np.concatenate([p["bbox"] for p in pb]).astype(np.float32)).cuda()
        cls = torch.from_numpy(np.concatenate([p["cls"] for p in pb]).astype(np.int32)).cuda()
        gt_off = [labels * i for i in range(B + 1)]
        xform = torch.from_numpy(np.asarray([on._xform(p) for p in pb], np.float32)).cuda()
        tp = torch.zeros((B, MAX_DET, 10), dtype=torch.uint8).cuda()
        matrix = torch.zeros(81 * 81, dtype=torch.int32).cuda()
        kernel = _device_windows(lambda: _ops.match_batch(dev_rows, count, cls, gt_off, metrics.IOUV, 80, gt=gt, xform=xform, tp=tp, matrix=matrix))

        def update(v):
            v.init_metrics()
            n = [MAX_DET] * B
            kept = [dev_rows[i, :n[i]] for i in range(B)]
            v._stash = (dev_rows, count, n, kept)  # (what postprocess leaves behind)
            v.update_metrics(kept, batch)

        t_off, t_on = _host_median(lambda: update(off)), _host_median(lambda: update(on))
        same = all(np.array_equal(a, b) for a, b in zip(off.stats["tp"], on.stats["tp"]))
        emit({"case": "update_metrics", "batch": B, "rows_per_image": MAX_DET, "labels_per_image": labels, "kernel_ms_med_min_max": kernel,
              "update_off_ms_med_min_max": t_off, "update_on_ms_med_min_max": t_on, "speedup": round(t_off[0] / t_on[0], 2), "same_tp": bool(same),
              "tp50": int(np.concatenate(on.stats["tp"])[:, 0].sum()), "note": "one workgroup per image: 32 of 256 CUs busy"})
    # val() end to end: yolo11n, 640 x 640, f16, 4 batches of 32 with 20 labels per image
    loader = []
    for j in range(4):
        _, batch = batch_of(20, 5000 + 100 * j)
        batch["img"] = synth.synth_images(B, IMG, IMG, seed=40 + j)
        loader.append(batch)
    for kw in ({}, {"confusion_matrix": True, "device_match": True}):
        y.val(loader, half=True, device="cuda:0", **kw)  # warm-up
        torch.cuda.synchronize()
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            res = y.val(loader, half=True, device="cuda:0", **kw)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        kept = sum(len(a) for a in y.validator.stats["conf"])
        emit({"case": "val", "model": "yolo11n", "imgsz": IMG, "batch": B, "batches": 4, "labels_per_image": 20, "flags": kw, "images_per_s": round(4 * B / min(ts), 1),
              "seconds_min_max": [round(min(ts), 4), round(max(ts), 4)], "kept_rows": int(kept), "mAP50": res["metrics/mAP50(B)"]})
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
