"""Developer tool: time of ey_mask_contours for the masks of a segmentation result, next to the device-to-host copy of the same masks.

Cases: 300 blob masks of 640 x 640 (one image's worth, "batch 1"), 2400 of them (eight images, "batch 8"), and 300 masks of 1080 x 1920
(retina masks).  A mask is one smooth blob (blurred noise, thresholded) cropped to a box of about a quarter of the image, as process_mask
leaves it; 8 distinct masks per case, dealt to the rows in turn.  Per case:
  * kernel_ms: one ey_mask_contours launch (nn._ops.mask_contours_launch, with its workspace allocation), device events around windows of
    launches of at least 0.2 s after a warm-up, five windows, the median with min and max; once over the whole masks and once with boxes=;
  * polygons_ms: nn._ops.mask_contours as a user calls it -- launch, counts to the host, vertices to the host, split into arrays -- by a
    host clock around calls that end synchronised;
  * copy_ms: masks.cpu(), the same way: the floor of the reference's method, which traces contours on the host (cv2.findContours itself is
    not installed and cannot be timed); and the same copy into a pinned host buffer made beforehand, the best a host route could do.
One JSON line per case, printed and written to profiles/contours_bench.txt (or --out PATH)."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WINDOW_S, WINDOWS, DISTINCT = 0.2, 5, 8


def blob_masks(h, w, seed):
    """-> (uint8 (DISTINCT, h, w), float32 (DISTINCT, 4) xyxy boxes): one cropped blob per mask."""
    import numpy as np
    from scipy import ndimage
    rng = np.random.default_rng(seed)
    masks, boxes = np.zeros((DISTINCT, h, w), np.uint8), np.zeros((DISTINCT, 4), np.float32)
    for k in range(DISTINCT):
        bh, bw = int(h * rng.uniform(0.35, 0.6)), int(w * rng.uniform(0.35, 0.6))
        y0, x0 = int(rng.integers(0, h - bh)), int(rng.integers(0, w - bw))
        f = ndimage.gaussian_filter(rng.standard_normal((bh, bw)), min(bh, bw) / 24.0)
        yy, xx = np.mgrid[:bh, :bw]
        bump = 1.0 - (((yy - bh / 2) / (bh / 2)) ** 2 + ((xx - bw / 2) / (bw / 2)) ** 2)  # positive inside the box's ellipse
        masks[k, y0:y0 + bh, x0:x0 + bw] = (f / f.std() + 1.5 * bump) > 0.6
        boxes[k] = (x0 + 0.3, y0 + 0.6, x0 + bw - 0.2, y0 + bh - 0.7)
    return masks, boxes


def _device_windows(run_once):
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
            torch.cuda.synchronize()
            if time.perf_counter() - t0 >= WINDOW_S:
                break
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / reps)
    return [round(v, 3) for v in (statistics.median(out), min(out), max(out))]


def _host_windows(run_once):
    """run_once() ends synchronised (it brings data to the host)."""
    import torch
    run_once()
    out = []
    for _ in range(WINDOWS):
        torch.cuda.synchronize()
        reps, t0 = 0, time.perf_counter()
        while True:
            run_once()
            reps += 1
            if time.perf_counter() - t0 >= WINDOW_S:
                break
        out.append((time.perf_counter() - t0) * 1e3 / reps)
    return [round(v, 3) for v in (statistics.median(out), min(out), max(out))]


def case(name, n, h, w):
    import torch
    from edge_yolo_amd.nn import _ops
    m, b = blob_masks(h, w, seed=h)
    reps = -(-n // DISTINCT)
    masks = torch.from_numpy(m).cuda().repeat(reps, 1, 1)[:n].contiguous()
    boxes = torch.from_numpy(b).cuda().repeat(reps, 1)[:n].contiguous()
    res = _ops.mask_contours(masks)
    assert all(len(a) == len(c) and all((p == q).all() for p, q in zip(a, c)) for a, c in zip(res, _ops.mask_contours(masks, boxes=boxes)))
    vertices = sum(len(c) for r in res for c in r)
    ccap = max(len(r) for r in res)
    vcap = max(sum(len(c) for c in r) for r in res)
    win = torch.cat([boxes[:, :2].floor(), boxes[:, 2:].ceil()], 1).to(torch.int32).contiguous()
    out = {"case": name, "masks": n, "h": h, "w": w, "mask_bytes": n * h * w, "contours": sum(len(r) for r in res), "vertices": vertices, "vertex_bytes": vertices * 8,
           "kernel_ms_whole_mask": _device_windows(lambda: _ops.mask_contours_launch(masks, None, ccap, vcap)),
           "kernel_ms_with_boxes": _device_windows(lambda: _ops.mask_contours_launch(masks, win, ccap, vcap)),
           "polygons_ms_whole_mask": _host_windows(lambda: _ops.mask_contours(masks)),
           "polygons_ms_with_boxes": _host_windows(lambda: _ops.mask_contours(masks, boxes=boxes)),
           "copy_ms_masks_to_host": _host_windows(lambda: masks.cpu())}
    pinned = torch.empty(masks.shape, dtype=masks.dtype, pin_memory=True)

    def to_pinned():
        pinned.copy_(masks, non_blocking=True)
        torch.cuda.synchronize()

    out["copy_ms_masks_to_pinned_host"] = _host_windows(to_pinned)
    out["note"] = "each timing: median, min, max in ms; masks.cpu() goes to pageable host memory, the pinned copy into a buffer allocated before the clock starts"
    del masks, pinned
    torch.cuda.empty_cache()
    return out


def main():
    out = os.path.join(ROOT, "profiles", "contours_bench.txt")
    if "--out" in sys.argv:
        out = sys.argv[sys.argv.index("--out") + 1]
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("contours_bench: no GPU; nothing is measured without one")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    lines = []
    for name, n, h, w in (("640x640 batch 1", 300, 640, 640), ("640x640 batch 8", 2400, 640, 640), ("1080x1920 retina", 300, 1080, 1920)):
        lines.append(json.dumps(case(name, n, h, w)))
        print(lines[-1], flush=True)
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
