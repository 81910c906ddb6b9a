"""Developer tool: time ey_mask_prompt (FastSAM's prompt selection: weights, scores and selection, three launches) at 300 masks per image,
640 x 640 masks, 1080 x 1920 originals, 4 boxes and 4 points, at batch 1 and 8, against the PyTorch composition of the reference's
expression on the same device (F.interpolate to the original size, then slice sums and point reads: predict.py:72-101), a yardstick
only, at batch 1 -- it needs 2.5 GB per image for the resized masks; and FastSAM("FastSAM-s.yaml").predict() with and without prompts next
to YOLO("yolov8s-seg.yaml").predict() in images/s (batch 32, 640^2, f16, device tensors, captured graph), in the same run.

The masks are one filled rectangle each, of 2 % to 30 % of the image side, as ey_process_mask leaves them after the box crop; the kernel
skips 16-byte words that are all clear, so the time depends on how many are set and the share is printed.  The kernel is replayed from a
hipGraph that walks a rotation of mask sets larger than the Infinity Cache; timed windows of about 0.2 s, five per form, the median is
reported with min and max.  One JSON line per case with the time per call against the algorithmic bytes (every mask byte read once) and
the MI355X's 8 TB/s HBM.  The lines are printed and written to profiles/fastsam_bench.txt (or --out PATH).

Every case runs in a child process of its own under a time limit; the parent never opens the GPU and stops at the first child that fails
or runs out of time.
usage: fastsam_bench.py [--out PATH]          (all cases)
       fastsam_bench.py --kernel B             (one batch size, what the children run)
       fastsam_bench.py --model NAME PROMPTS   (one model; PROMPTS 0 or 1)"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_PER, MH, MW, H0, W0 = 300, 640, 640, 1080, 1920
BOXES = [[100, 80, 700, 600], [0, 0, 1920, 1080], [1500, 700, 1930, 1090], [960, 540, 961, 541]]
POINTS, LABELS = [[200, 200], [1000, 500], [1800, 1000], [5, 5]], [1, 0, 1, 1]
HBM = 8.0e12
WORKING_SET = 600 << 20  # bytes the rotated mask sets cover: more than twice the 256 MB Infinity Cache
WINDOW_S = 0.2
CHILD_TIMEOUT = 240  # seconds per child


def make_masks(n, seed):
    import torch
    g = torch.Generator().manual_seed(seed)
    m = torch.zeros((n, MH, MW), dtype=torch.uint8)
    for k in range(n):
        h, w = (int(v) for v in (torch.rand(2, generator=g) * 0.28 + 0.02) * torch.tensor([MH, MW]))
        y, x = int(torch.rand(1, generator=g) * (MH - h)), int(torch.rand(1, generator=g) * (MW - w))
        m[k, y:y + h, x:x + w] = 1
    return m


def torch_form(masks, boxes, points, labels):
    """predict.py:72-101 with torch operators: resize, areas, IoU argmax, point reads -> keep."""
    import torch
    import torch.nn.functional as F
    sys.path.insert(0, ROOT)
    from edge_yolo_amd.nn._ops import mask_geometry
    top, bottom, left, right, _, _ = mask_geometry((MH, MW), (H0, W0))
    r = F.interpolate(masks[None, :, top:bottom, left:right].float(), (H0, W0), mode="bilinear", align_corners=False)[0]
    idx = torch.zeros(len(r), dtype=torch.bool, device=r.device)
    area = (boxes[:, 3] - boxes[:, 1]) * (boxes[:, 2] - boxes[:, 0])
    inter = torch.stack([r[:, b[1]:b[3], b[0]:b[2]].sum(dim=(1, 2)) for b in boxes.tolist()])
    full = r.sum(dim=(1, 2))
    idx[torch.argmax(inter / (area[:, None] + full - inter), dim=1)] = True
    pk = torch.zeros(len(r), dtype=torch.bool, device=r.device)
    for p, lab in zip(points.tolist(), labels):
        pk[torch.nonzero(r[:, p[1], p[0]], as_tuple=True)[0]] = bool(lab)
    return idx | pk


def one_kernel(B, reps=20):
    import torch
    sys.path.insert(0, ROOT)
    import edge_yolo_amd  # noqa: F401
    from edge_yolo_amd.nn import _ops as ops

    def window(g, k):
        st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        st.record()
        for _ in range(k):
            g.replay()
        en.record()
        torch.cuda.synchronize()
        return st.elapsed_time(en) * 1000 / (k * reps)

    with torch.no_grad():
        nbytes = B * N_PER * MH * MW
        nsets = max(2, -(-WORKING_SET // nbytes))
        host = [make_masks(N_PER, s) for s in range(min(B * nsets, 4))]  # (four different images, repeated)
        sets = [torch.cat([host[(s * B + b) % len(host)] for b in range(B)]).cuda() for s in range(nsets)]
        off, shapes = [N_PER * b for b in range(B + 1)], [(H0, W0)] * B
        ws = torch.empty(1 << 22, dtype=torch.uint8, device="cuda")
        outs = [ops.mask_prompt(m, off, shapes, BOXES, POINTS, LABELS, workspace=ws) for m in sets]
        fns = [lambda m=m, o=o: ops.mask_prompt(m, off, shapes, BOXES, POINTS, LABELS, out=o, workspace=ws) for m, o in zip(sets, outs)]
        for _ in range(3):
            for fn in fns:
                fn()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for i in range(reps):
                fns[i % len(fns)]()
        g.replay()
        torch.cuda.synchronize()
        k = max(1, int(WINDOW_S * 1e6 / (window(g, 1) * reps)) + 1)
        t_hip = [window(g, k) for _ in range(5)]
        hip = sorted(t_hip)[2]
        d = dict(B=B, masks_per_image=N_PER, mask=[MH, MW], original=[H0, W0], boxes=len(BOXES), points=len(POINTS), set_bytes_share=round(float(sets[0].float().mean()), 4),
                 buffer_sets=nsets, working_set_MB=round(nsets * nbytes / 1e6), calls_per_window=reps * k, hip_us=round(hip, 1), hip_us_min=round(min(t_hip), 1),
                 hip_us_max=round(max(t_hip), 1), alg_MB=round(nbytes / 1e6, 1), hbm_floor_us=round(nbytes / HBM * 1e6, 1), achieved_TBps=round(nbytes / hip / 1e6, 2),
                 share_of_hbm_roof=round(nbytes / HBM * 1e6 / hip, 3))
        if B == 1:  # the composition: eager (it allocates 2.5 GB per call), five timed calls after two warm-up calls
            bx, pt = torch.tensor(BOXES, device="cuda"), torch.tensor(POINTS, device="cuda")
            ts = []
            for i in range(7):
                st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                st.record()
                keep = torch_form(sets[i % nsets], bx, pt, LABELS)
                en.record()
                torch.cuda.synchronize()
                ts.append(st.elapsed_time(en) * 1000)
            tor = sorted(ts[2:])[2]
            same = bool(torch.equal(torch_form(sets[0], bx, pt, LABELS), outs[0]["keep"].bool()))
            d.update(torch_us=round(tor, 1), torch_us_min=round(min(ts[2:]), 1), torch_us_max=round(max(ts[2:]), 1), torch_over_hip=round(tor / hip, 1),
                     torch_peak_MB=round(torch.cuda.max_memory_allocated() / 1e6), same_selection_as_torch=same)
        return d


def one_model(name, prompts, warmup=5, calls=10, windows=5):
    import time

    import torch
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import edge_yolo_amd
    import seg_synth
    import synthdata as synth
    fast = name.startswith("FastSAM")
    model = (edge_yolo_amd.FastSAM if fast else edge_yolo_amd.YOLO)(name)
    model.model.load_state_dict(seg_synth.state_dict(model.model.state_dict()))
    x = synth.synth_images(32, 640, 640).cuda().half()
    kw = dict(conf=0.25, iou=0.7, half=True, device="cuda:0")
    if prompts:
        kw.update(bboxes=[[60, 50, 400, 300], [0, 0, 640, 640], [500, 400, 650, 650], [320, 320, 321, 321]], points=[[100, 100], [320, 250], [600, 600], [5, 5]], labels=LABELS)
    for _ in range(warmup):
        res = model.predict(x, **kw)
    torch.cuda.synchronize()
    ts = []
    for _ in range(windows):
        t0 = time.perf_counter()
        for _ in range(calls):
            res = model.predict(x, **kw)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) / calls)
    med = sorted(ts)[len(ts) // 2]
    return dict(model=name, prompts=bool(prompts), batch=32, imgsz=640, half=True, calls_per_window=calls, windows=windows, ms_per_batch=round(med * 1e3, 3),
                ms_min=round(min(ts) * 1e3, 3), ms_max=round(max(ts) * 1e3, 3), images_per_s=round(32 / med, 1), masks_before_prompts=sum(model.predictor._mask_counts),
                instances_returned=sum(len(r) for r in res))


def _child(args, what):
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, timeout=CHILD_TIMEOUT, stdout=subprocess.PIPE, text=True)
    except subprocess.TimeoutExpired:
        sys.exit(f"{what}: no result within {CHILD_TIMEOUT} s; stopping")
    if r.returncode != 0:
        sys.exit(f"{what}: exit status {r.returncode}; stopping")
    return [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]


if __name__ == "__main__":
    argv = sys.argv[1:]
    if argv and argv[0] == "--kernel":
        print(json.dumps(one_kernel(int(argv[1]))), flush=True)
        sys.exit(0)
    if argv and argv[0] == "--model":
        print(json.dumps(one_model(argv[1], int(argv[2]))), flush=True)
        sys.exit(0)
    out = os.path.join(ROOT, "profiles", "fastsam_bench.txt")
    if argv and argv[0] == "--out":
        out = argv[1]
    with open(out, "w") as f:
        def emit(line):
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
        emit(f"# tools/fastsam_bench.py: ey_mask_prompt, {N_PER} masks per image of {MH}x{MW}, originals {H0}x{W0}, {len(BOXES)} boxes and {len(POINTS)} points; median of 5 windows")
        for B in (1, 8):
            emit(_child(["--kernel", str(B)], f"kernel B{B}"))
        emit("# predict(): batch 32, 640x640, f16, device tensors, captured graph, synthetic weights; median of 5 windows of 10 calls")
        for name, prompts in (("yolov8s-seg.yaml", 0), ("FastSAM-s.yaml", 0), ("FastSAM-s.yaml", 1)):
            emit(_child(["--model", name, str(prompts)], f"{name} prompts={prompts}"))
