"""Developer tool: time ey_scdown (SCDown as one launch) at the SCDown shapes of yolov10n and yolov10s (640^2 input, batch 32, f16) against the two
launches it replaces, ey_conv2d + ey_dwconv_s2 with the full-resolution map in memory between them -- the yardstick -- and
YOLO("yolov10n") / YOLO("yolov10s").predict() next to YOLO("yolo11n").predict() in images/s (batch 32, 640^2, f16, device tensors, captured
graph) with the launches of one device step, in the same run.

Both forms are replayed from a hipGraph that walks a rotation of buffers larger than the Infinity Cache; the timed windows are about 0.2 s each
and alternate between the two forms (five each, the median is reported, min and max next to it).  One JSON line per shape with the time per
call against the algorithmic bytes of each form (every input read once, every output written once; the two-launch form also writes and reads
the map between the convs) and the MI355X's 8 TB/s HBM.  The lines are printed and written to profiles/v10_bench.txt (or --out PATH).

Every shape and every model runs in a child process of its own under a time limit; the parent never opens the GPU and stops at the first child
that fails or runs out of time.
usage: v10_bench.py [--out PATH] [reps]        (all shapes, all models)
       v10_bench.py --scdown C1 C2 H W reps    (one shape, what the children run)
       v10_bench.py --model NAME"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 32
# (scale, layer, C1, C2, H, W): the SCDown layers 5, 7 and 20 at 640x640
SCDOWN = [("n", 5, 64, 128, 80, 80), ("n", 7, 128, 256, 40, 40), ("n", 20, 128, 128, 40, 40),
          ("s", 5, 128, 256, 80, 80), ("s", 7, 256, 512, 40, 40), ("s", 20, 256, 256, 40, 40)]
MODELS = ["yolov10n.yaml", "yolov10s.yaml", "yolo11n.yaml"]
HBM = 8.0e12
WORKING_SET = 600 << 20  # bytes the rotated buffers cover: more than twice the 256 MB Infinity Cache
WINDOW_S = 0.2
CHILD_TIMEOUT = 300  # seconds per child


def _compare(torch, reps, fused_fns, two_fns):
    def graph_of(fns):
        """A hipGraph holding `reps` calls, walking round-robin over `fns` (one per buffer set), after 3 eager warm-up rounds."""
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
        return g

    def window(g, k):
        """us per call over k back-to-back replays between two events."""
        st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        st.record()
        for _ in range(k):
            g.replay()
        en.record()
        torch.cuda.synchronize()
        return st.elapsed_time(en) * 1000 / (k * reps)

    g_f, g_t = graph_of(fused_fns), graph_of(two_fns)
    k_f = max(1, int(WINDOW_S * 1e6 / (window(g_f, 1) * reps)) + 1)
    k_t = max(1, int(WINDOW_S * 1e6 / (window(g_t, 1) * reps)) + 1)
    t_f, t_t = [], []
    for _ in range(5):  # alternate the two forms: a drift of the machine hits both
        t_f.append(window(g_f, k_f))
        t_t.append(window(g_t, k_t))
    return t_f, t_t, reps * k_f


def one_scdown(C1, C2, H, W, reps):
    import torch
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import edge_yolo_amd  # noqa: F401
    import synthdata as synth
    from edge_yolo_amd import _lib as L
    from edge_yolo_amd.nn import _ops as ops
    from edge_yolo_amd.nn.modules import SCDown
    with torch.no_grad():
        torch.manual_seed(0)
        m = SCDown(C1, C2, 3, 2)
        m.load_state_dict(synth.synth_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}))
        m = m.cuda().half().eval()
        Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        wbytes = 2 * (C1 * C2 + 9 * C2)
        fused_bytes = 2 * B * (H * W * C1 + Ho * Wo * C2) + wbytes
        two_bytes = fused_bytes + 2 * 2 * B * H * W * C2
        nsets = max(2, -(-WORKING_SET // two_bytes))
        xs = [torch.randn(B, H, W, C1, device="cuda", dtype=torch.float16).permute(0, 3, 1, 2) for _ in range(nsets)]
        mids = [L.empty_nhwc(B, C2, H, W, torch.float16, "cuda") for _ in range(nsets)]
        ys = [L.empty_nhwc(B, C2, Ho, Wo, torch.float16, "cuda") for _ in range(nsets)]
        y2 = L.empty_nhwc(B, C2, Ho, Wo, torch.float16, "cuda")

        def fused(x, y):
            if ops.scdown(m.cv1, m.cv2, x, out=y) is None:
                raise RuntimeError("ey_scdown refused the shape")

        def two(x, mid, y):
            ops.dwconv_s2(m.cv2, m.cv1(x, out=mid), m.cv2.folded, 3, L.ACT_NONE, out=y)

        t_f, t_t, calls = _compare(torch, reps, [lambda x=x, y=y: fused(x, y) for x, y in zip(xs, ys)], [lambda x=x, a=a, y=y: two(x, a, y) for x, a, y in zip(xs, mids, ys)])
        fused(xs[0], ys[0])
        two(xs[0], mids[0], y2)
        same = bool(torch.equal(ys[0], y2))
        f, t = sorted(t_f)[2], sorted(t_t)[2]
        return dict(what="scdown", B=B, C1=C1, C2=C2, H=H, W=W, buffer_sets=nsets, working_set_MB=round(nsets * two_bytes / 1e6), calls_per_window=calls,
                    fused_us=round(f, 1), fused_us_min=round(min(t_f), 1), fused_us_max=round(max(t_f), 1), fused_alg_MB=round(fused_bytes / 1e6, 1),
                    fused_hbm_floor_us=round(fused_bytes / HBM * 1e6, 1), fused_share_of_hbm_roof=round(fused_bytes / HBM * 1e6 / f, 3),
                    two_launch_us=round(t, 1), two_launch_us_min=round(min(t_t), 1), two_launch_us_max=round(max(t_t), 1), two_launch_alg_MB=round(two_bytes / 1e6, 1),
                    two_launch_hbm_floor_us=round(two_bytes / HBM * 1e6, 1), two_launch_share_of_hbm_roof=round(two_bytes / HBM * 1e6 / t, 3),
                    two_launch_over_fused=round(t / f, 2), bits_equal=same)


def one_model(name, warmup=5, calls=20, windows=5):
    import time

    import torch
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import edge_yolo_amd
    import synthdata as synth
    from edge_yolo_amd import profiling
    model = edge_yolo_amd.YOLO(name)
    model.model.load_state_dict(synth.synth_state_dict({k: tuple(v.shape) for k, v in model.model.state_dict().items()}))
    x = synth.synth_images(B, 640, 640).cuda().half()
    kw = dict(conf=0.25, iou=0.7, half=True, device="cuda:0")
    for _ in range(warmup):
        res = model.predict(x, **kw)
    torch.cuda.synchronize()
    ts = []
    for _ in range(windows):
        t0 = time.perf_counter()
        for _ in range(calls):
            model.predict(x, **kw)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) / calls)
    med = sorted(ts)[len(ts) // 2]
    with profiling.trace() as tr:  # the launches of one eager device step (what the graph replays)
        model.predictor._device_step(x)
    torch.cuda.synchronize()
    agg = {}
    for r in tr.records:
        agg[r[0]] = agg.get(r[0], 0) + r[6]
    return dict(model=name, batch=B, imgsz=640, half=True, end2end=bool(model.model.end2end), calls_per_window=calls, windows=windows, ms_per_batch=round(med * 1e3, 3),
                ms_min=round(min(ts) * 1e3, 3), ms_max=round(max(ts) * 1e3, 3), images_per_s=round(B / med, 1), launches=sum(agg.values()),
                scdown_launches=agg.get("scdown_kernel", 0), detections=sum(len(r) for r in res))


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
    if argv and argv[0] == "--scdown":
        print(json.dumps(one_scdown(*(int(a) for a in argv[1:6]))), flush=True)
        sys.exit(0)
    if argv and argv[0] == "--model":
        print(json.dumps(one_model(argv[1])), flush=True)
        sys.exit(0)
    out = os.path.join(ROOT, "profiles", "v10_bench.txt")
    if argv and argv[0] == "--out":
        out, argv = argv[1], argv[2:]
    reps = int(argv[0]) if argv else 48
    with open(out, "w") as f:
        def emit(line):
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
        emit(f"# tools/v10_bench.py: ey_scdown vs ey_conv2d + ey_dwconv_s2, batch {B}, f16, 640x640 input; median of 5 windows")
        for scale, layer, C1, C2, H, W in SCDOWN:
            emit(f"# yolov10{scale} layer {layer}: SCDown {C1} -> {C2}, {H}x{W}")
            emit(_child(["--scdown", str(C1), str(C2), str(H), str(W), str(reps)], f"scdown {C1}->{C2} {H}x{W}"))
        emit(f"# predict(): batch {B}, 640x640, f16, device tensors, captured graph; median of 5 windows of 20 calls; launches of one device step")
        for name in MODELS:
            emit(_child(["--model", name], name))
