"""Developer tool: time ey_ghost_conv (a 1x1 GhostConv as one launch) at the 1x1 GhostConv shapes of yolov8n-ghost and yolov8s-ghost (640^2 input,
batch 32, f16), without and with the residual of a GhostBottleneck, against the composed form it replaces -- ey_conv2d into the first half of
the output, ey_dwconv (the direct kernel at hidden widths that are no multiples of 8) from there into the second half, and with a residual
both into a scratch map plus ey_cbfuse as the elementwise add: only kernels that exist without ey_ghost_conv, the yardstick -- and
YOLO(...).predict() of yolov8n, yolov8n-ghost and yolov8s-ghost next to yolo11n in images/s (batch 32, 640^2, f16, device tensors, captured
graph) with the launches of one device step, in the same run.

Both forms are replayed from a hipGraph that walks a rotation of buffers larger than the Infinity Cache; the timed windows are about 0.2 s each
and alternate between the two forms (five each, the median is reported, min and max next to it).  The composed form's scratch map comes from
the allocator inside the captured graph, as in a model's forward.  One JSON line per shape with the time per call against the algorithmic
bytes of each form (every input read once, every output written once; the composed form also reads the 1x1's output back, and with a residual
writes and reads the scratch map) and the MI355X's 8 TB/s HBM.  The lines are printed and written to profiles/ghost_bench.txt (or --out PATH).

Every shape and every model runs in a child process of its own under a time limit; the parent never opens the GPU (it builds the two models on
the CPU to list their shapes) and stops at the first child that fails or runs out of time.
usage: ghost_bench.py [--out PATH] [reps]             (all shapes, all models)
       ghost_bench.py --ghost C1 Ch H W RES reps     (one shape, what the children run)
       ghost_bench.py --model NAME"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 32
GHOST_MODELS = ["yolov8n-ghost.yaml", "yolov8s-ghost.yaml"]
MODELS = ["yolov8n.yaml", "yolov8n-ghost.yaml", "yolov8s-ghost.yaml", "yolo11n.yaml"]
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


def ghost_shapes(name, imgsz=640):
    """[(C1, Ch, H, W, res, count)]: the distinct 1x1 GhostConv calls of one forward, on the CPU.  res: the GhostConv closes a GhostBottleneck."""
    sys.path.insert(0, ROOT)
    from edge_yolo_amd.nn.modules import GhostBottleneck, GhostConv
    from edge_yolo_amd.nn.tasks import DetectionModel
    m = DetectionModel(name)
    seen = {}
    for layer in m.model:
        hw = int(imgsz / m._down[layer.i])
        closing = {id(g.conv[2]) for g in layer.modules() if isinstance(g, GhostBottleneck)}
        for g in layer.modules():
            if isinstance(g, GhostConv) and g.cv1.conv.kernel_size == (1, 1):
                key = (g.cv1.conv.in_channels, g.cv1.conv.out_channels, hw, hw, int(id(g) in closing))
                seen[key] = seen.get(key, 0) + 1
    return [k + (n,) for k, n in seen.items()]


def one_ghost(C1, Ch, H, W, res, reps):
    import torch
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import edge_yolo_amd  # noqa: F401
    import synthdata as synth
    from edge_yolo_amd import _lib as L
    from edge_yolo_amd.nn import _ops as ops
    from edge_yolo_amd.nn.modules import GhostConv
    with torch.no_grad():
        torch.manual_seed(0)
        m = GhostConv(C1, 2 * Ch, act=not res)  # the closing GhostConv of a bottleneck has no activation
        m.load_state_dict(synth.synth_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}))
        m = m.cuda().half().eval()
        px = B * H * W
        wbytes = 2 * (C1 * Ch + 25 * Ch)
        fused_bytes = 2 * px * (C1 + 2 * Ch + (2 * Ch if res else 0)) + wbytes
        two_bytes = fused_bytes + 2 * px * (5 * Ch if res else Ch)
        nsets = max(2, -(-WORKING_SET // two_bytes))
        xs = [torch.randn(B, H, W, C1, device="cuda", dtype=torch.float16).permute(0, 3, 1, 2) for _ in range(nsets)]
        rs = [torch.randn(B, H, W, 2 * Ch, device="cuda", dtype=torch.float16).permute(0, 3, 1, 2) if res else None for _ in range(nsets)]
        ys = [L.empty_nhwc(B, 2 * Ch, H, W, torch.float16, "cuda") for _ in range(nsets)]
        y2 = L.empty_nhwc(B, 2 * Ch, H, W, torch.float16, "cuda")

        def fused(x, r, y):
            if ops.ghost_conv(m.cv1, m.cv2, x, out=y, res=r) is None:
                raise RuntimeError("ey_ghost_conv refused the shape")

        def two(x, r, y):
            L.check(L.lib().ey_tune_set(b"ghost", 0), "tune")
            try:
                m(x, out=y, res=r)
            finally:
                L.check(L.lib().ey_tune_set(b"ghost", 1), "tune")

        t_f, t_t, calls = _compare(torch, reps, [lambda x=x, r=r, y=y: fused(x, r, y) for x, r, y in zip(xs, rs, ys)], [lambda x=x, r=r, y=y: two(x, r, y) for x, r, y in zip(xs, rs, ys)])
        fused(xs[0], rs[0], ys[0])
        two(xs[0], rs[0], y2)
        same = bool(torch.equal(ys[0], y2))
        f, t = sorted(t_f)[2], sorted(t_t)[2]
        return dict(what="ghost_conv", B=B, C1=C1, Ch=Ch, H=H, W=W, res=bool(res), buffer_sets=nsets, working_set_MB=round(nsets * two_bytes / 1e6), calls_per_window=calls,
                    fused_us=round(f, 1), fused_us_min=round(min(t_f), 1), fused_us_max=round(max(t_f), 1), fused_alg_MB=round(fused_bytes / 1e6, 1),
                    fused_hbm_floor_us=round(fused_bytes / HBM * 1e6, 1), fused_share_of_hbm_roof=round(fused_bytes / HBM * 1e6 / f, 3),
                    composed_us=round(t, 1), composed_us_min=round(min(t_t), 1), composed_us_max=round(max(t_t), 1), composed_launches=3 if res else 2,
                    composed_alg_MB=round(two_bytes / 1e6, 1), composed_hbm_floor_us=round(two_bytes / HBM * 1e6, 1),
                    composed_share_of_hbm_roof=round(two_bytes / HBM * 1e6 / t, 3), composed_over_fused=round(t / f, 2), bits_equal=same)


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
    return dict(model=name, batch=B, imgsz=640, half=True, calls_per_window=calls, windows=windows, ms_per_batch=round(med * 1e3, 3),
                ms_min=round(min(ts) * 1e3, 3), ms_max=round(max(ts) * 1e3, 3), images_per_s=round(B / med, 1), launches=sum(agg.values()),
                ghost_conv_launches=agg.get("ghost_conv_kernel", 0), detections=sum(len(r) for r in res))


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
    if argv and argv[0] == "--ghost":
        print(json.dumps(one_ghost(*(int(a) for a in argv[1:7]))), flush=True)
        sys.exit(0)
    if argv and argv[0] == "--model":
        print(json.dumps(one_model(argv[1])), flush=True)
        sys.exit(0)
    out = os.path.join(ROOT, "profiles", "ghost_bench.txt")
    if argv and argv[0] == "--out":
        out, argv = argv[1], argv[2:]
    reps = int(argv[0]) if argv else 48
    with open(out, "w") as f:
        def emit(line):
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
        emit(f"# tools/ghost_bench.py: ey_ghost_conv vs the composed form (ey_conv2d + ey_dwconv / direct [+ ey_cbfuse]), batch {B}, f16, 640x640 input; median of 5 windows")
        for name in GHOST_MODELS:
            for C1, Ch, H, W, res, n in ghost_shapes(name):
                emit(f"# {name[:-5]}: GhostConv {C1} -> 2 x {Ch}, {H}x{W}{', + residual' if res else ''} ({n} per forward)")
                emit(_child(["--ghost", str(C1), str(Ch), str(H), str(W), str(res), str(reps)], f"ghost_conv {C1}->{Ch} {H}x{W} res={res}"))
        emit(f"# predict(): batch {B}, 640x640, f16, device tensors, captured graph; median of 5 windows of 20 calls; launches of one device step")
        for name in MODELS:
            emit(_child(["--model", name], name))
