"""Developer tool: time ey_adown_pool at the three ADown shapes of yolov9c and ey_cbfuse at the five CBFuse shapes of yolov9e (640^2 input,
batch 32, f16), each against the PyTorch composition of the same operation on the same device and f16 data (NCHW, its own layout:
avg_pool2d / chunk / max_pool2d; interpolate / stack / sum), a yardstick only; and YOLO("yolov9t") / YOLO("yolov9c").predict() next to
YOLO("yolo11n").predict() in images/s (batch 32, 640^2, f16, device tensors, captured graph) with the launches of one device step, in the
same run.

Both kernel forms are replayed from a hipGraph that walks a rotation of buffers larger than the Infinity Cache; the timed windows are about
0.2 s each and alternate between the two forms (five each, the median is reported, min and max next to it).  One JSON line per shape with the
time per call against the algorithmic bytes of the call (every input read once, every output written once) and the MI355X's 8 TB/s HBM.  The
CBFuse sources are channel slices of buffers as wide as the CBLinear outputs they come from.  The lines are printed and written to
profiles/gelan_bench.txt (or --out PATH).

Every shape and every model runs in a child process of its own under a time limit; the parent never opens the GPU and stops at the first
child that fails or runs out of time.
usage: gelan_bench.py [--out PATH] [reps]      (all shapes, all models)
       gelan_bench.py --adown C H W reps       (one shape, what the children run)
       gelan_bench.py --cbfuse LEVEL reps
       gelan_bench.py --model NAME"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 32
ADOWN = [(256, 160, 160), (512, 80, 80), (512, 40, 40)]  # yolov9c layers 3 / 16, 5 / 19 and 7: the block's input
# yolov9e at 640x640: CBLinear layers 10-14 give maps of 320, 160, 80, 40, 20 pixels a side, 64 / 192 / 448 / 960 / 1984 channels wide in all;
# CBFuse layer 16 + 2 L takes slice L (64 << L channels, at channel offset 64 (2^L - 1)) of each CBLinear from the L-th on, plus the main branch
CBL_SIDE, CBL_WIDTH = [320, 160, 80, 40, 20], [64, 192, 448, 960, 1984]
MODELS = ["yolov9t.yaml", "yolov9c.yaml", "yolo11n.yaml"]
HBM = 8.0e12
WORKING_SET = 600 << 20  # bytes the rotated buffers cover: more than twice the 256 MB Infinity Cache
WINDOW_S = 0.2
CHILD_TIMEOUT = 300  # seconds per child


def _timing(torch, reps):
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

    def compare(hip_fns, torch_fns):
        g_hip, g_torch = graph_of(hip_fns), graph_of(torch_fns)
        k_hip = max(1, int(WINDOW_S * 1e6 / (window(g_hip, 1) * reps)) + 1)
        k_torch = max(1, int(WINDOW_S * 1e6 / (window(g_torch, 1) * reps)) + 1)
        t_hip, t_torch = [], []
        for _ in range(5):  # alternate the two forms: a drift of the machine hits both
            t_hip.append(window(g_hip, k_hip))
            t_torch.append(window(g_torch, k_torch))
        return t_hip, t_torch, reps * k_hip

    return compare


def _row(nbytes, nsets, calls, t_hip, t_torch, **head):
    hip, tor = sorted(t_hip)[2], sorted(t_torch)[2]
    return dict(**head, buffer_sets=nsets, working_set_MB=round(nsets * nbytes / 1e6), calls_per_window=calls, hip_us=round(hip, 1),
                hip_us_min=round(min(t_hip), 1), hip_us_max=round(max(t_hip), 1), alg_MB=round(nbytes / 1e6, 1), hbm_floor_us=round(nbytes / HBM * 1e6, 1),
                achieved_TBps=round(nbytes / hip / 1e6, 2), share_of_hbm_roof=round(nbytes / HBM * 1e6 / hip, 3), torch_us=round(tor, 1),
                torch_us_min=round(min(t_torch), 1), torch_us_max=round(max(t_torch), 1), torch_over_hip=round(tor / hip, 2))


def _setup():
    import torch
    sys.path.insert(0, ROOT)
    import edge_yolo_amd  # noqa: F401
    from edge_yolo_amd import _lib as L
    from edge_yolo_amd.nn import _ops as ops
    return torch, L, ops


def one_adown(C, H, W, reps):
    torch, L, ops = _setup()
    import torch.nn.functional as F
    c = C // 2

    def torch_form(x):
        a = F.avg_pool2d(x, 2, 1, 0, False, True)
        x1, x2 = a.chunk(2, 1)
        return x1, F.max_pool2d(x2, 3, 2, 1)

    with torch.no_grad():
        torch.manual_seed(0)
        nbytes = 2 * B * (H * W * C + (H - 1) * (W - 1) * c + (H // 2) * (W // 2) * c)
        nsets = max(2, -(-WORKING_SET // nbytes))
        xs = [torch.randn(B, H, W, C, device="cuda", dtype=torch.float16).permute(0, 3, 1, 2) for _ in range(nsets)]
        av = [L.empty_nhwc(B, c, H - 1, W - 1, torch.float16, "cuda") for _ in range(nsets)]
        mv = [L.empty_nhwc(B, c, H // 2, W // 2, torch.float16, "cuda") for _ in range(nsets)]
        xc = [t.contiguous() for t in xs]  # the composition's layout (NCHW), converted outside the timed region
        t_hip, t_torch, calls = _timing(torch, reps)([lambda x=x, a=a, m=m: ops.adown_pool(x, c, a=a, m=m) for x, a, m in zip(xs, av, mv)],
                                                     [lambda x=x: torch_form(x) for x in xc])
        ops.adown_pool(xs[0], c, a=av[0], m=mv[0])
        ta, tm = torch_form(xc[0])
        same = bool(torch.equal(av[0], ta) and torch.equal(mv[0], tm))
        return _row(nbytes, nsets, calls, t_hip, t_torch, what="adown_pool", B=B, C=C, c_avg=c, H=H, W=W, bits_equal_torch=same)


def one_cbfuse(level, reps):
    torch, L, ops = _setup()
    import torch.nn.functional as F
    C, side = 64 << level, CBL_SIDE[level]
    off = 64 * ((1 << level) - 1)

    def torch_form(srcs):
        res = [F.interpolate(s, size=(side, side), mode="nearest") for s in srcs[:-1]]
        return torch.sum(torch.stack(res + srcs[-1:]), dim=0)

    with torch.no_grad():
        torch.manual_seed(0)
        n = len(CBL_SIDE) - level + 1
        nbytes = 2 * B * C * (sum(s * s for s in CBL_SIDE[level:]) + 2 * side * side)
        nsets = max(2, -(-WORKING_SET // nbytes))
        sets, csets, outs = [], [], []
        for _ in range(nsets):
            srcs = [torch.randn(B, s, s, w, device="cuda", dtype=torch.float16).permute(0, 3, 1, 2)[:, off:off + C] for s, w in zip(CBL_SIDE[level:], CBL_WIDTH[level:])]
            srcs.append(torch.randn(B, side, side, C, device="cuda", dtype=torch.float16).permute(0, 3, 1, 2))
            sets.append(srcs)
            csets.append([t.contiguous() for t in srcs])
            outs.append(L.empty_nhwc(B, C, side, side, torch.float16, "cuda"))
        t_hip, t_torch, calls = _timing(torch, reps)([lambda s=s, o=o: ops.cbfuse(s, out=o) for s, o in zip(sets, outs)], [lambda s=s: torch_form(s) for s in csets])
        ops.cbfuse(sets[0], out=outs[0])
        err = float((outs[0].float() - torch_form(csets[0]).float()).abs().max())
        return _row(nbytes, nsets, calls, t_hip, t_torch, what="cbfuse", layer=16 + 2 * level if level < 2 else 15 + 3 * level, B=B, C=C, H=side, W=side, n=n,
                    max_abs_diff_vs_torch_f16=err)


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
                adown_launches=agg.get("adown_kernel", 0), detections=sum(len(r) for r in res))


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
    if argv and argv[0] == "--adown":
        print(json.dumps(one_adown(*(int(a) for a in argv[1:5]))), flush=True)
        sys.exit(0)
    if argv and argv[0] == "--cbfuse":
        print(json.dumps(one_cbfuse(int(argv[1]), int(argv[2]))), flush=True)
        sys.exit(0)
    if argv and argv[0] == "--model":
        print(json.dumps(one_model(argv[1])), flush=True)
        sys.exit(0)
    out = os.path.join(ROOT, "profiles", "gelan_bench.txt")
    if argv and argv[0] == "--out":
        out, argv = argv[1], argv[2:]
    reps = int(argv[0]) if argv else 48
    with open(out, "w") as f:
        def emit(line):
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
        emit(f"# tools/gelan_bench.py: ey_adown_pool and ey_cbfuse vs the torch compositions, batch {B}, f16, 640x640 input; median of 5 windows")
        for C, H, W in ADOWN:
            emit(f"# yolov9c ADown: C{C} {H}x{W}")
            emit(_child(["--adown", str(C), str(H), str(W), str(reps)], f"adown C{C} {H}x{W}"))
        for level in range(5):
            emit(f"# yolov9e CBFuse: C{64 << level} {CBL_SIDE[level]}x{CBL_SIDE[level]}, {6 - level} sources")
            emit(_child(["--cbfuse", str(level), str(reps)], f"cbfuse level {level}"))
        emit(f"# predict(): batch {B}, 640x640, f16, device tensors, captured graph; median of 5 windows of 20 calls; launches of one device step")
        for name in MODELS:
            emit(_child(["--model", name], name))
