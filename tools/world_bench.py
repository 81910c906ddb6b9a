"""Developer tool: time ey_max_sigmoid_attn (the gate of YOLO-World's C2fAttn, one launch) at the twelve C2fAttn shapes of
yolov8n/s/l-worldv2 at 640^2, batch 32, f16, 80 texts, against the PyTorch composition of the same expression on the same device and f16 data
(einsum, max, division, bias, sigmoid, scale, multiply; NCHW, its own best layout), a yardstick only; and YOLOWorld("yolov8n-worldv2")
.predict() next to YOLO("yolo11n").predict() in images/s (batch 32, 640^2, f16, device tensors, captured graph), in the same run.

Both kernel forms are replayed from a hipGraph that walks a rotation of buffers larger than the Infinity Cache; the timed windows are about
0.2 s each and alternate between the two forms (five each, the median is reported, min and max next to it).  One JSON line per shape with the
time per call against the algorithmic bytes of the call (e and p read once, y written once: 3 B H W C 2 bytes) and the MI355X's 8 TB/s HBM.
The lines are printed and written to profiles/world_bench.txt (or --out PATH).

Every shape and every model runs in a child process of its own under a time limit; the parent never opens the GPU and stops at the first
child that fails or runs out of time.
usage: world_bench.py [--out PATH] [reps]       (all shapes, both models)
       world_bench.py --shape C H W reps        (one shape, what the children run)
       world_bench.py --model NAME              (one model)"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, TEXTS = 32, 80
# (model, C2fAttn layer, C = hidden width, H, W) at 640x640: layers 12 and 18 work on P4, 15 on P3, 21 on P5
SHAPES = [("yolov8n-worldv2", 12, 64, 40, 40), ("yolov8n-worldv2", 15, 32, 80, 80), ("yolov8n-worldv2", 18, 64, 40, 40), ("yolov8n-worldv2", 21, 128, 20, 20),
          ("yolov8s-worldv2", 12, 128, 40, 40), ("yolov8s-worldv2", 15, 64, 80, 80), ("yolov8s-worldv2", 18, 128, 40, 40), ("yolov8s-worldv2", 21, 256, 20, 20),
          ("yolov8l-worldv2", 12, 256, 40, 40), ("yolov8l-worldv2", 15, 128, 80, 80), ("yolov8l-worldv2", 18, 256, 40, 40), ("yolov8l-worldv2", 21, 256, 20, 20)]
MODELS = ["yolov8n-worldv2.yaml", "yolo11n.yaml"]
HBM = 8.0e12
WORKING_SET = 600 << 20  # bytes the rotated buffers cover: more than twice the 256 MB Infinity Cache
WINDOW_S = 0.2
CHILD_TIMEOUT = 240  # seconds per child


def torch_form(e, p, g, bias, scale, nh):
    """The reference's expression (block.py:563-576) with torch operators on NCHW f16 data; g (1, n, C)."""
    import torch
    Bn, C, H, W = e.shape
    hc = C // nh
    aw = torch.einsum("bmchw,bnmc->bmhwn", e.view(Bn, nh, hc, H, W), g.expand(Bn, -1, -1).view(Bn, -1, nh, hc))
    aw = aw.max(dim=-1)[0] / (hc ** 0.5) + bias[None, :, None, None]
    aw = aw.sigmoid() * scale
    return (p.view(Bn, nh, -1, H, W) * aw.unsqueeze(2)).view(Bn, -1, H, W)


def one_shape(C, H, W, reps):
    import torch
    sys.path.insert(0, ROOT)
    import edge_yolo_amd  # noqa: F401
    from edge_yolo_amd import _lib as L
    from edge_yolo_amd.nn import _ops as ops

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

    with torch.no_grad():
        torch.manual_seed(0)
        nh = C // 32
        nbytes = 3 * B * H * W * C * 2
        nsets = max(2, -(-WORKING_SET // nbytes))
        mk = lambda: torch.randn(B, H, W, C, device="cuda", dtype=torch.float16).permute(0, 3, 1, 2)  # noqa: E731
        es, ps = [mk() for _ in range(nsets)], [mk() for _ in range(nsets)]
        outs = [L.empty_nhwc(B, C, H, W, torch.float16, "cuda") for _ in range(nsets)]
        ecs, pcs = [t.contiguous() for t in es], [t.contiguous() for t in ps]  # the composition's layout (NCHW), converted outside the timed region
        g = torch.randn(1, TEXTS, C, device="cuda", dtype=torch.float16)
        bias = torch.randn(nh, device="cuda") * 0.5
        scale = torch.ones(1, nh, 1, 1, device="cuda", dtype=torch.float16)
        bias_h = bias.half()
        g_hip = graph_of([lambda e=e, p=p, o=o: ops.max_sigmoid_attn(e, p, g, bias, None, nh, out=o) for e, p, o in zip(es, ps, outs)])
        g_torch = graph_of([lambda e=e, p=p: torch_form(e, p, g, bias_h, scale, nh) for e, p in zip(ecs, pcs)])
        k_hip = max(1, int(WINDOW_S * 1e6 / (window(g_hip, 1) * reps)) + 1)
        k_torch = max(1, int(WINDOW_S * 1e6 / (window(g_torch, 1) * reps)) + 1)
        t_hip, t_torch = [], []
        for _ in range(5):  # alternate the two forms: a drift of the machine hits both
            t_hip.append(window(g_hip, k_hip))
            t_torch.append(window(g_torch, k_torch))
        hip, tor = sorted(t_hip)[2], sorted(t_torch)[2]
        ops.max_sigmoid_attn(es[0], ps[0], g, bias, None, nh, out=outs[0])
        err = float((outs[0].float() - torch_form(ecs[0], pcs[0], g, bias_h, scale, nh).float()).abs().max())
        return dict(B=B, C=C, H=H, W=W, heads=nh, texts=TEXTS, buffer_sets=nsets, working_set_MB=round(nsets * nbytes / 1e6), calls_per_window=reps * k_hip,
                    hip_us=round(hip, 1), hip_us_min=round(min(t_hip), 1), hip_us_max=round(max(t_hip), 1), alg_MB=round(nbytes / 1e6, 1),
                    hbm_floor_us=round(nbytes / HBM * 1e6, 1), achieved_TBps=round(nbytes / hip / 1e6, 2), share_of_hbm_roof=round(nbytes / HBM * 1e6 / hip, 3),
                    torch_us=round(tor, 1), torch_us_min=round(min(t_torch), 1), torch_us_max=round(max(t_torch), 1), torch_over_hip=round(tor / hip, 2),
                    max_abs_diff_vs_torch_f16=err)


def one_model(name, warmup=5, calls=20, windows=5):
    import time

    import torch
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import edge_yolo_amd
    import synthdata as synth
    import world_synth as ws
    world = "world" in name
    model = (edge_yolo_amd.YOLOWorld if world else edge_yolo_amd.YOLO)(name)
    own = model.model.state_dict()
    model.model.load_state_dict(ws.state_dict(own) if world else synth.synth_state_dict({k: tuple(v.shape) for k, v in own.items()}), strict=False)
    if world:
        model.set_classes(ws.names(TEXTS), ws.text("bench", TEXTS))
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
    return dict(model=name, batch=B, imgsz=640, half=True, texts=TEXTS if world else None, calls_per_window=calls, windows=windows,
                ms_per_batch=round(med * 1e3, 3), ms_min=round(min(ts) * 1e3, 3), ms_max=round(max(ts) * 1e3, 3), images_per_s=round(B / med, 1),
                detections=sum(len(r) for r in res))


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
    if argv and argv[0] == "--shape":
        print(json.dumps(one_shape(*(int(a) for a in argv[1:5]))), flush=True)
        sys.exit(0)
    if argv and argv[0] == "--model":
        print(json.dumps(one_model(argv[1])), flush=True)
        sys.exit(0)
    out = os.path.join(ROOT, "profiles", "world_bench.txt")
    if argv and argv[0] == "--out":
        out, argv = argv[1], argv[2:]
    reps = int(argv[0]) if argv else 240
    with open(out, "w") as f:
        def emit(line):
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
        emit(f"# tools/world_bench.py: ey_max_sigmoid_attn vs the torch composition, batch {B}, f16, {TEXTS} texts, 640x640 input; median of 5 windows")
        for model, layer, C, H, W in SHAPES:
            emit(f"# {model} layer {layer}: C{C} {H}x{W}")
            emit(_child(["--shape", str(C), str(H), str(W), str(reps)], f"C{C} {H}x{W}"))
        emit(f"# predict(): batch {B}, 640x640, f16, device tensors, captured graph; median of 5 windows of 20 calls")
        for name in MODELS:
            emit(_child(["--model", name], name))
