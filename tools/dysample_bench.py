"""Developer tool: time ey_dysample (offsets + bilinear gather, one launch) at the DySample layer shapes of yolov13n-DySample and
yolov13l-DySample at 640^2, batch 32, f16, against the PyTorch composition of the same operation (F.conv2d, F.pixel_shuffle,
F.grid_sample on the same device and f16 data), a yardstick only.  Both forms are replayed from a hipGraph that walks a rotation of
buffers larger than the Infinity Cache; the timed windows are about 0.3 s each and alternate between the two forms (five each, the
median is reported).  Prints one JSON line per shape with the time per call against the algorithmic bytes of the call (x read once,
y written once: 5 B H W C 2 bytes) and the MI355X's 8 TB/s HBM.

Every shape runs in a child process of its own under a time limit; the parent never opens the GPU and stops at the first child that
fails or runs out of time.
usage: dysample_bench.py [reps]            (all shapes)
       dysample_bench.py --shape C H W reps  (one shape, what the children run)"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, GROUPS = 32, 4
# (model, layers, C, H, W): layer 10 and 19 read a P4 map (40x40 at 640^2), layer 15 the P5 map
SHAPES = [("yolov13n", "10, 19", 128, 40, 40), ("yolov13n", "15", 256, 20, 20), ("yolov13l", "10, 19", 512, 40, 40), ("yolov13l", "15", 512, 20, 20)]
HBM = 8.0e12
WORKING_SET = 600 << 20  # bytes the rotated buffers cover: more than twice the 256 MB Infinity Cache, so x comes from HBM and y goes there
WINDOW_S = 0.3  # each timed window replays the graph until about this long
CHILD_TIMEOUT = 240  # seconds per shape: torch import + 2 x (warm-up, capture) + 10 windows


def torch_form(x, w, b, pos, groups):
    """DySample 'lp' written with torch operators on NCHW f16 data: conv, normalised grid, pixel_shuffle, grid_sample."""
    import torch
    import torch.nn.functional as F
    Bn, C, H, W = x.shape
    off = (F.conv2d(x, w, b) * 0.25 + pos).view(Bn, 2, -1, H, W)
    gy, gx = torch.meshgrid(torch.arange(H, device=x.device, dtype=x.dtype) + 0.5, torch.arange(W, device=x.device, dtype=x.dtype) + 0.5, indexing="ij")
    base = torch.stack([gx, gy]).view(1, 2, 1, H, W)
    size = torch.cat([torch.full((1,), float(W), device=x.device, dtype=x.dtype), torch.full((1,), float(H), device=x.device, dtype=x.dtype)]).view(1, 2, 1, 1, 1)
    grid = 2 * (base + off) / size - 1
    grid = F.pixel_shuffle(grid.view(Bn, -1, H, W), 2).view(Bn, 2, groups, 2 * H, 2 * W).permute(0, 2, 3, 4, 1).reshape(Bn * groups, 2 * H, 2 * W, 2)
    y = F.grid_sample(x.reshape(Bn * groups, C // groups, H, W), grid, mode="bilinear", align_corners=False, padding_mode="border")
    return y.view(Bn, C, 2 * H, 2 * W)


def one_shape(C, H, W, reps):
    import torch
    sys.path.insert(0, ROOT)
    import edge_yolo_amd  # noqa: F401
    from edge_yolo_amd import _lib as L
    from edge_yolo_amd.nn import _ops as ops
    from edge_yolo_amd.nn.modules import DySample

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
        m = DySample(C, 2, "lp", GROUPS)
        m.offset.weight.data.normal_(0, 2.0 / C ** 0.5)  # offsets of about half a pixel rms: the gather really leaves its cell
        m = m.to("cuda").half().eval()
        nbytes = 5 * B * H * W * C * 2
        nsets = max(2, -(-WORKING_SET // nbytes))  # rotate over input / output pairs that together exceed the Infinity Cache twice over
        xs = [torch.randn(B, H, W, C, device="cuda", dtype=torch.float16).permute(0, 3, 1, 2) for _ in range(nsets)]
        outs = [L.empty_nhwc(B, C, 2 * H, 2 * W, torch.float16, "cuda") for _ in range(nsets)]
        xcs = [x.contiguous() for x in xs]  # the composition's own best layout (NCHW), converted outside the timed region
        g_hip = graph_of([lambda x=x, o=o: ops.dysample(m, x, out=o) for x, o in zip(xs, outs)])
        g_torch = graph_of([lambda x=x: torch_form(x, m.offset.weight, m.offset.bias, m.init_pos, GROUPS) for x in xcs])
        k_hip = max(1, int(WINDOW_S * 1e6 / (window(g_hip, 1) * reps)) + 1)
        k_torch = max(1, int(WINDOW_S * 1e6 / (window(g_torch, 1) * reps)) + 1)
        t_hip, t_torch = [], []
        for _ in range(5):  # alternate the two forms: a drift of the machine hits both
            t_hip.append(window(g_hip, k_hip))
            t_torch.append(window(g_torch, k_torch))
        hip, tor = sorted(t_hip)[2], sorted(t_torch)[2]
        ops.dysample(m, xs[0], out=outs[0])
        err = float((outs[0].float() - torch_form(xcs[0], m.offset.weight, m.offset.bias, m.init_pos, GROUPS).float()).abs().max())
        print(json.dumps(dict(B=B, C=C, H=H, W=W, groups=GROUPS, buffer_sets=nsets, working_set_MB=round(nsets * nbytes / 1e6), calls_per_window=reps * k_hip,
                              window_ms=round(hip * reps * k_hip / 1e3), hip_us=round(hip, 1), hip_us_min=round(min(t_hip), 1), hip_us_max=round(max(t_hip), 1),
                              alg_MB=round(nbytes / 1e6, 1), hbm_floor_us=round(nbytes / HBM * 1e6, 1), achieved_TBps=round(nbytes / hip / 1e6, 2),
                              share_of_hbm_roof=round(nbytes / HBM * 1e6 / hip, 3), torch_us=round(tor, 1), torch_us_min=round(min(t_torch), 1),
                              torch_us_max=round(max(t_torch), 1), torch_over_hip=round(tor / hip, 2), max_abs_diff_vs_torch_f16=err)), flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--shape":
        one_shape(*(int(a) for a in sys.argv[2:6]))
        sys.exit(0)
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 240
    for model, layers, C, H, W in SHAPES:
        print(f"# {model}-DySample layers {layers}: C{C} {H}x{W}", flush=True)
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--shape", str(C), str(H), str(W), str(reps)], timeout=CHILD_TIMEOUT).returncode
        except subprocess.TimeoutExpired:
            sys.exit(f"C{C} {H}x{W}: no result within {CHILD_TIMEOUT} s; stopping")
        if rc != 0:
            sys.exit(f"C{C} {H}x{W}: exit status {rc}; stopping")
