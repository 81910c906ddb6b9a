"""Developer tool for the segment task.  Three measurements, each in a child process of its own under a time limit (the parent never opens
the GPU and stops at the first child that fails or runs out of time):

  mask   ey_process_mask against the eager torch composition of the same operations (per image, as the reference's predictor does:
         matmul, crop, F.interpolate(bilinear), gt) on the same GPU: 640^2 input, proto 160x160x32 f16, batch 32, K boxes per image.
         Both forms are replayed from a hipGraph; timed windows alternate between them (five each, median reported).  Bytes = what the
         kernel must move: the N output masks once + proto once + rows / boxes / coefficients; share of the 8 TB/s HBM peak on those.
  deconv ey_deconv2x2 at the Proto width of a scale (n: 64, l: 256; 80x80 input, batch 32, f16) against F.conv_transpose2d in NCHW and
         in channels_last layout (the faster one is the yardstick).
  trace  one eager predict step of yolo11n-seg at batch 32, 640^2, f16 (synthetic weights): launches, share of the new kernels,
         and images/s of predict() with the captured graph.

usage: process_mask_bench.py                 (everything: mask 20, mask 300, deconv n, deconv l, trace)
       process_mask_bench.py --mask K | --deconv C | --trace     (one measurement, what the children run)"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, IMG, MH, NM = 32, 640, 160, 32
HBM = 8.0e12
CHILD_TIMEOUT = 300


def _setup():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    import edge_yolo_amd  # noqa: F401
    return torch


def _timers(torch):
    def graph_of(fn, warm=2):
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            fn()
        g.replay()
        torch.cuda.synchronize()
        return g

    def window(g, k):
        st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        st.record()
        for _ in range(k):
            g.replay()
        en.record()
        torch.cuda.synchronize()
        return st.elapsed_time(en) * 1000 / k  # us per replay

    def ab(g_a, g_b, target_s=0.25):
        ka = max(1, int(target_s * 1e6 / window(g_a, 1)))
        kb = max(1, int(target_s * 1e6 / window(g_b, 1)))
        ta, tb = [], []
        for _ in range(5):  # alternate: a drift of the machine hits both
            ta.append(window(g_a, ka))
            tb.append(window(g_b, kb))
        return sorted(ta), sorted(tb)

    return graph_of, window, ab


def mask(K):
    torch = _setup()
    import torch.nn.functional as F
    from edge_yolo_amd.nn import _ops as ops
    graph_of, window, ab = _timers(torch)
    torch.manual_seed(0)
    N = B * K
    proto = torch.randn(B, MH, MH, NM, device="cuda", dtype=torch.float16).permute(0, 3, 1, 2)
    coef = torch.randn(B, K, 1, NM, device="cuda", dtype=torch.float16).permute(0, 3, 1, 2)  # one level, K "anchors" per image
    rows = torch.stack([torch.arange(N, dtype=torch.int32) // K, torch.arange(N, dtype=torch.int32) % K], 1).cuda().contiguous()
    # boxes as a detector gives them: centres uniform, sides log-normal around 64 px (synthdata.synth_pred's rule)
    c = torch.rand(N, 2) * IMG
    wh = torch.exp(torch.randn(N, 2) * 0.6 + 4.16)
    boxes = torch.cat([c - wh / 2, c + wh / 2], 1).float().cuda().contiguous()
    out = torch.empty(N, IMG, IMG, dtype=torch.uint8, device="cuda")

    def hip():
        ops.process_mask(proto, [coef], rows, boxes, IMG // MH, out=out)

    pc = proto.contiguous().view(B, NM, -1)  # NCHW protos, the composition's own layout
    cf = coef.permute(0, 2, 3, 1).reshape(N, NM).float()

    def crop(m, b):
        x1, y1, x2, y2 = torch.chunk(b[:, :, None], 4, 1)
        r = torch.arange(m.shape[2], device=m.device, dtype=x1.dtype)[None, None, :]
        cc = torch.arange(m.shape[1], device=m.device, dtype=x1.dtype)[None, :, None]
        return m * ((r >= x1) * (r < x2) * (cc >= y1) * (cc < y2))

    res = [None] * B

    def eager():
        for i in range(B):
            m = (cf[i * K:(i + 1) * K] @ pc[i].float()).view(-1, MH, MH)
            m = crop(m, boxes[i * K:(i + 1) * K] * (MH / IMG))
            res[i] = F.interpolate(m[None], (IMG, IMG), mode="bilinear", align_corners=False)[0].gt_(0.0)

    g_hip, g_t = graph_of(hip), graph_of(eager)
    th, tt = ab(g_hip, g_t)
    hip()
    eager()
    torch.cuda.synchronize()
    diff = sum(int((res[i].to(torch.uint8) != out[i * K:(i + 1) * K]).sum()) for i in range(B))
    nbytes = out.numel() + proto.numel() * 2 + N * (NM * 2 + 24)
    print(json.dumps(dict(what="process_mask", boxes_per_image=K, N=N, hip_us=round(th[2], 1), hip_us_min=round(th[0], 1), hip_us_max=round(th[4], 1),
                          torch_us=round(tt[2], 1), torch_us_min=round(tt[0], 1), torch_us_max=round(tt[4], 1), torch_over_hip=round(tt[2] / th[2], 2),
                          alg_MB=round(nbytes / 1e6, 1), achieved_TBps=round(nbytes / th[2] / 1e6, 3), share_of_hbm_peak=round(nbytes / HBM * 1e6 / th[2], 3),
                          pixels_differing_from_torch=diff, pixels=int(out.numel()))), flush=True)


def deconv(C):
    torch = _setup()
    import torch.nn as nn
    import torch.nn.functional as F
    from edge_yolo_amd import _lib as L
    from edge_yolo_amd.nn import _ops as ops
    from edge_yolo_amd.nn.modules import Proto
    graph_of, window, ab = _timers(torch)
    torch.manual_seed(0)
    torch.set_grad_enabled(False)
    H = IMG // 8
    m = Proto(C, C, NM).to("cuda").half().eval()
    x = torch.randn(B, H, H, C, device="cuda", dtype=torch.float16).permute(0, 3, 1, 2)
    y = L.empty_nhwc(B, C, 2 * H, 2 * H, torch.float16, "cuda")
    up = m.upsample
    xc, xl = x.contiguous(), x.contiguous(memory_format=torch.channels_last)
    g_hip = graph_of(lambda: ops.deconv2x2(m, x, up, out=y))
    g_nchw = graph_of(lambda: F.conv_transpose2d(xc, up.weight, up.bias, stride=2))
    g_cl = graph_of(lambda: F.conv_transpose2d(xl, up.weight, up.bias, stride=2))
    th, tn = ab(g_hip, g_nchw)
    _, tc = ab(g_hip, g_cl)
    err = float((y.float() - F.conv_transpose2d(xc, up.weight, up.bias, stride=2).float()).abs().max())
    nbytes = 5 * B * H * H * C * 2 + 4 * C * C * 2
    flops = 8.0 * B * H * H * C * C
    best = min(tn[2], tc[2])
    print(json.dumps(dict(what="deconv2x2", C=C, H=H, W=H, B=B, hip_us=round(th[2], 1), hip_us_min=round(th[0], 1), hip_us_max=round(th[4], 1),
                          torch_nchw_us=round(tn[2], 1), torch_channels_last_us=round(tc[2], 1), torch_over_hip=round(best / th[2], 2),
                          alg_MB=round(nbytes / 1e6, 1), share_of_hbm_peak=round(nbytes / HBM * 1e6 / th[2], 3), TFLOPs=round(flops / th[2] / 1e6, 1),
                          max_abs_diff_vs_torch_f16=err)), flush=True)


def trace():
    torch = _setup()
    import time
    import edge_yolo_amd
    from edge_yolo_amd import profiling
    import seg_synth
    import synthdata as synth
    model = edge_yolo_amd.YOLO("yolo11n-seg.yaml")
    model.model.load_state_dict(seg_synth.state_dict(model.model.state_dict()))
    x = synth.synth_images(B, IMG, IMG).cuda().half()
    kw = dict(conf=0.25, iou=0.7, half=True, device="cuda:0")
    res = model.predict(x, graph=False, **kw)
    with profiling.trace() as t:
        model.predict(x, graph=False, **kw)
    agg = t.summary()
    total = sum(a["ms"] for a in agg.values())
    new = {k: dict(launches=a["launches"], ms=round(a["ms"], 4), share=round(a["ms"] / total, 4)) for k, a in agg.items() if k in ("process_mask_kernel", "deconv2x2_kernel")}
    for _ in range(3):
        model.predict(x, graph=True, **kw)
    torch.cuda.synchronize()
    t0, n = time.perf_counter(), 20
    for _ in range(n):
        model.predict(x, graph=True, **kw)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / n
    print(json.dumps(dict(what="predict yolo11n-seg", batch=B, imgsz=IMG, half=True, kept_boxes=sum(len(r) for r in res),
                          launches=sum(a["kernels"] for a in agg.values()), traced_device_ms=round(total, 3), new_kernels=new,
                          ms_per_batch=round(dt * 1e3, 3), images_per_s=round(B / dt, 1))), flush=True)


if __name__ == "__main__":
    a = sys.argv[1:]
    if a and a[0] == "--mask":
        mask(int(a[1]))
    elif a and a[0] == "--deconv":
        deconv(int(a[1]))
    elif a and a[0] == "--trace":
        trace()
    else:
        for args in (["--mask", "20"], ["--mask", "300"], ["--deconv", "64"], ["--deconv", "256"], ["--trace"]):
            print("# " + " ".join(args), flush=True)
            try:
                rc = subprocess.run([sys.executable, os.path.abspath(__file__), *args], timeout=CHILD_TIMEOUT).returncode
            except subprocess.TimeoutExpired:
                sys.exit(f"{args}: no result within {CHILD_TIMEOUT} s; stopping")
            if rc != 0:
                sys.exit(f"{args}: exit status {rc}; stopping")
