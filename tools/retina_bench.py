"""Developer tool for masks at the original resolution (retina_masks=True): ey_process_mask_native against the composition the library could
already run on the GPU for the same result -- torch.matmul (coefficients x prototypes, fp32), _ops.scale_masks (ey_scale_masks, fp32, to the
original shape), then torch's crop_mask and compare -- one image, proto 160x160x32 f16, N kept boxes, for every original size and N below.

One child process per original size, each under a time limit (the parent never opens the GPU and stops at the first child that fails or
runs out of time).  Both forms are replayed from a hipGraph; timed windows alternate between them (five each, median reported, min and max
beside it).  Bytes = the N H0 W0 result bytes, which is what the fused kernel must write; achieved write bandwidth is those over its time, and
its share of the 8 TB/s HBM peak.  The composition also writes the (N, H0, W0) fp32 resized map, reads it and writes the cropped copy, reads
that and writes the bits: at least 17 bytes per result byte.

usage: retina_bench.py [--out FILE]            (everything; the lines also go to FILE, default profiles/retina_bench.txt)
       retina_bench.py --size H0 W0            (one original size, what the children run)"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MH, NM = 160, 32
SIZES = [(480, 640), (1080, 1920), (2160, 3840)]
COUNTS = [1, 17, 100, 300]
HBM = 8.0e12
CHILD_TIMEOUT = 420


def _setup():
    sys.path.insert(0, ROOT)
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

    return graph_of, ab


def size(h0, w0):
    torch = _setup()
    from edge_yolo_amd.nn import _ops as ops
    graph_of, ab = _timers(torch)
    torch.manual_seed(0)
    proto = torch.randn(1, MH, MH, NM, device="cuda", dtype=torch.float16).permute(0, 3, 1, 2)
    pc = proto.contiguous().view(NM, -1).float()  # CHW prototypes in fp32, the composition's own operand (converted once, outside the timing)
    for N in COUNTS:
        coef = torch.randn(1, N, 1, NM, device="cuda", dtype=torch.float16).permute(0, 3, 1, 2)  # one level, N "anchors"
        rows = torch.stack([torch.zeros(N, dtype=torch.int32), torch.arange(N, dtype=torch.int32)], 1).cuda().contiguous()
        # boxes as a detector gives them, in original-image pixels: centres uniform, sides log-normal around 15 % of the shorter side
        c = torch.rand(N, 2) * torch.tensor([w0, h0])
        wh = torch.exp(torch.randn(N, 2) * 0.6) * 0.15 * min(h0, w0)
        boxes = torch.cat([c - wh / 2, c + wh / 2], 1).float().cuda().contiguous()
        out = torch.empty(N * h0 * w0, dtype=torch.uint8, device="cuda")
        cf = coef.permute(0, 2, 3, 1).reshape(N, NM).float()
        x1, y1, x2, y2 = torch.chunk(boxes[:, :, None], 4, 1)
        r = torch.arange(w0, device="cuda", dtype=torch.float32)[None, None, :]
        cc = torch.arange(h0, device="cuda", dtype=torch.float32)[None, :, None]
        res = [None]

        def hip():
            ops.process_mask_native(proto, [coef], rows, boxes, [0, N], [(h0, w0)], out=out)

        def composed():
            m = torch.matmul(cf, pc).view(1, N, MH, MH)
            m = ops.scale_masks(m, (h0, w0))[0]
            res[0] = (m * ((r >= x1) * (r < x2) * (cc >= y1) * (cc < y2))).gt_(0.0)

        g_hip, g_c = graph_of(hip), graph_of(composed)
        th, tc = ab(g_hip, g_c)
        g_hip.replay()
        g_c.replay()
        torch.cuda.synchronize()
        diff = int((res[0].to(torch.uint8) != out.view(N, h0, w0)).sum())
        nbytes = N * h0 * w0
        print(json.dumps(dict(what="process_mask_native", H0=h0, W0=w0, N=N, hip_us=round(th[2], 1), hip_us_min=round(th[0], 1), hip_us_max=round(th[4], 1),
                              composed_us=round(tc[2], 1), composed_us_min=round(tc[0], 1), composed_us_max=round(tc[4], 1), composed_over_hip=round(tc[2] / th[2], 2),
                              result_MB=round(nbytes / 1e6, 1), write_TBps=round(nbytes / th[2] / 1e6, 3), share_of_hbm_peak=round(nbytes / HBM * 1e6 / th[2], 3),
                              set_pixels=int(out.sum(dtype=torch.int64)), pixels_differing_from_composition=diff, pixels=nbytes)), flush=True)
        del g_hip, g_c, res, out
        torch.cuda.empty_cache()


if __name__ == "__main__":
    a = sys.argv[1:]
    if a and a[0] == "--size":
        size(int(a[1]), int(a[2]))
    else:
        path = a[1] if a and a[0] == "--out" else os.path.join(ROOT, "profiles", "retina_bench.txt")
        lines = []
        for h0, w0 in SIZES:
            try:
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--size", str(h0), str(w0)], timeout=CHILD_TIMEOUT, stdout=subprocess.PIPE, text=True)
            except subprocess.TimeoutExpired:
                sys.exit(f"{h0}x{w0}: no result within {CHILD_TIMEOUT} s; stopping")
            sys.stdout.write(p.stdout)
            sys.stdout.flush()
            lines.append(p.stdout)
            if p.returncode != 0:
                sys.exit(f"{h0}x{w0}: exit status {p.returncode}; stopping")
        with open(path, "w") as f:
            f.write(f"# tools/retina_bench.py: ey_process_mask_native vs torch.matmul -> ey_scale_masks (fp32) -> torch crop + compare; proto {MH}x{MH}x{NM} f16, one image\n")
            f.write("".join(lines))
