"""Developer tool: time the kernels of the classic families (YOLOv3, YOLOv5, YOLOv6) at batch 32, 640^2, f16.

* ey_stem_conv_ks at the layer-0 shapes of yolov5 n / s / x (6x6 stride 2 pad 2, 3 -> 16 / 32 / 80) and of yolov3 / yolov3-tiny (3x3 stride 1,
  3 -> 32 / 16), against the path such a layer took before the kernel existed: the NCHW -> NHWC copy of the image (ey_nchw_to_nhwc) followed by
  the scalar ey_conv2d_direct -- the yardstick, timed in the same run.
* ey_maxpool2d at the six pooling shapes of yolov3-tiny (the last one with the zero padding in the same launch) against
  torch.nn.functional.max_pool2d on the same channels-last tensors (plus F.pad for the last one).
* YOLO(...).predict() of yolov5n, yolov5s, yolov3-tiny and yolov6n next to yolo11n in images/s (device tensors, captured graph) with the launches
  of one device step, in the same run.

Both forms of a kernel comparison are replayed from a hipGraph that walks a rotation of buffers larger than the Infinity Cache; the timed windows
are about 0.2 s each and alternate between the two forms (five each, the median is reported, min and max next to it).  One JSON line per shape
with the time per call against the algorithmic bytes (every input read once, every output written once) and the MI355X's 8 TB/s HBM.  The lines
are printed and written to profiles/classic_bench.txt (or --out PATH).

Every shape and every model runs in a child process of its own under a time limit; the parent never opens the GPU and stops at the first child
that fails or runs out of time.
usage: classic_bench.py [--out PATH] [reps]          (all shapes, all models)
       classic_bench.py --stem K S P COUT reps       (one stem shape, what the children run)
       classic_bench.py --pool C HW S PAD reps       (one pooling shape)
       classic_bench.py --model NAME"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ghost_bench import B, HBM, WORKING_SET, _compare, one_model  # noqa: E402  (the same timing scheme and the same predict() measurement)

STEMS = [("yolov5n", 6, 2, 2, 16), ("yolov5s", 6, 2, 2, 32), ("yolov5x", 6, 2, 2, 80), ("yolov3", 3, 1, 1, 32), ("yolov3-tiny", 3, 1, 1, 16)]
POOLS = [(16, 640, 2, 0), (32, 320, 2, 0), (64, 160, 2, 0), (128, 80, 2, 0), (256, 40, 2, 0), (512, 20, 1, 1)]  # (C, H = W, stride, zero pad right / bottom)
MODELS = ["yolov5n.yaml", "yolov5s.yaml", "yolov3-tiny.yaml", "yolov6n.yaml", "yolo11n.yaml"]
CHILD_TIMEOUT = 300  # seconds per child
IMG = 640


def _stats(prefix, ts, nbytes):
    med = sorted(ts)[len(ts) // 2]
    return {f"{prefix}_us": round(med, 1), f"{prefix}_us_min": round(min(ts), 1), f"{prefix}_us_max": round(max(ts), 1),
            f"{prefix}_share_of_hbm_roof": round(nbytes / HBM * 1e6 / med, 3)}


def one_stem(k, s, p, cout, reps):
    import torch
    sys.path.insert(0, ROOT)
    import edge_yolo_amd  # noqa: F401
    import synthdata as synth
    from edge_yolo_amd import _lib as L
    from edge_yolo_amd.nn import _ops as ops
    from edge_yolo_amd.nn.modules import Conv
    with torch.no_grad():
        m = Conv(3, cout, k, s, p)
        m.load_state_dict({kk: synth.synth_tensor("model.0." + kk, tuple(v.shape)) for kk, v in m.state_dict().items()})  # (keyed as layer 0 of a model)
        m = m.cuda().half().eval()
        act = L.ACT_SILU
        Ho = (IMG + 2 * p - k) // s + 1
        nbytes = 2 * B * (3 * IMG * IMG + cout * Ho * Ho)
        nsets = max(2, -(-WORKING_SET // nbytes))
        xs = [torch.rand(B, 3, IMG, IMG, device="cuda", dtype=torch.float16) for _ in range(nsets)]
        ys = [L.empty_nhwc(B, cout, Ho, Ho, torch.float16, "cuda") for _ in range(nsets)]
        y2 = L.empty_nhwc(B, cout, Ho, Ho, torch.float16, "cuda")

        def new(x, y):
            ops.stem_conv_ks(m, x, m.folded, k, s, p, act, x.dtype, out=y)

        def old(x, y):  # what Conv.forward did with this layer before: layout copy, then the scalar direct kernel
            ops.conv2d_direct(m, L.as_nhwc(x), m.folded, k, s, p, 1, act, out=y)

        t_n, t_o, calls = _compare(torch, reps, [lambda x=x, y=y: new(x, y) for x, y in zip(xs, ys)], [lambda x=x, y=y: old(x, y) for x, y in zip(xs, ys)])
        new(xs[0], ys[0])
        old(xs[0], y2)
        diff = float((ys[0].float() - y2.float()).abs().max())  # (the direct kernel keeps fp32 weights, the MFMA form rounds them to f16)
        r = dict(what="stem_conv_ks", B=B, k=k, s=s, p=p, Cout=cout, H=IMG, W=IMG, buffer_sets=nsets, calls_per_window=calls, alg_MB=round(nbytes / 1e6, 1),
                 alg_MB_per_image=round(nbytes / B / 1e6, 2), hbm_floor_us=round(nbytes / HBM * 1e6, 1))
        r.update(_stats("stem", t_n, nbytes))
        r.update(_stats("copy_plus_direct", t_o, nbytes + 2 * 2 * B * 3 * IMG * IMG))
        r["direct_over_stem"] = round(r["copy_plus_direct_us"] / r["stem_us"], 2)
        r["max_abs_diff"] = round(diff, 5)
        return r


def one_pool(c, hw, s, pad, reps):
    import torch
    import torch.nn.functional as F
    sys.path.insert(0, ROOT)
    import edge_yolo_amd  # noqa: F401
    from edge_yolo_amd import _lib as L
    from edge_yolo_amd.nn import _ops as ops
    with torch.no_grad():
        pads = (0, pad, 0, pad)
        Ho = (hw + pad - 2) // s + 1
        nbytes = 2 * B * c * (hw * hw + Ho * Ho)
        nsets = max(2, -(-WORKING_SET // nbytes))
        xs = [torch.randn(B, hw, hw, c, device="cuda", dtype=torch.float16).permute(0, 3, 1, 2) for _ in range(nsets)]
        ys = [L.empty_nhwc(B, c, Ho, Ho, torch.float16, "cuda") for _ in range(nsets)]

        def new(x, y):
            ops.maxpool2d(x, 2, s, pads, out=y)

        def old(x, y):
            return F.max_pool2d(F.pad(x, pads) if pad else x, 2, s)

        t_n, t_o, calls = _compare(torch, reps, [lambda x=x, y=y: new(x, y) for x, y in zip(xs, ys)], [lambda x=x, y=y: old(x, y) for x, y in zip(xs, ys)])
        new(xs[0], ys[0])
        same = bool(torch.equal(ys[0], old(xs[0], None)))
        r = dict(what="maxpool2d", B=B, C=c, H=hw, W=hw, k=2, s=s, pad=list(pads), buffer_sets=nsets, calls_per_window=calls, alg_MB=round(nbytes / 1e6, 1),
                 hbm_floor_us=round(nbytes / HBM * 1e6, 1))
        r.update(_stats("maxpool", t_n, nbytes))
        r.update(_stats("torch", t_o, nbytes))
        r["torch_over_maxpool"] = round(r["torch_us"] / r["maxpool_us"], 2)
        r["bits_equal"] = same
        return r


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
    if argv and argv[0] == "--stem":
        print(json.dumps(one_stem(*(int(a) for a in argv[1:6]))), flush=True)
        sys.exit(0)
    if argv and argv[0] == "--pool":
        print(json.dumps(one_pool(*(int(a) for a in argv[1:6]))), flush=True)
        sys.exit(0)
    if argv and argv[0] == "--model":
        r = one_model(argv[1])
        r.pop("ghost_conv_launches", None)
        print(json.dumps(r), flush=True)
        sys.exit(0)
    out = os.path.join(ROOT, "profiles", "classic_bench.txt")
    if argv and argv[0] == "--out":
        out, argv = argv[1], argv[2:]
    reps = int(argv[0]) if argv else 16
    with open(out, "w") as f:
        def emit(line):
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
        emit(f"# tools/classic_bench.py: batch {B}, f16, 640x640 input; median of 5 alternating windows")
        emit("# ey_stem_conv_ks (planar image in, NHWC out) vs the NCHW -> NHWC copy + ey_conv2d_direct it replaces")
        for name, k, s, p, cout in STEMS:
            emit(f"# {name}: layer 0 = Conv(3, {cout}, {k}, {s}, {p})")
            emit(_child(["--stem", str(k), str(s), str(p), str(cout), str(reps)], f"stem {name}"))
        emit("# ey_maxpool2d at yolov3-tiny's six pooling shapes vs torch.nn.functional.max_pool2d (+ F.pad for the padded one) on channels-last tensors")
        for c, hw, s, pad in POOLS:
            emit(_child(["--pool", str(c), str(hw), str(s), str(pad), str(4 * reps)], f"maxpool C{c} {hw}x{hw}"))
        emit(f"# predict(): batch {B}, 640x640, f16, device tensors, captured graph; median of 5 windows of 20 calls; launches of one device step")
        for name in MODELS:
            emit(_child(["--model", name], name))
