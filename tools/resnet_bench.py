"""Developer tool: time the kernels of the ResNet backbones (yolov8-cls-resnet50 / -resnet101) at batch 32, f16.

* Layer 0 (Conv 7x7 / 2 / 3 + SiLU, then MaxPool 3x3 / 2 / 1) at 224^2 and 640^2, three ways: ONE ey_resnet_stem launch (fused), ey_stem_conv_ks
  (7, 2, 3) followed by ey_maxpool3x3s2 (the pair), and PyTorch-ROCm's F.conv2d + F.silu + F.max_pool2d on channels_last f16 tensors, the outside
  yardstick (the pair is timed in both comparisons).  Bytes are algorithmic: the image in and the quarter-resolution map out; for the pair and
  torch also the half-resolution 64-channel map out and in again.
* The closing 1x1 of the 16 blocks of ResNet-50 at 224^2 (eight distinct shapes): ONE ey_resnet_tail launch (fused) against the composed form
  (the shortcut conv where the block has one, then cv3 on ey_conv2d with ReLU and the shortcut / the block input as its pre-activation
  term).  FLOPs are 2 M Cout K; the MFMA roof is 2.5 PFLOP/s dense f16.
* YOLO(...).predict() of yolov8n-cls-resnet50 next to yolo11n-cls at 224^2 in images/s with the launches of one device step (tools/cls_bench.py's
  measurement, run in the same call).

Both forms of a comparison are replayed from a hipGraph that walks a rotation of buffers larger than the Infinity Cache; the timed windows are
about 0.2 s each and alternate between the two forms (five each; median, min and max).  One JSON line per shape, printed and written to
profiles/resnet_bench.txt (or --out PATH).  Every shape and every model runs in a child process of its own under a time limit; the parent never
opens the GPU and stops at the first child that fails or runs out of time.
usage: resnet_bench.py [--out PATH] [reps]
       resnet_bench.py --stem IMG reps | --tail C1 C2 S HOUT reps      (what the children run; C1 = 0: identity block)"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ghost_bench import B, HBM, WORKING_SET, _compare  # noqa: E402  (the same timing scheme)

MFMA = 2.5e15
CHILD_TIMEOUT = 300
# (C1, C2, stride, output H = W at 224^2, blocks of this shape in ResNet-50): C1 = 0 is the identity block
TAILS = [(64, 64, 1, 56, 1), (0, 64, 1, 56, 2), (256, 128, 2, 28, 1), (0, 128, 1, 28, 3), (512, 256, 2, 14, 1), (0, 256, 1, 14, 5), (1024, 512, 2, 7, 1), (0, 512, 1, 7, 2)]


def _stats(prefix, ts, nbytes, flops=0.0):
    med = sorted(ts)[len(ts) // 2]
    d = {f"{prefix}_us": round(med, 1), f"{prefix}_us_min": round(min(ts), 1), f"{prefix}_us_max": round(max(ts), 1),
         f"{prefix}_share_of_hbm_roof": round(nbytes / HBM * 1e6 / med, 3)}
    if flops:
        d[f"{prefix}_share_of_mfma_roof"] = round(flops / MFMA * 1e6 / med, 3)
    return d


def _setup():
    import torch
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import edge_yolo_amd  # noqa: F401
    torch.set_grad_enabled(False)
    return torch


def one_stem(img, reps):
    torch = _setup()
    import torch.nn.functional as F
    import synthdata as synth
    from edge_yolo_amd.nn.modules import ResNetLayer
    m = ResNetLayer(3, 64, 1, True, 1)
    m.load_state_dict({k: synth.synth_tensor("model.0." + k, tuple(v.shape)) for k, v in m.state_dict().items()})
    m = m.cuda().half().eval()
    w, b = (t.cuda().half() for t in m.layer[0].folded())
    wcl = w.contiguous(memory_format=torch.channels_last)
    Hc, Hp = (img - 1) // 2 + 1, ((img - 1) // 2) // 2 + 1
    nbytes = 2 * B * (3 * img * img + 2 * 64 * Hc * Hc + 64 * Hp * Hp)
    flops = 2.0 * B * Hc * Hc * 64 * 147
    nsets = max(2, -(-WORKING_SET // nbytes))
    xs = [torch.rand(B, 3, img, img, device="cuda", dtype=torch.float16) for _ in range(nsets)]
    xcl = [x.contiguous(memory_format=torch.channels_last) for x in xs]

    def pair(x):
        m.stem_fused = False
        return m(x)

    def fused(x):
        m.stem_fused = True
        return m(x)

    def torch_cl(x):
        return F.max_pool2d(F.silu(F.conv2d(x, wcl, b, 2, 3)), 3, 2, 1)

    from edge_yolo_amd import profiling
    with profiling.trace() as tr:
        yf = fused(xs[0])
    assert [r[0] for r in tr.records] == ["resnet_stem_mfma_kernel"], [r[0] for r in tr.records]
    t_f, t_p, calls = _compare(torch, reps, [lambda x=x: fused(x) for x in xs], [lambda x=x: pair(x) for x in xs])
    t_p2, t_t, _ = _compare(torch, reps, [lambda x=x: pair(x) for x in xs], [lambda x=x: torch_cl(x) for x in xcl])
    diff = float((pair(xs[0]).float() - torch_cl(xcl[0]).float()).abs().max())
    fused_bytes = 2 * B * (3 * img * img + 64 * Hp * Hp)
    r = dict(what="resnet_layer0", B=B, H=img, W=img, buffer_sets=nsets, calls_per_window=calls, pair_alg_MB_per_image=round(nbytes / B / 1e6, 2),
             fused_alg_MB_per_image=round(fused_bytes / B / 1e6, 2), pair_hbm_floor_us=round(nbytes / HBM * 1e6, 1), fused_hbm_floor_us=round(fused_bytes / HBM * 1e6, 1))
    r.update(_stats("fused", t_f, fused_bytes, flops))
    r.update(_stats("stem_plus_pool", t_p, nbytes, flops))
    r.update(_stats("stem_plus_pool_again", t_p2, nbytes, flops))
    r.update(_stats("torch_channels_last", t_t, nbytes, flops))
    r.update(fused_launches=1, pair_launches=2, pair_over_fused=round(r["stem_plus_pool_us"] / r["fused_us"], 2),
             torch_over_pair=round(r["torch_channels_last_us"] / r["stem_plus_pool_again_us"], 2), fused_equals_pair=bool(torch.equal(yf, pair(xs[0]))), max_abs_diff_to_torch=round(diff, 4))
    return r


def one_tail(C1, C2, s, Ho, reps):
    torch = _setup()
    import synthdata as synth
    from edge_yolo_amd import _lib as L
    from edge_yolo_amd.nn.modules import ResNetBlock
    cx = C1 if C1 else 4 * C2
    m = ResNetBlock(cx, C2, s)
    m.load_state_dict({k: synth.synth_tensor("model.1.layer.0." + k, tuple(v.shape)) for k, v in m.state_dict().items()})
    m = m.cuda().half().eval()
    H = Ho * s
    px = B * Ho * Ho
    K = C2 + C1
    nbytes = 2 * (px * (C2 + 4 * C2) + (px * C1 if C1 else px * 4 * C2) + 4 * C2 * K)
    flops = 2.0 * px * 4 * C2 * K
    nsets = max(2, -(-WORKING_SET // nbytes))
    ts = [torch.randn(B, Ho, Ho, C2, device="cuda", dtype=torch.float16).permute(0, 3, 1, 2) for _ in range(nsets)]
    xs = [torch.randn(B, H, H, cx, device="cuda", dtype=torch.float16).permute(0, 3, 1, 2) for _ in range(nsets)]
    ys = [L.empty_nhwc(B, 4 * C2, Ho, Ho, torch.float16, "cuda") for _ in range(nsets)]

    def run(fused, t, x, y):
        m.tail_fused = fused
        return m.tail(t, x, out=y)

    a = [lambda t=t, x=x, y=y: run(True, t, x, y) for t, x, y in zip(ts, xs, ys)]
    b = [lambda t=t, x=x, y=y: run(False, t, x, y) for t, x, y in zip(ts, xs, ys)]
    t_a, t_b, calls = _compare(torch, reps, a, b)
    from edge_yolo_amd import profiling
    with profiling.trace() as tr:
        ya = run(True, ts[0], xs[0], ys[0]).clone()
    assert [r[0] for r in tr.records] == ["resnet_tail_kernel"], [r[0] for r in tr.records]
    diff = float((ya.float() - run(False, ts[0], xs[0], ys[1]).float()).abs().max())
    r = dict(what="resnet_tail", block="projection" if C1 else "identity", B=B, C1=C1, C2=C2, stride=s, Ho=Ho, Wo=Ho, K=K, Cout=4 * C2, buffer_sets=nsets,
             calls_per_window=calls, alg_MB=round(nbytes / 1e6, 1), GFLOP=round(flops / 1e9, 2), hbm_floor_us=round(nbytes / HBM * 1e6, 1))
    r.update(_stats("fused", t_a, nbytes, flops))
    r.update(_stats("composed", t_b, nbytes + (2 * 2 * px * 4 * C2 if C1 else 0), flops))
    r.update(fused_launches=1, composed_launches=2 if C1 else 1, composed_over_fused=round(r["composed_us"] / r["fused_us"], 2), max_abs_diff=round(diff, 4))
    return r


def _child(args, what, script=None):
    try:
        r = subprocess.run([sys.executable, script or os.path.abspath(__file__)] + args, timeout=CHILD_TIMEOUT, stdout=subprocess.PIPE, text=True)
    except subprocess.TimeoutExpired:
        sys.exit(f"{what}: no result within {CHILD_TIMEOUT} s; stopping")
    if r.returncode != 0:
        sys.exit(f"{what}: exit status {r.returncode}; stopping")
    return [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]


if __name__ == "__main__":
    argv = sys.argv[1:]
    if argv and argv[0] == "--stem":
        print(json.dumps(one_stem(int(argv[1]), int(argv[2]))), flush=True)
        sys.exit(0)
    if argv and argv[0] == "--tail":
        print(json.dumps(one_tail(*(int(a) for a in argv[1:6]))), flush=True)
        sys.exit(0)
    out = os.path.join(ROOT, "profiles", "resnet_bench.txt")
    if argv and argv[0] == "--out":
        out, argv = argv[1], argv[2:]
    reps = int(argv[0]) if argv else 16
    with open(out, "w") as f:
        def emit(line):
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
        emit(f"# tools/resnet_bench.py: batch {B}, f16; median of 5 alternating windows")
        emit("# layer 0: ey_resnet_stem (fused, one launch) vs ey_stem_conv_ks (7, 2, 3) + ey_maxpool3x3s2 (the pair) vs F.conv2d + F.silu + F.max_pool2d, channels_last f16")
        for img in (224, 640):
            emit(_child(["--stem", str(img), str(reps)], f"layer 0 at {img}"))
        emit("# block tails of ResNet-50 at 224x224: ey_resnet_tail (fused, one launch) vs the composed form (shortcut conv where there is one + cv3 with addz)")
        for C1, C2, s, Ho, n in TAILS:
            emit(f"# {n} block(s) of this shape per forward")
            emit(_child(["--tail", str(C1), str(C2), str(s), str(Ho), str(2 * reps)], f"tail C1={C1} C2={C2}"))
        emit(f"# predict(): batch {B}, 224x224, f16, device tensors, captured graph; median of 5 windows of 20 calls; launches of one device step")
        cls_bench = os.path.join(ROOT, "tools", "cls_bench.py")
        for name in ("yolov8n-cls-resnet50.yaml", "yolo11n-cls.yaml"):
            emit(_child(["--predict", name, "224"], name, script=cls_bench))
