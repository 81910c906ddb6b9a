"""Developer tool for the classify task.  Each measurement runs in a child process of its own under a time limit (the parent never opens the
GPU and stops at the first child that fails or runs out of time); the result lines are printed and written to profiles/cls_bench.txt.

  tail B       the two kernels of the Classify head (ey_classify_pool, ey_classify_linear_softmax) at batch B on a 7x7x256 f16 map, nc 1000,
               against the composition they replace: the existing 1x1 Conv (MFMA, SiLU) writing the (B,1280,7,7) map -> torch.mean ->
               torch.nn.functional.linear -> softmax -> topk(5).  Both are replayed from a hipGraph; timed windows alternate between them
               (five each; median, minimum and maximum reported).  The pool kernel and the conv + mean it replaces are also timed alone: the
               fused pool is the shipped form when its slowest window beats the fastest of conv + mean.
  transform    ey_classify_transform for 32 images 480x640 -> 224 (one launch, device-resident uint8 batch) against per-image Pillow on the
               host (resize, crop, to float) plus the upload of the float batch.
  predict T    images/s of YOLO(T).predict, batch 32, f16, synthetic weights, device-resident input, with the launches per batch: yolo11n-cls
               at 224^2, and yolo11n detect at 640^2 from the same run for scale (the tasks are not comparable beyond that).

usage: cls_bench.py                                   (everything)
       cls_bench.py --tail B | --transform | --predict YAML IMGSZ     (one measurement, what the children run)"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
C1, HW, NC, B_PRED = 256, 7, 1000, 32
CHILD_TIMEOUT = 420


def _r(t):
    return dict(us=round(t[2], 2), us_min=round(t[0], 2), us_max=round(t[4], 2))


def tail(B):
    from process_mask_bench import _setup, _timers
    torch = _setup()
    import torch.nn.functional as F
    from edge_yolo_amd import _lib as L
    from edge_yolo_amd.nn import _ops
    from edge_yolo_amd.nn.modules import Classify
    graph_of, window, ab = _timers(torch)
    torch.manual_seed(0)
    torch.set_grad_enabled(False)
    head = Classify(C1, NC)
    for p in head.parameters():
        torch.nn.init.normal_(p, 0.0, 0.05)
    head = head.cuda().half().eval()
    head.conv.fuse_bn()
    x = L.empty_nhwc(B, C1, HW, HW, torch.float16, "cuda")
    x.copy_(torch.randn(B, C1, HW, HW, device="cuda"))
    wc, bc, wl, bl = head._weights(torch.float16, x.device)
    out = {}

    def hip():
        out["hip"] = head(x)

    def composition():
        m = head.conv(x)  # the MFMA 1x1 conv + SiLU of the other tasks, writing the (B,1280,7,7) map
        pooled = m.float().mean((2, 3))
        logits = F.linear(pooled, head.linear.weight.float(), head.linear.bias.float())
        probs = logits.softmax(1)
        out["ref"] = (probs, logits, probs.topk(5, 1))

    def pool_only():
        out["pool"] = _ops.classify_pool(x, wc, bc, L.ACT_SILU)

    def conv_mean():
        out["cm"] = head.conv(x).float().mean((2, 3))

    g_hip, g_ref, g_pool, g_cm = graph_of(hip), graph_of(composition), graph_of(pool_only), graph_of(conv_mean)
    th, tr = ab(g_hip, g_ref)
    tp, tc = ab(g_pool, g_cm)
    for g in (g_hip, g_ref, g_pool, g_cm):
        g.replay()
    torch.cuda.synchronize()
    gap = float((out["hip"][0] - out["ref"][0]).abs().max())
    same_top1 = bool(torch.equal(head.top5[0][:, 0].long(), out["ref"][2].indices[:, 0]))
    print(json.dumps(dict(what="classify_tail", B=B, map=f"{HW}x{HW}x{C1}", nc=NC, hip=_r(th), composition=_r(tr), composition_over_hip=round(tr[2] / th[2], 2),
                          pool=_r(tp), conv_mean=_r(tc), conv_mean_over_pool=round(tc[2] / tp[2], 2), fused_pool_wins=bool(tp[4] < tc[0]),
                          pool_TFLOPs=round(2.0 * B * HW * HW * C1 * 1280 / tp[2] / 1e6, 2), max_prob_gap_to_composition=gap, top1_equal=same_top1)), flush=True)


def transform():
    from process_mask_bench import _setup, _timers
    torch = _setup()
    import time
    import numpy as np
    from PIL import Image
    from edge_yolo_amd.data.augment import ClassifyTransform
    graph_of, window, ab = _timers(torch)
    B, h, w, S = 32, 480, 640, 224
    r = np.random.default_rng(0)
    ims = r.integers(0, 256, (B, h, w, 3), dtype=np.uint8)
    dev = torch.tensor(ims).cuda()
    t = ClassifyTransform(S)
    out = {}

    def hip():
        out["y"] = t.batch_tensor(dev, torch.float16)

    g = graph_of(hip)
    k = max(1, int(0.25e6 / window(g, 1)))
    th = sorted(window(g, k) for _ in range(5))

    def host():
        nh, nw = t.resized(h, w, S)
        top, left = t.crop_origin(nh, S), t.crop_origin(nw, S)
        rows = [np.asarray(Image.fromarray(a[..., ::-1]).resize((nw, nh), Image.BILINEAR))[top:top + S, left:left + S] for a in ims]
        x = torch.from_numpy(np.stack(rows)).permute(0, 3, 1, 2).float().div(255.0)
        y = x.cuda().half()
        torch.cuda.synchronize()
        return y

    host()
    tt = []
    for _ in range(5):
        t0 = time.perf_counter()
        y = host()
        tt.append((time.perf_counter() - t0) * 1e6)
    tt.sort()
    g.replay()
    torch.cuda.synchronize()
    gap = float((out["y"].float() - y.float()).abs().max()) * 255.0
    print(json.dumps(dict(what="classify_transform", B=B, src=f"{h}x{w}", size=S, hip=_r(th), pillow_host_plus_upload=_r(tt), host_over_hip=round(tt[2] / th[2], 1),
                          GB_per_s=round((B * h * w * 3 + B * 3 * S * S * 2) / th[2] / 1e3, 1), max_gap_to_pillow_levels=round(gap, 3))), flush=True)


def predict(name, imgsz):
    from process_mask_bench import _setup
    torch = _setup()
    import time
    import edge_yolo_amd
    import synthdata as synth
    from edge_yolo_amd import profiling
    model = edge_yolo_amd.YOLO(name)
    model.model.load_state_dict(synth.synth_state_dict({k: tuple(v.shape) for k, v in model.model.state_dict().items()}))
    x = synth.synth_images(B_PRED, imgsz, imgsz).cuda().half()
    for _ in range(3):
        res = model.predict(x, half=True, device="cuda:0")
    torch.cuda.synchronize()
    times = []
    for _ in range(5):
        t0, k = time.perf_counter(), 20
        for _ in range(k):
            res = model.predict(x, half=True, device="cuda:0")
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) / k)
    times.sort()
    launches = None
    if model.task == "classify":  # the launches of one eager device step (what the graph replays)
        with profiling.trace() as tr:
            model.predictor._device_step(x)
        torch.cuda.synchronize()
        launches = sum(r[6] for r in tr.records)
    print(json.dumps(dict(what="predict", model=name, task=model.task, batch=B_PRED, imgsz=imgsz, half=True, ms_per_batch=round(times[2] * 1e3, 3),
                          ms_min=round(times[0] * 1e3, 3), ms_max=round(times[4] * 1e3, 3), images_per_s=round(B_PRED / times[2], 1),
                          launches=launches, results=len(res))), flush=True)


if __name__ == "__main__":
    a = sys.argv[1:]
    if a and a[0] == "--tail":
        tail(int(a[1]))
    elif a and a[0] == "--transform":
        transform()
    elif a and a[0] == "--predict":
        predict(a[1], int(a[2]))
    else:
        lines = []
        for args in (["--tail", "32"], ["--tail", "256"], ["--transform"], ["--predict", "yolo11n-cls.yaml", "224"], ["--predict", "yolo11n.yaml", "640"]):
            lines.append("# " + " ".join(args))
            print(lines[-1], flush=True)
            try:
                p = subprocess.run([sys.executable, os.path.abspath(__file__), *args], timeout=CHILD_TIMEOUT, stdout=subprocess.PIPE, text=True)
            except subprocess.TimeoutExpired:
                sys.exit(f"{args}: no result within {CHILD_TIMEOUT} s; stopping")
            print(p.stdout, end="", flush=True)
            if p.returncode != 0:
                sys.exit(f"{args}: exit status {p.returncode}; stopping")
            lines += [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
        out = a[1] if len(a) == 2 and a[0] == "--out" else os.path.join(ROOT, "profiles", "cls_bench.txt")
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")
