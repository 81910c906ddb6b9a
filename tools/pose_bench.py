"""Developer tool for the pose task.  Each measurement runs in a child process of its own under a time limit (the parent never opens the GPU
and stops at the first child that fails or runs out of time); the result lines are printed and written to profiles/pose_bench.txt.

  rows       ey_kpts_decode_rows at batch 32, 8400 anchors (80^2 + 40^2 + 20^2), 51 channels, f16 maps, max_det 300, against the composition
             it replaces: ey_kpts_decode_levels of every anchor into (B, 51, A), then the torch.gather of the kept columns by anchor index
             that nms_device's coefficient branch uses.  Both are replayed from a hipGraph; timed windows alternate between them (five each,
             median, minimum and maximum reported: the spread of the session).  The outputs are compared.
  oks        ey_kpt_iou for 32 images x (10 ground truths x 300 predictions), one call, against the per-image torch composition of the
             reference's kpt_iou on the same GPU (elementwise ops, one set per image), both from a hipGraph.
  predict T  images/s of YOLO(T).predict at 640^2, batch 32, f16, synthetic weights, device-resident input (T = yolo11n-pose.yaml or yolo11n.yaml).

usage: pose_bench.py                                (everything: rows, oks, predict pose, predict detect)
       pose_bench.py --rows | --oks | --predict YAML     (one measurement, what the children run)"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
B, IMG, MAX_DET, KPT = 32, 640, 300, (17, 3)
CONF = 0.25
CHILD_TIMEOUT = 420


def _maps(torch):
    from edge_yolo_amd import _lib as L
    torch.manual_seed(0)
    levels, a_off = [], 0
    for s in (8, 16, 32):
        h = IMG // s
        m = L.empty_nhwc(B, 56, h, h, torch.float16, "cuda")[:, :51]
        m.copy_(torch.randn(B, 51, h, h, device="cuda") * 2)
        levels.append((m, float(s), a_off))
        a_off += h * h
    return levels, a_off


def rows():
    from process_mask_bench import _setup, _timers
    torch = _setup()
    from edge_yolo_amd.nn import _ops
    graph_of, window, ab = _timers(torch)
    levels, A = _maps(torch)
    g = torch.Generator(device="cuda").manual_seed(1)
    index = torch.randint(0, A, (B, MAX_DET), device="cuda", generator=g, dtype=torch.int32)
    count = torch.full((B,), MAX_DET, dtype=torch.int32, device="cuda")
    full = torch.empty((B, 51, A), dtype=torch.float32, device="cuda")
    out = [None, None]

    def hip():
        out[0] = _ops.kpts_decode_rows(levels, KPT, index, count, A)

    def composition():
        _ops.kpts_decode_levels(levels, KPT, full)
        ok = index >= 0
        idx = index.clamp(min=0).long()[:, None, :].expand(-1, 51, -1)
        out[1] = torch.gather(full, 2, idx).transpose(1, 2) * ok[..., None]

    g_hip, g_t = graph_of(hip), graph_of(composition)
    th, tt = ab(g_hip, g_t)
    g_hip.replay()
    g_t.replay()
    torch.cuda.synchronize()
    same = bool(torch.equal(out[0].view(B, MAX_DET, 51), out[1]))
    nbytes = B * MAX_DET * 51 * (2 + 4)
    print(json.dumps(dict(what="kpts_decode_rows", B=B, A=A, nk=51, max_det=MAX_DET, hip_us=round(th[2], 2), hip_us_min=round(th[0], 2), hip_us_max=round(th[4], 2),
                          composition_us=round(tt[2], 2), composition_us_min=round(tt[0], 2), composition_us_max=round(tt[4], 2),
                          composition_over_hip=round(tt[2] / th[2], 2), GB_per_s=round(nbytes / th[2] / 1e3, 1), equal_to_composition=same)), flush=True)


def oks():
    from process_mask_bench import _setup, _timers
    torch = _setup()
    import numpy as np
    import pose_synth
    from edge_yolo_amd.nn import _ops
    graph_of, window, ab = _timers(torch)
    M, N = 10, MAX_DET
    gts, preds, areas = [], [], []
    for b in range(B):
        r = np.random.default_rng([b, 5])
        g, box = pose_synth.people(r, M, 17, float(IMG))
        gts.append(g); preds.append(pose_synth.guesses(r, g, box, N, 3)); areas.append(pose_synth._area(box))
    gt, pred, area = (torch.tensor(np.concatenate(t)).cuda() for t in (gts, preds, areas))
    sigma = torch.tensor(pose_synth.OKS_SIGMA.astype(np.float32)).cuda()
    pred_off, gt_off = [N * b for b in range(B + 1)], [M * b for b in range(B + 1)]
    res = [None, [None] * B]

    def hip():
        res[0] = _ops.kpt_iou(pred, pred_off, gt, gt_off, area, sigma)[0]

    def composition():
        for b in range(B):
            k1, k2, a = gt[b * M:(b + 1) * M], pred[b * N:(b + 1) * N], area[b * M:(b + 1) * M]
            d = (k1[:, None, :, 0] - k2[..., 0]).pow(2) + (k1[:, None, :, 1] - k2[..., 1]).pow(2)
            mask = k1[..., 2] != 0
            e = d / ((2 * sigma).pow(2) * (a[:, None, None] + 1e-7) * 2)
            res[1][b] = ((-e).exp() * mask[:, None]).sum(-1) / (mask.sum(-1)[:, None] + 1e-7)

    g_hip, g_t = graph_of(hip), graph_of(composition)
    th, tt = ab(g_hip, g_t)
    g_hip.replay()
    g_t.replay()
    torch.cuda.synchronize()
    gap = float((res[0].view(B, M, N) - torch.stack(res[1])).abs().max())
    pairs = B * M * N
    print(json.dumps(dict(what="kpt_iou", B=B, gt_per_image=M, pred_per_image=N, K=17, hip_us=round(th[2], 2), hip_us_min=round(th[0], 2), hip_us_max=round(th[4], 2),
                          torch_us=round(tt[2], 1), torch_us_min=round(tt[0], 1), torch_us_max=round(tt[4], 1), torch_over_hip=round(tt[2] / th[2], 2),
                          Mpairs_per_s=round(pairs / th[2], 1), max_gap_to_torch=gap)), flush=True)


def predict(name):
    from process_mask_bench import _setup
    torch = _setup()
    import time
    import edge_yolo_amd
    import synthdata as synth
    model = edge_yolo_amd.YOLO(name)
    model.model.load_state_dict(synth.synth_state_dict({k: tuple(v.shape) for k, v in model.model.state_dict().items()}))
    x = synth.synth_images(B, IMG, IMG).cuda().half()
    for _ in range(3):
        res = model.predict(x, half=True, conf=CONF, device="cuda:0")
    torch.cuda.synchronize()
    times = []
    for _ in range(5):
        t0, k = time.perf_counter(), 20
        for _ in range(k):
            res = model.predict(x, half=True, conf=CONF, device="cuda:0")
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) / k)
    times.sort()
    print(json.dumps(dict(what="predict", model=name, task=model.task, batch=B, imgsz=IMG, half=True, ms_per_batch=round(times[2] * 1e3, 3),
                          ms_min=round(times[0] * 1e3, 3), ms_max=round(times[4] * 1e3, 3), images_per_s=round(B / times[2], 1),
                          kept_rows=sum(len(r) for r in res))), flush=True)


if __name__ == "__main__":
    a = sys.argv[1:]
    if a and a[0] == "--rows":
        rows()
    elif a and a[0] == "--oks":
        oks()
    elif a and a[0] == "--predict":
        predict(a[1])
    else:
        lines = []
        for args in (["--rows"], ["--oks"], ["--predict", "yolo11n-pose.yaml"], ["--predict", "yolo11n.yaml"]):
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
        out = a[1] if len(a) == 2 and a[0] == "--out" else os.path.join(ROOT, "profiles", "pose_bench.txt")
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")
