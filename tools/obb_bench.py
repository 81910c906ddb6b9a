"""Developer tool for the obb task.  Each measurement runs in a child process of its own under a time limit (the parent never opens the GPU
and stops at the first child that fails or runs out of time):

  nms N      ey_nms_rotated (init + score + rank + pair + resolve, five launches) at batch 32 with N candidates per image out of 8400
             anchors, 15 classes, each image a clustered scene of its own, against the torch-op composition of fast-NMS on ProbIoU on the
             same GPU: per image argsort of the scores, the all-pairs matrix from elementwise torch ops, triu, column max, compare (the
             reference's nms_rotated up to, not including, its nonzero, which synchronises and cannot be captured).  The composition gets
             the candidates already selected (boxes with their class offset, scores); the kernel starts from the prediction tensor.  Both
             are replayed from a hipGraph; timed windows alternate between them (five each, median reported).  The kept columns of both
             are compared.
  predict T  images/s of YOLO(T).predict at 640^2, batch 32, f16, synthetic weights, device-resident input (T = yolo11n-obb.yaml or yolo11n.yaml).

usage: obb_bench.py                      (everything: nms 300, nms 2048, nms 8400, predict obb, predict detect)
       obb_bench.py --nms N | --predict YAML     (one measurement, what the children run)"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
B, A, NC, IMG = 32, 8400, 15, 640
CONF, IOU, MAX_WH = 0.25, 0.45, 7680.0
CHILD_TIMEOUT = 420


def _scenes(torch, n):
    """pred (B, 4+NC+1, A) fp32: per image a clustered scene (tests/obb_synth.scene) whose first n anchors, shuffled, score above conf."""
    import numpy as np
    import obb_synth
    p = np.zeros((B, 4 + NC + 1, A), np.float32)
    for b in range(B):
        r = np.random.default_rng([b, n])
        box = obb_synth.scene(r, A, max(4, n // 12), imgsz=float(IMG))
        best = np.where(np.arange(A) < n, r.uniform(CONF + 0.01, 0.99, A), r.uniform(0.0, CONF - 0.01, A))
        cls = r.integers(0, NC, A)
        perm = r.permutation(A)
        box, best, cls = box[perm], best[perm], cls[perm]
        sc = r.uniform(0.0, 0.5, (NC, A)) * best[None]
        sc[cls, np.arange(A)] = best
        p[b, :4], p[b, 4:4 + NC], p[b, 4 + NC] = box[:, :4].T, sc, box[:, 4]
    return torch.tensor(p).cuda()


def _torch_probiou(torch, o):
    """(n,5) -> (n,n) ProbIoU from elementwise torch ops: Gaussian covariance terms per box, Bhattacharyya distance per pair, Hellinger tail."""
    eps = 1e-7
    x, y = o[:, 0:1], o[:, 1:2]
    va, vb = o[:, 2:3] ** 2 / 12, o[:, 3:4] ** 2 / 12
    c, s = torch.cos(o[:, 4:5]), torch.sin(o[:, 4:5])
    a, b, k = va * c * c + vb * s * s, va * s * s + vb * c * c, (va - vb) * c * s
    sa, sb, sk = a + a.T, b + b.T, k + k.T
    det = sa * sb - sk * sk
    dx, dy = x - x.T, y - y.T
    t1 = (sa * dy * dy + sb * dx * dx) / (det + eps) * 0.25
    t2 = (sk * -dx * dy) / (det + eps) * 0.5
    d = (a * b - k * k).clamp(min=0)
    t3 = (det / (4 * (d * d.T).sqrt() + eps) + eps).log() * 0.5
    bd = (t1 + t2 + t3).clamp(eps, 100.0)
    return 1 - (1 - (-bd).exp() + eps).sqrt()


def nms(n):
    from process_mask_bench import _setup, _timers
    torch = _setup()
    from edge_yolo_amd.utils import ops as uops
    graph_of, window, ab = _timers(torch)
    pred = _scenes(torch, n)
    out = [None]

    def hip():
        out[0] = uops.nms_device(pred, CONF, IOU, None, False, 300, nc=NC, rotated=True)

    # the composition's input: the candidates of each image, class offset added (what the reference hands to nms_rotated)
    cands = []
    for b in range(B):
        sc, cls = pred[b, 4:4 + NC].max(0)
        sel = (sc > CONF).nonzero().squeeze(1)
        off = cls[sel].float()[:, None] * MAX_WH
        cands.append((torch.cat([pred[b, :2, sel].T + off, pred[b, 2:4, sel].T, pred[b, 4 + NC:, sel].T], 1).contiguous(), sc[sel].contiguous(), sel))
    keep = [None] * B

    def eager():
        for b, (boxes, scores, _) in enumerate(cands):
            order = torch.argsort(scores, descending=True)
            ious = _torch_probiou(torch, boxes[order]).triu_(diagonal=1)
            keep[b] = (order, ious.max(dim=0)[0] < IOU)

    g_hip, g_t = graph_of(hip), graph_of(eager)
    th, tt = ab(g_hip, g_t)
    g_hip.replay()
    g_t.replay()
    torch.cuda.synchronize()
    rows, count, index = out[0]
    differ, kept = 0, 0
    for b in range(B):
        order, flag = keep[b]
        want = cands[b][2][order[flag]][:300].cpu().tolist()
        got = index[b, :int(count[b])].cpu().tolist()
        kept += len(got)
        differ += len(set(want) ^ set(got))
    pairs = B * n * (n - 1) // 2
    print(json.dumps(dict(what="nms_rotated", B=B, A=A, nc=NC, candidates=n, hip_us=round(th[2], 1), hip_us_min=round(th[0], 1), hip_us_max=round(th[4], 1),
                          torch_us=round(tt[2], 1), torch_us_min=round(tt[0], 1), torch_us_max=round(tt[4], 1), torch_over_hip=round(tt[2] / th[2], 2),
                          pairs=pairs, Gpairs_per_s=round(pairs / th[2] / 1e3, 2), kept_rows=kept, kept_anchors_differing_from_torch=differ)), flush=True)


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
    if a and a[0] == "--nms":
        nms(int(a[1]))
    elif a and a[0] == "--predict":
        predict(a[1])
    else:
        for args in (["--nms", "300"], ["--nms", "2048"], ["--nms", "8400"], ["--predict", "yolo11n-obb.yaml"], ["--predict", "yolo11n.yaml"]):
            print("# " + " ".join(args), flush=True)
            try:
                rc = subprocess.run([sys.executable, os.path.abspath(__file__), *args], timeout=CHILD_TIMEOUT).returncode
            except subprocess.TimeoutExpired:
                sys.exit(f"{args}: no result within {CHILD_TIMEOUT} s; stopping")
            if rc != 0:
                sys.exit(f"{args}: exit status {rc}; stopping")
