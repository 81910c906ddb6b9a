"""Developer tool for obb validation.  Each measurement runs in a child process of its own under a time limit (the parent never opens the GPU
and stops at the first child that fails or runs out of time):

  nms N      ey_nms_rotated_ml (init + score + select + rank + pair + resolve, six launches) at batch 32, 8400 anchors, 15 classes, with N
             (anchor, class) scores per image above conf (max_nms 30000: N above it makes the cut active), each image a clustered scene of
             its own, against (a) the torch-op composition of the reference's algorithm on the same GPU -- per image argsort of the
             candidates' scores, the cut, the all-pairs ProbIoU matrix from elementwise torch ops, triu, column max, compare; it gets the
             candidates already selected, the kernel starts from the prediction tensor; with the cut active the 30000^2 matrices are built
             for the first image only and the time is scaled by the batch -- and (b) single-label ey_nms_rotated on a prediction with the
             same number of candidates (N <= 8400), whose pair stage is the same kernel.  All are replayed from a hipGraph; timed windows
             alternate (five each, median reported).  The kept rows of the kernel and the composition are compared.
  probiou    ey_probiou_batch for 32 images x (20 labels x 300 predictions), one call, against 32 ey_probiou calls.

usage: obbval_bench.py                   (everything: nms 300, nms 8400, nms 40000, probiou)
       obbval_bench.py --nms N | --probiou      (one measurement, what the children run)"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
B, A, NC, IMG = 32, 8400, 15, 640
CONF, IOU, MAX_WH, MAX_NMS = 0.25, 0.45, 7680.0, 30000
CHILD_TIMEOUT = 420


def _scenes(torch, n):
    """pred (B, 4+NC+1, A) fp32: per image a clustered scene (tests/obb_synth.scene) with n of the A * NC scores, at random places, above conf."""
    import numpy as np
    import obb_synth
    p = np.zeros((B, 4 + NC + 1, A), np.float32)
    for b in range(B):
        r = np.random.default_rng([b, n, 1])
        box = obb_synth.scene(r, A, max(4, min(n, A) // 12), imgsz=float(IMG))
        hot = np.zeros(NC * A, bool)
        hot[r.permutation(NC * A)[:n]] = True
        sc = np.where(hot.reshape(NC, A), r.uniform(CONF + 0.01, 0.99, (NC, A)), r.uniform(0.0, CONF - 0.01, (NC, A)))
        p[b, :4], p[b, 4:4 + NC], p[b, 4 + NC] = box[:, :4].T, sc, box[:, 4]
    return torch.tensor(p).cuda()


def nms(n):
    from obb_bench import _scenes as single_scenes
    from obb_bench import _torch_probiou
    from process_mask_bench import _setup, _timers
    torch = _setup()
    from edge_yolo_amd.utils import ops as uops
    graph_of, window, ab = _timers(torch)
    pred = _scenes(torch, n)
    out = [None]

    def hip():
        out[0] = uops.nms_rotated_multi_label(pred, CONF, IOU, None, False, 300, nc=NC, max_nms=MAX_NMS)

    # the composition's input: the candidates of each image in torch.where order, class offset added (what the reference hands to nms_rotated)
    cut = n > MAX_NMS
    cands = []
    for b in range(1 if cut else B):
        a, c = torch.where(pred[b, 4:4 + NC].T > CONF)
        off = c.float()[:, None] * MAX_WH
        cands.append((torch.cat([pred[b, :2, a].T + off, pred[b, 2:4, a].T, pred[b, 4 + NC:, a].T], 1).contiguous(), pred[b, 4 + c, a].contiguous(), a, c))
    keep = [None] * len(cands)

    def eager():
        for b, (boxes, scores, _, _) in enumerate(cands):
            order = torch.argsort(scores, descending=True)[:MAX_NMS]
            ious = _torch_probiou(torch, boxes[order]).triu_(diagonal=1)
            keep[b] = (order, ious.max(dim=0)[0] < IOU)

    g_hip, g_t = graph_of(hip), graph_of(eager, warm=1)
    th, tt = ab(g_hip, g_t)
    scale = B if cut else 1
    g_hip.replay()
    g_t.replay()
    torch.cuda.synchronize()
    rows, count, index = out[0]
    differ, kept = 0, 0
    for b in range(len(cands)):
        order, flag = keep[b]
        sel = order[flag][:300]
        want = list(zip(cands[b][2][sel].cpu().tolist(), cands[b][3][sel].cpu().tolist()))
        k = int(count[b])
        got = list(zip(index[b, :k].cpu().tolist(), rows[b, :k, 5].long().cpu().tolist()))
        kept += len(got)
        differ += len(set(want) ^ set(got))
    m = min(n, MAX_NMS)
    pairs = B * m * (m - 1) // 2
    res = dict(what="nms_rotated_ml", B=B, A=A, nc=NC, candidates=n, after_cut=m, hip_us=round(th[2], 1), hip_us_min=round(th[0], 1), hip_us_max=round(th[4], 1),
               torch_us=round(tt[2] * scale, 1), torch_us_min=round(tt[0] * scale, 1), torch_us_max=round(tt[4] * scale, 1), torch_images_timed=len(cands),
               torch_over_hip=round(tt[2] * scale / th[2], 2), pairs=pairs, Gpairs_per_s=round(pairs / th[2] / 1e3, 2), kept_rows_compared=kept,
               kept_pairs_differing_from_torch=differ)
    if n <= A:  # single label with as many candidates: the same pair stage behind the all-pairs rank over A keys
        sp = single_scenes(torch, n)
        g_s = graph_of(lambda: uops.nms_device(sp, CONF, IOU, None, False, 300, nc=NC, rotated=True))
        ts, th2 = ab(g_s, g_hip)
        res.update(single_label_us=round(ts[2], 1), single_label_us_min=round(ts[0], 1), single_label_us_max=round(ts[4], 1), hip_us_beside_single=round(th2[2], 1))
    print(json.dumps(res), flush=True)


def probiou():
    import numpy as np
    from process_mask_bench import _setup, _timers
    torch = _setup()
    import obb_synth
    from edge_yolo_amd.nn import _ops
    graph_of, window, ab = _timers(torch)
    M, N = 20, 300
    r = np.random.default_rng(5)
    pred = torch.tensor(np.concatenate([obb_synth.scene(r, N, 25, imgsz=float(IMG)) for _ in range(B)])).cuda()
    gt = torch.tensor(np.concatenate([obb_synth.scene(r, M, 20, imgsz=float(IMG)) for _ in range(B)])).cuda()
    poff, goff = [N * b for b in range(B + 1)], [M * b for b in range(B + 1)]
    flat = torch.empty(B * M * N, device="cuda")
    single = [None] * B

    def batch():
        _ops.probiou_batch(pred, poff, gt, goff, out=flat)

    def calls():
        for b in range(B):
            single[b] = _ops.probiou(gt[goff[b]:goff[b + 1]], pred[poff[b]:poff[b + 1]])

    g_b, g_c = graph_of(batch), graph_of(calls)
    tb, tc = ab(g_b, g_c)
    g_b.replay()
    g_c.replay()
    torch.cuda.synchronize()
    same = all(torch.equal(flat[b * M * N:(b + 1) * M * N].view(M, N), single[b]) for b in range(B))
    print(json.dumps(dict(what="probiou_batch", B=B, labels=M, predictions=N, batch_us=round(tb[2], 1), batch_us_min=round(tb[0], 1), batch_us_max=round(tb[4], 1),
                          calls_us=round(tc[2], 1), calls_us_min=round(tc[0], 1), calls_us_max=round(tc[4], 1), calls_over_batch=round(tc[2] / tb[2], 2),
                          bit_identical=same)), flush=True)


if __name__ == "__main__":
    a = sys.argv[1:]
    if a and a[0] == "--nms":
        nms(int(a[1]))
    elif a and a[0] == "--probiou":
        probiou()
    else:
        for args in (["--nms", "300"], ["--nms", "8400"], ["--nms", "40000"], ["--probiou"]):
            print("# " + " ".join(args), flush=True)
            try:
                rc = subprocess.run([sys.executable, os.path.abspath(__file__), *args], timeout=CHILD_TIMEOUT).returncode
            except subprocess.TimeoutExpired:
                sys.exit(f"{args}: no result within {CHILD_TIMEOUT} s; stopping")
            if rc != 0:
                sys.exit(f"{args}: exit status {rc}; stopping")
