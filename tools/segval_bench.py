"""Developer tool for segment validation.  Each measurement runs in a child process of its own under a time limit (the parent never opens
the GPU and stops at the first child that fails or runs out of time):

  iou    ey_mask_iou (pack predictions + pack ground truth + pairs, three launches) against the torch composition the reference uses
         (utils/metrics.py::mask_iou per image: matmul of float masks, sums, division; in index mode with the reference's
         repeat + where expansion in front, models/yolo/segment/val.py:206-209) on the same GPU: batch 32, 300 predictions and 20 instances
         per image, masks S x S.  Both forms are replayed from a hipGraph; timed windows alternate between them (five each, median
         reported).  The kernel reads uint8 masks (what ey_process_mask writes), torch the float masks the reference's process_mask returns.
         Bytes = what the kernel must move: every mask once (pack), the packed words once more and the matrices (pair).
  step   one validation step of yolo11n-seg at batch 32, 640^2, f16 (synthetic weights, 20 labels per image): forward, NMS, masks, IoU,
         matching; launches, share of the mask kernels in the traced device time, wall time per step.

usage: segval_bench.py                      (everything: iou 160 stack, iou 160 index, iou 640 stack, iou 640 index, step)
       segval_bench.py --iou S stack|index | --step     (one measurement, what the children run)"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
B, N, M, IMG = 32, 300, 20, 640
HBM = 8.0e12
CHILD_TIMEOUT = 300


def iou(S, mode):
    from process_mask_bench import _setup, _timers
    torch = _setup()
    from edge_yolo_amd import _lib as L
    from edge_yolo_amd.nn import _ops as ops
    graph_of, window, ab = _timers(torch)
    torch.manual_seed(0)
    index = mode == "index"
    pred = torch.empty(B * N, S, S, dtype=torch.uint8, device="cuda")
    for i in range(B):  # blobs are not needed: the cost does not depend on the pattern; a fifth of the pixels set
        pred[i * N:(i + 1) * N] = torch.rand(N, S, S, device="cuda") < 0.2
    if index:
        gt = torch.randint(0, M + 1, (B, S, S), dtype=torch.int32, device="cuda")
    else:
        gt = (torch.rand(B * M, S, S, device="cuda") < 0.2).to(torch.uint8)
    pred_off, gt_off = [i * N for i in range(B + 1)], [i * M for i in range(B + 1)]
    out = torch.empty(B * M * N, dtype=torch.float32, device="cuda")
    ws = torch.empty(L.lib().ey_mask_iou_workspace_bytes(S, S, B * N, B * M), dtype=torch.uint8, device="cuda")

    def hip():
        ops.mask_iou(pred, pred_off, gt, gt_off, index=index, iou=out, workspace=ws)

    pf = pred.view(B * N, -1).float()  # what the reference holds: float masks
    gf = gt.float() if index else gt.view(B * M, -1).float()
    idx = torch.arange(M, device="cuda").view(M, 1, 1) + 1
    res = [None] * B

    def eager():
        for i in range(B):
            g = torch.where(gf[i:i + 1].repeat(M, 1, 1) == idx, 1.0, 0.0).view(M, -1) if index else gf[i * M:(i + 1) * M]
            p = pf[i * N:(i + 1) * N]
            inter = torch.matmul(g, p.T).clamp_(0)
            union = (g.sum(1)[:, None] + p.sum(1)[None]) - inter
            res[i] = inter / (union + 1e-7)

    g_hip, g_t = graph_of(hip), graph_of(eager)
    th, tt = ab(g_hip, g_t)
    hip()
    eager()
    torch.cuda.synchronize()
    diff = int((torch.stack(res).view(torch.int32) != out.view(B, M, N).view(torch.int32)).sum())
    words = (S * S + 63) // 64
    nbytes = pred.numel() + gt.numel() * gt.element_size() + 2 * 8 * words * B * (N + M) + 4 * out.numel()
    print(json.dumps(dict(what="mask_iou", S=S, gt=mode, B=B, N=N, M=M, hip_us=round(th[2], 1), hip_us_min=round(th[0], 1), hip_us_max=round(th[4], 1),
                          torch_us=round(tt[2], 1), torch_us_min=round(tt[0], 1), torch_us_max=round(tt[4], 1), torch_over_hip=round(tt[2] / th[2], 2),
                          alg_MB=round(nbytes / 1e6, 1), achieved_TBps=round(nbytes / th[2] / 1e6, 3), share_of_hbm_peak=round(nbytes / HBM * 1e6 / th[2], 3),
                          torch_operand_MB=round((pf.numel() + gf.numel()) * 4 / 1e6, 1), values_differing_from_torch=diff, values=int(out.numel()))), flush=True)


def step():
    from process_mask_bench import _setup
    torch = _setup()
    import time
    import numpy as np
    from edge_yolo_amd import profiling
    from edge_yolo_amd.engine.validator import SegmentationValidator
    from edge_yolo_amd.nn.tasks import SegmentationModel
    import seg_synth
    import synthdata as synth
    m = SegmentationModel("yolo11n-seg.yaml")
    m.load_state_dict(seg_synth.state_dict(m.state_dict()))
    m = m.to("cuda")
    m.fuse()
    m = m.half().eval()
    r = np.random.default_rng(0)
    c, wh = r.uniform(0.2, 0.8, (B * M, 2)), r.uniform(0.05, 0.3, (B * M, 2))
    batch = {"img": synth.synth_images(B, IMG, IMG).half().cuda(), "cls": r.integers(0, 80, (B * M, 1)).astype(np.float32),
             "bboxes": np.concatenate([c, wh], 1).astype(np.float32), "batch_idx": np.repeat(np.arange(B), M).astype(np.float32),
             "masks": torch.randint(0, M + 1, (B, IMG // 4, IMG // 4), dtype=torch.uint8).cuda(), "ori_shape": [(IMG, IMG)] * B, "ratio_pad": None}
    v = SegmentationValidator(m, half=True)

    def one():
        b = v.preprocess(batch)
        preds = v.postprocess(m(b["img"]))
        v.update_metrics(preds, b)
        return preds

    with torch.no_grad():
        preds = one()
        with profiling.trace() as t:
            one()
        agg = t.summary()
        total = sum(a["ms"] for a in agg.values())
        new = {k: dict(launches=a["kernels"], ms=round(a["ms"], 4), share=round(a["ms"] / total, 4)) for k, a in agg.items() if k in ("process_mask_kernel", "mask_iou_kernels")}
        torch.cuda.synchronize()
        t0, n = time.perf_counter(), 10
        for _ in range(n):
            one()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / n
    print(json.dumps(dict(what="val step yolo11n-seg", batch=B, imgsz=IMG, half=True, kept_rows=sum(len(p) for p in preds[0]), labels=B * M,
                          launches=sum(a["kernels"] for a in agg.values()), traced_device_ms=round(total, 3), mask_kernels=new,
                          ms_per_step=round(dt * 1e3, 3), images_per_s=round(B / dt, 1))), flush=True)


if __name__ == "__main__":
    a = sys.argv[1:]
    if a and a[0] == "--iou":
        iou(int(a[1]), a[2])
    elif a and a[0] == "--step":
        step()
    else:
        for args in (["--iou", "160", "stack"], ["--iou", "160", "index"], ["--iou", "640", "stack"], ["--iou", "640", "index"], ["--step"]):
            print("# " + " ".join(args), flush=True)
            try:
                rc = subprocess.run([sys.executable, os.path.abspath(__file__), *args], timeout=CHILD_TIMEOUT).returncode
            except subprocess.TimeoutExpired:
                sys.exit(f"{args}: no result within {CHILD_TIMEOUT} s; stopping")
            if rc != 0:
                sys.exit(f"{args}: exit status {rc}; stopping")
