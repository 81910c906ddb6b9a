"""-m gpu: the segment task end to end.  yolo11n-seg (64x96) and the EdgeLine-n graph with a Segment head (64x64) against the reference's
forward (tests/golden, fp32; tolerances of tests/test_gpu_model.py), NMS with mask coefficients, mask assembly on the golden's own
prototypes / rows / boxes, and YOLO(...).predict(): masks equal the float64 restatement applied to that run's own prototypes, coefficient
maps, anchor indices and boxes (which proves the gather and the level mapping), across batch sizes, and None where nothing is kept."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import fp64_mask_ref as f64  # noqa: E402
import seg_synth  # noqa: E402
import synthdata as synth  # noqa: E402

LAYER_TOL = dict(rtol=1e-4, atol=2e-4)  # tests/test_gpu_model.py, fp32 layers


def _cfg(which):
    from edge_yolo_amd.nn.tasks import yaml_model_load
    return "yolo11n-seg.yaml" if which == "yolo11n" else seg_synth.edgeline_seg_cfg(yaml_model_load("yolo11n-test.yaml"))


def _build(which, dtype):
    from edge_yolo_amd.nn.tasks import SegmentationModel
    m = SegmentationModel(_cfg(which))
    m.load_state_dict(seg_synth.state_dict(m.state_dict()))
    m = m.to("cuda")
    m.fuse()
    return (m.half() if dtype == torch.float16 else m.float()).eval()


MODELS = [("yolo11n", "yolo11n_seg_64x96", None, (1, 64, 96)), ("edgeline", "edgeline_n_seg_64", "edgeline_n_64", (2, 64, 64))]


@pytest.mark.parametrize("which,tag,base,shape", MODELS, ids=["yolo11n-seg", "edgeline-n-seg"])
def test_fp32_vs_reference_golden(golden_dir, which, tag, base, shape):
    g = dict(np.load(os.path.join(golden_dir, tag + ".npz")))
    if base:  # layers 0-22 repeat the detect golden bit for bit (make_golden_seg.py checks it)
        g.update({k: v for k, v in np.load(os.path.join(golden_dir, base + ".npz")).items() if k.startswith("layer") and k != "layer23"})
    m = _build(which, torch.float32)
    x = synth.synth_images(*shape).cuda()
    y, (raw, mc, p) = m(x)
    for name, got in (("y", y), ("mc", mc), ("p", p)):
        got = got.float().cpu().numpy()
        print(f"{tag} {name}: max abs err {float(np.abs(got - g[name]).max()):.3e}")
        np.testing.assert_allclose(got, g[name], err_msg=name, **LAYER_TOL)
    for i, r in enumerate(raw):
        np.testing.assert_allclose(r.float().cpu().numpy(), g[f"raw{i}"], err_msg=f"raw{i}", **LAYER_TOL)
    ys, seen = [], 0
    for layer in m.model[:-1]:
        if layer.f != -1:
            x = ys[layer.f] if isinstance(layer.f, int) else [x if j == -1 else ys[j] for j in layer.f]
        x = layer(x)
        ys.append(x if layer.i in m.save else None)
        if torch.is_tensor(x):
            np.testing.assert_allclose(x.float().cpu().numpy(), g[f"layer{layer.i}"], err_msg=f"layer {layer.i} {layer.type}", **LAYER_TOL)
            seen += 1
    assert seen >= 15


@pytest.mark.parametrize("which,tag,base,shape", MODELS, ids=["yolo11n-seg", "edgeline-n-seg"])
def test_fp16_vs_reference_golden(golden_dir, which, tag, base, shape):
    """Throughput mode, the f16 rule of tests/test_gpu_model.py: scores within 2e-2, boxes within 1.5 % of the image size."""
    g = np.load(os.path.join(golden_dir, tag + ".npz"))
    m = _build(which, torch.float16)
    y, (raw, mc, p) = m(synth.synth_images(*shape).cuda().half())
    y = y.cpu().numpy()
    assert y.dtype == np.float32 and y.shape == g["y"].shape and mc.dtype == torch.float16 and p.dtype == torch.float16
    assert float(np.abs(y[:, 4:84] - g["y"][:, 4:84]).max()) < 2e-2
    assert float(np.abs(y[:, :4] - g["y"][:, :4]).max()) < 0.015 * max(shape[2:])
    assert tuple(p.shape) == g["p"].shape and bool(torch.isfinite(p).all()) and bool(torch.isfinite(mc).all())


def test_nms_with_mask_coefficients(golden_dir):
    from edge_yolo_amd.utils import ops as uops
    g = np.load(os.path.join(golden_dir, "seg_ops.npz"))
    pred = seg_synth.nms_pred().cuda()
    for conf, iou, key in ((0.25, 0.7, "nms_a"), (0.5, 0.45, "nms_b")):
        rows = uops.non_max_suppression(pred, conf, iou, nc=4, max_det=50)[0].cpu().numpy()
        assert rows.shape == g[key].shape == (50, 38)
        np.testing.assert_array_equal(rows, g[key])
    boxes, count, index = uops.nms_device(pred, 0.25, 0.7, nc=4, max_det=50)
    assert tuple(boxes.shape) == (1, 50, 38) and int(count[0]) == 50
    np.testing.assert_array_equal(boxes[0, :, 6:].cpu().numpy(), pred[0, 8:, index[0].long()].T.cpu().numpy())


@pytest.mark.parametrize("which,tag,base,shape", MODELS, ids=["yolo11n-seg", "edgeline-n-seg"])
def test_process_mask_on_the_golden(golden_dir, which, tag, base, shape):
    """utils.ops.process_mask on the reference's own p, NMS rows and boxes: the reference's bits under the derived criterion."""
    from edge_yolo_amd.utils import ops as uops
    g = np.load(os.path.join(golden_dir, tag + ".npz"))
    for i in range(shape[0]):
        det, p = g[f"det{i}"], g["p"][i]
        got = uops.process_mask(torch.tensor(p).cuda(), torch.tensor(det[:, 6:]).cuda(), torch.tensor(det[:, :4]).cuda(), shape[1:], upsample=True).cpu().numpy()
        assert got.shape == g[f"masks{i}"].shape and len(det) >= 5
        ref = f64.process_mask64(p, det[:, 6:], det[:, :4], 4)
        f64.check_bits(g[f"masks{i}"], ref, 32)
        und, tot = f64.check_bits(got, ref, 32)
        decided = np.abs(ref["v"]) > f64.mask_bound(ref, 32)
        np.testing.assert_array_equal(got[decided], g[f"masks{i}"][decided])
        print(f"{tag} image {i}: {len(det)} masks, undecided {und} of {tot}")


def _expected_masks(pred, x):
    """float64 masks from one eager device step's own outputs: p, per-level coefficient maps, index, count, boxes."""
    boxes, count, index, _, p, *mcs = pred._device_step(pred.preprocess(x))
    torch.cuda.synchronize()
    flat = torch.cat([m.float().flatten(2) for m in mcs], 2).permute(0, 2, 1).cpu().numpy()  # [B, A, nm]
    out = []
    for i in range(boxes.shape[0]):
        n = int(count[i])
        idx = index[i, :n].cpu().numpy()
        out.append((n, f64.process_mask64(p[i].float().cpu().numpy(), flat[i, idx], boxes[i, :n, :4].cpu().numpy(), 4) if n else None, boxes[i, :n].cpu().numpy()))
    return out


@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
def test_predict_masks_end_to_end(half):
    import edge_yolo_amd
    model = edge_yolo_amd.YOLO("yolo11n-seg.yaml")
    model.model.load_state_dict(seg_synth.state_dict(model.model.state_dict()))
    kept = 0
    for B in (1, 3):  # (the second call has another batch size: another captured graph, another launch size)
        x = synth.synth_images(B, 64, 96, seed=B)
        res = model.predict(x, conf=0.05, iou=0.7, half=half, device="cuda:0")
        assert len(res) == B
        want = _expected_masks(model.predictor, x)
        for r, (n, ref, rows) in zip(res, want):
            assert len(r) == n
            if n == 0:
                assert r.masks is None
                continue
            assert r.masks.data.dtype == torch.bool and tuple(r.masks.shape) == (n, 64, 96) and r.masks.orig_shape == (64, 96)
            np.testing.assert_array_equal(r.boxes.data.cpu().numpy()[:, 4:], rows[:, 4:])
            f64.check_bits(r.masks.data.cpu().numpy().astype(np.uint8), ref, 32)
            assert bool(r.masks.data.any())
            kept += n
    assert kept >= 5
    again = model.predict(synth.synth_images(1, 64, 96, seed=1), conf=0.05, iou=0.7, half=half, device="cuda:0")  # graph replay
    assert torch.equal(again[0].masks.data, model.predict(synth.synth_images(1, 64, 96, seed=1), conf=0.05, iou=0.7, half=half, device="cuda:0", graph=False)[0].masks.data)
    none = model.predict(synth.synth_images(2, 64, 96), conf=0.9999, device="cuda:0", half=half)
    assert all(len(r) == 0 and r.masks is None for r in none)
    with pytest.warns(UserWarning, match="augment"):
        aug = model.predict(synth.synth_images(1, 64, 96, seed=1), conf=0.05, iou=0.7, half=half, device="cuda:0", augment=True)
    assert torch.equal(aug[0].masks.data, again[0].masks.data)
