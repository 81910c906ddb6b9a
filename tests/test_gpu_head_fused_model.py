"""-m gpu: Detect.forward(nms=...) with the towers' closing 1x1 convs inside the decode kernel (tunable head_fuse = 1, 2) against the
separate launches (head_fuse = 0) on whole models: candidate buffers byte-equal, NMS rows / counts / anchor indices equal,
nms["keep_raw"] returns the raw maps, and a captured graph replays what eager execution computes."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import synthdata as synth  # noqa: E402

TAIL_BOX, TAIL_BOX_CLS = 3, 4  # EY_HD_TAIL_BOX, EY_HD_TAIL_BOX_CLS


def _model(name):
    import edge_yolo_amd  # noqa: F401
    from edge_yolo_amd.nn.tasks import DetectionModel
    m = DetectionModel(name)
    m.load_state_dict(synth.synth_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}))
    return m.cuda().fuse().half().eval()


def _views(c):
    """keys, class ids (the A anchor slots of each image) and boxes of a Candidates buffer, as raw integers."""
    B, A = c.B, c.A
    P = (A + 255) // 256 * 256
    keys = c.buf[:B * P * 8].view(torch.int64).view(B, P)[:, :A]
    cls_id = c.buf[B * P * 8:B * P * 12].view(torch.int32).view(B, P)[:, :A]
    box4 = c.buf[B * P * 12:B * P * 12 + B * 4 * A * 4].view(torch.int32).view(B, 4, A)
    return keys, cls_id, box4


def _set(fuse):
    from edge_yolo_amd import _lib as L
    L.check(L.lib().ey_tune_set(b"head_fuse", fuse), "ey_tune_set")


@pytest.mark.parametrize("name,B,H,W", [("yolo11n-test.yaml", 2, 64, 96), ("yolo11n-GF2Detect.yaml", 1, 64, 64)])
def test_model_fused_equals_unfused(name, B, H, W):
    from edge_yolo_amd import _lib as L
    from edge_yolo_amd.engine.predictor import GraphRunner
    from edge_yolo_amd.utils import ops
    m = _model(name)
    x = synth.synth_images(B, H, W).cuda().half()
    conf = 0.05
    default = int(L.lib().ey_tune_get(b"head_fuse"))
    assert default in (0, 1, 2)
    quality = 10 if m.model[-1]._quality_params(0, x.device) is not None else 0  # EY_HD_QUALITY
    try:
        _set(0)
        want, raws = m(x, head_nms={"conf": conf, "classes": None, "keep_pred": True})
        assert L.lib().ey_head_decode_last_variant() == 1 + quality + 100 and all(r is not None for r in raws)
        want_rows = ops.nms_device(want, conf, 0.6, max_det=100)
        for fuse in (1, 2):
            _set(fuse)
            got, none = m(x, head_nms={"conf": conf, "classes": None, "keep_pred": True})
            assert L.lib().ey_head_decode_last_variant() == (TAIL_BOX, TAIL_BOX_CLS)[fuse - 1] + quality + 100, f"head_fuse={fuse}: the fused kernel did not run"
            assert all(r is None for r in none)
            for part, a, b in zip(("keys", "cls_id", "box4"), _views(got), _views(want)):
                assert torch.equal(a, b), f"{name} head_fuse={fuse}: candidate {part} differ"
            assert torch.equal(got.pred, want.pred), f"{name} head_fuse={fuse}: pred differs"
            lean, _ = m(x, head_nms={"conf": conf, "classes": [0, 2, 5]})
            _set(0)
            lean0, _ = m(x, head_nms={"conf": conf, "classes": [0, 2, 5]})
            _set(fuse)
            for g, w in zip(ops.nms_device(got, conf, 0.6, max_det=100), want_rows):
                assert torch.equal(g, w), f"{name} head_fuse={fuse}: NMS results differ"
            for g, w in zip(ops.nms_device(lean, conf, 0.6, classes=[0, 2, 5], max_det=100), ops.nms_device(lean0, conf, 0.6, classes=[0, 2, 5], max_det=100)):
                assert torch.equal(g, w), f"{name} head_fuse={fuse}: NMS results differ (class filter, no pred)"
            # keep_raw: today's launches and the raw maps, whatever the tunable says
            kept, maps = m(x, head_nms={"conf": conf, "classes": None, "keep_pred": True, "keep_raw": True})
            assert L.lib().ey_head_decode_last_variant() == 1 + quality + 100
            assert all(torch.equal(a, b) for a, b in zip(maps, raws)) and torch.equal(kept.pred, want.pred)
            # captured graph == eager
            runner = GraphRunner(lambda im: ops.nms_device(m(im, head_nms={"conf": conf, "classes": None})[0], conf, 0.6, max_det=100))
            for _ in range(2):
                out = runner(x)
                for g, w in zip(out, want_rows):
                    assert torch.equal(g, w), f"{name} head_fuse={fuse}: graph replay differs from eager"
        print(f"[fused model] {name}: head_fuse 1 and 2 equal 0 ({int(want_rows[1].sum())} boxes); keep_raw and graph replay equal")
    finally:
        _set(default)
