"""-m gpu: Masks.xy / xyn end to end.  YOLO("yolo11n-seg.yaml") with synthetic weights on the synthetic 64x96 input, and the same model
through RetinaMasksPredictor on images of two original shapes: the polygons of every result equal, exactly in float32, masks2segments'
post-processing of the restatement's contours (tests/contours_ref.py) of that result's own masks, pushed through scale_coords."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import contours_ref as ref  # noqa: E402
import retina_synth as rs  # noqa: E402
import seg_synth  # noqa: E402
import synthdata as synth  # noqa: E402


def _model():
    import edge_yolo_amd
    model = edge_yolo_amd.YOLO("yolo11n-seg.yaml")
    model.model.load_state_dict(seg_synth.state_dict(model.model.state_dict()))
    return model


def _check(results, shapes):
    """-> (masks, vertices) checked."""
    from edge_yolo_amd.utils import ops
    masks = vertices = 0
    for r, shape in zip(results, shapes):
        if r.masks is None:  # (nothing kept in this image; the callers assert that masks were traced at all)
            assert len(r) == 0
            continue
        assert len(r.masks) > 0 and tuple(r.masks.shape[1:]) == tuple(shape[0]) and r.masks.orig_shape == tuple(shape[1])
        data = r.masks.data.cpu().numpy().astype(np.uint8)
        xy, xyn = r.masks.xy, r.masks.xyn
        assert len(xy) == len(xyn) == len(r.masks) == len(r)
        assert torch.equal(r.masks.data.cpu(), torch.tensor(data).bool())  # (reading the polygons leaves the masks alone)
        for m, a, b in zip(data, xy, xyn):
            seg = ops._contours2segment(ref.find_contours(m))
            want = ops.scale_coords(m.shape, seg.copy(), r.masks.orig_shape, normalize=False)
            wantn = ops.scale_coords(m.shape, seg.copy(), r.masks.orig_shape, normalize=True)
            assert a.dtype == b.dtype == np.float32 and a.shape == want.shape and np.array_equal(a, want) and np.array_equal(b, wantn)
            assert (b >= 0).all() and (b <= 1).all()
            vertices += len(a)
        masks += len(r.masks)
    return masks, vertices


def test_predict_polygons():
    model = _model()
    res = model.predict(synth.synth_images(2, 64, 96, seed=3), conf=0.05, iou=0.7, half=False, device="cuda:0")
    masks, vertices = _check(res, [((64, 96), (64, 96))] * 2)
    print(f"{masks} masks, {vertices} vertices")
    assert masks >= 2 and vertices >= 8
    with pytest.raises(NotImplementedError, match="device"):
        res[0].masks.cpu().xy


def test_retina_polygons():
    from edge_yolo_amd.engine.predictor import RetinaMasksPredictor
    model = _model()
    r = np.random.default_rng(5)
    src = [r.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in rs.MODEL_SHAPES]
    res = model.predict(src, predictor=RetinaMasksPredictor, conf=0.02, iou=0.7, half=False, device="cuda:0", imgsz=96)
    masks, vertices = _check(res, [(s, s) for s in rs.MODEL_SHAPES])
    print(f"{masks} retina masks, {vertices} vertices")
    assert masks >= 2 and vertices >= 8
