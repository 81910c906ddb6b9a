"""-m gpu: YOLO(...).track() on small synthetic-weight models.  The rows predict(x, conf=0.1) returns, pushed through the float64 restatement
(tests/fp64_track_ref.py) frame by frame, are what track(x, persist=True) must return; persist=False restarts the ids; the segment and pose
tasks carry the masks and keypoints of the tracked rows; an image without tracks keeps its untracked Results."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import fp64_track_ref as ref  # noqa: E402
import pose_synth  # noqa: E402
import seg_synth  # noqa: E402
import synthdata as synth  # noqa: E402


def _facade(name):
    import edge_yolo_amd
    model = edge_yolo_amd.YOLO(name)
    own = model.model.state_dict()
    sd = seg_synth.state_dict(own) if "seg" in name else pose_synth.state_dict(own) if "pose" in name else synth.synth_state_dict({k: tuple(v.shape) for k, v in own.items()})
    model.model.load_state_dict(sd)
    return model


def _frames(B, h, w, n):
    """n frames of B streams: each stream's image drifts by 2 px per frame."""
    x = synth.synth_images(B, h, w)
    return [torch.roll(x, shifts=(2 * f, 2 * f), dims=(2, 3)) for f in range(n)]


def _check(res, pred, want):
    """one image: tracked Results `res` against the untracked `pred` and the restatement's rows `want`."""
    if len(pred) == 0 or len(want) == 0:
        assert res.boxes.id is None and not res.boxes.is_track and res.boxes.data.shape == pred.boxes.data.shape
        return 0
    got = res.boxes.data.cpu().numpy()
    assert res.boxes.is_track and got.shape == (len(want), 7)
    np.testing.assert_array_equal(got[:, 4:], want[:, 4:7])  # id, conf, cls
    ulp = np.spacing(np.abs(want[:, :4]).max(1).astype(np.float32))[:, None]
    assert (np.abs(got[:, :4].astype(np.float64) - want[:, :4]) <= ulp).all()
    idx = want[:, 7].astype(np.int64)
    np.testing.assert_array_equal(res.boxes.conf.cpu().numpy(), pred.boxes.conf.cpu().numpy()[idx])
    np.testing.assert_array_equal(res.boxes.cls.cpu().numpy(), pred.boxes.cls.cpu().numpy()[idx])
    if pred.masks is not None:
        assert torch.equal(res.masks.data, pred.masks.data[torch.from_numpy(idx).to(pred.masks.data.device)])
    if pred.keypoints is not None:
        assert torch.equal(res.keypoints.data, pred.keypoints.data[torch.from_numpy(idx).to(pred.keypoints.data.device)])
    return len(want)


@pytest.mark.parametrize("name,hw", [("yolo11n-test.yaml", (128, 128)), ("yolo11n-seg.yaml", (64, 96)), ("yolo11n-pose.yaml", (64, 96))])
def test_track_equals_predict_through_restatement(name, hw):
    model = _facade(name)
    # agnostic NMS: the synthetic weights put several classes on one and the same box, and tracks with identical boxes make assignments
    # with many optima, which the kernel and scipy may resolve differently (divergences)
    B, kw = 2, dict(iou=0.7, agnostic_nms=True, device="cuda:0")
    trackers = [ref.RefTracker() for _ in range(B)]
    tracked = 0
    for f, x in enumerate(_frames(B, *hw, 5)):
        pred = model.predict(x, conf=0.1, **kw)
        res = model.track(x, persist=True, **kw)  # (conf defaults to 0.1)
        assert len(res) == B
        for i in range(B):
            rows = pred[i].boxes.data.float().cpu().numpy()
            want = trackers[i].update(rows)
            tracked += _check(res[i], pred[i], want)
    assert tracked >= 5, "the fixture tracks nothing"
    import track_synth as ts  # (the margins of this fixture's decisions, for the record)
    for t in trackers:
        print(name, ts.margins(t))
    # persist=False: new trackers, ids from 1, frame 1 (every track is output at once)
    x = _frames(B, *hw, 1)[0]
    fresh = model.track(x, **kw)
    pred = model.predict(x, conf=0.1, **kw)
    for i in range(B):
        want = ref.RefTracker().update(pred[i].boxes.data.float().cpu().numpy())
        _check(fresh[i], pred[i], want)
        if len(want):
            assert fresh[i].boxes.id.cpu().tolist() == list(range(1, len(want) + 1))
    # an image without detections keeps its untracked Results
    none = model.track(x, conf=0.9999, **kw)
    assert all(r.boxes.id is None and len(r) == 0 for r in none)


def test_track_settings_and_batch_size_restart_state():
    model = _facade("yolo11n-test.yaml")
    kw = dict(device="cuda:0", persist=True)
    x = synth.synth_images(2, 128, 128)
    a = model.track(x, **kw)
    b = model.track(x, **kw)  # second frame of the same streams: the frame-1 tracks are matched again
    assert all(sorted(q.boxes.id.tolist()) == sorted(p.boxes.id.tolist()) for p, q in zip(a, b) if p.boxes.is_track)
    t0 = model._tracker
    assert t0.state["hdr"][:, 0].tolist() == [2, 2]
    model.track(x, tracker={"track_buffer": 10}, **kw)
    assert model._tracker is not t0 and model._tracker.state["hdr"][:, 0].tolist() == [1, 1]
    t1 = model._tracker
    model.track(x[:1], tracker={"track_buffer": 10}, **kw)
    assert model._tracker is not t1 and model._tracker.streams == 1
    model.track(x[:1], tracker={"track_buffer": 10}, max_tracks=512, **kw)
    assert model._tracker.max_tracks == 512 and model._tracker.overflow == [0]
