"""ByteTrack (reference trackers/byte_tracker.py BYTETracker) whose whole state lives on the device: `streams` independent trackers advanced
by one ey_bytetrack_update launch per frame.  The reference keeps Python objects per track and matches with numpy, scipy
and lap on the host; nothing here leaves the device but what the caller reads."""
from pathlib import Path

import torch

from ..nn import _ops

# the reference's cfg/trackers/bytetrack.yaml values, stated here (frame_rate is 30, so max_time_lost = track_buffer)
DEFAULT_SETTINGS = {"tracker_type": "bytetrack", "track_high_thresh": 0.25, "track_low_thresh": 0.1, "new_track_thresh": 0.25, "track_buffer": 30,
                    "match_thresh": 0.8, "fuse_score": True}


def load_settings(tracker=None):
    """tracker: None (the defaults), a dict, or the path of a YAML file holding some of DEFAULT_SETTINGS' keys -> the complete settings dict.
    tracker_type 'botsort' raises NotImplementedError (its global motion compensation needs OpenCV, which this build does not have)."""
    if tracker is None:
        given = {}
    elif isinstance(tracker, dict):
        given = dict(tracker)
    elif isinstance(tracker, (str, Path)):
        import yaml
        with open(tracker, "r") as f:
            given = yaml.safe_load(f) or {}
        if not isinstance(given, dict):
            raise ValueError(f"tracker '{tracker}': expected a YAML mapping of tracker settings")
    else:
        raise TypeError(f"tracker=: expected None, a dict or a YAML path, got {type(tracker).__name__}")
    kind = given.get("tracker_type", "bytetrack")
    if kind == "botsort":
        raise NotImplementedError("tracker_type 'botsort': BoT-SORT's global motion compensation needs OpenCV and is not built; use 'bytetrack'")
    if kind != "bytetrack":
        raise ValueError(f"tracker_type '{kind}': only 'bytetrack' is built")
    unknown = sorted(set(given) - set(DEFAULT_SETTINGS))
    if unknown:
        raise ValueError(f"tracker settings {unknown} are not ByteTrack's ({sorted(DEFAULT_SETTINGS)})")
    s = {**DEFAULT_SETTINGS, **given}
    for k in ("track_high_thresh", "track_low_thresh", "new_track_thresh", "match_thresh"):
        s[k] = float(s[k])
    s["track_buffer"], s["fuse_score"] = int(s["track_buffer"]), bool(s["fuse_score"])
    return s


class BYTETracker:
    """`streams` ByteTrack trackers on `device`.  Each stream has `max_tracks` slots (fp64 mean and covariance, state, activated flag, id,
    score, cls, idx, frame, start frame, tracklet_len) plus its frame count, id counter and overflow counter; ids count per stream from 1.
    A slot freed by the unconfirmed round of a frame is free for the new tracks of the same frame, one freed by expiry or as a duplicate
    from the next frame on; with no free slot a new track is not started and `overflow` counts it."""

    def __init__(self, args=None, streams=1, max_det=300, max_tracks=1024, device=None):
        self.args = load_settings(args)
        self.streams, self.max_det, self.max_tracks = int(streams), int(max_det), int(max_tracks)
        if self.streams < 1 or self.max_det < 1 or self.max_tracks < 1:
            raise ValueError("BYTETracker: streams, max_det and max_tracks must be at least 1")
        self.device = torch.device("cuda:0" if device is None else device)
        self.state = _ops.bytetrack_state(self.streams, self.max_tracks, self.device)
        self._ws = None

    def update(self, rows, count):
        """rows: float32 (streams, max_det, 6) device tensor x1,y1,x2,y2,score,cls; count: int32 (streams,) -> (tracks (streams, max_det, 8) =
        x1,y1,x2,y2,id,score,cls,idx in ascending id, ids int32 (streams, max_det), counts int32 (streams,)); a stream whose count is 0 is
        left alone (no frame is counted, reference trackers/track.py:78-79)."""
        if tuple(rows.shape) != (self.streams, self.max_det, 6):
            raise ValueError(f"BYTETracker.update: rows must be ({self.streams}, {self.max_det}, 6), got {tuple(rows.shape)}")
        if self._ws is None:
            from .. import _lib as L
            self._ws = torch.empty(int(L.lib().ey_bytetrack_workspace_bytes(self.streams, self.max_det, self.max_tracks)), dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            return _ops.bytetrack_update(rows, count, self.state, self.args, workspace=self._ws)

    def reset(self, streams=None):
        """forget every track of the given streams (all by default); their ids start at 1 again."""
        sel = slice(None) if streams is None else torch.as_tensor(list(streams), dtype=torch.long, device=self.device)
        for t in self.state.values():
            t[sel] = 0

    @property
    def overflow(self):
        """per stream, how many new tracks were not started for want of a free slot."""
        return self.state["hdr"][:, 2].tolist()
