"""Object tracking on the device (reference ultralytics/trackers): ByteTrack for a batch of independent streams, one HIP launch per frame."""
from .byte_tracker import DEFAULT_SETTINGS, BYTETracker, load_settings  # noqa: F401
