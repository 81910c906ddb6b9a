"""Golden vectors for mask polygons, from the real reference imported through _ref_import: masks2segments (utils/ops.py:793-821, both
strategies), merge_multi_segment (data/converter.py:532-579) and Masks.xy / xyn (engine/results.py:1202-1251) on the synthetic masks of
tests/contours_synth.py.  cv2 is not installed: the one call the reference makes into it, cv2.findContours(x, RETR_EXTERNAL,
CHAIN_APPROX_SIMPLE), is set on the stand-in to the restatement of tests/contours_ref.py, returning OpenCV's (k, 1, 2) int32 arrays, so
everything around that call is the reference's own output and the call itself stays unpinned.

    python tests/golden/make_golden_contours.py

writes contours_ops.npz:
  * seg_all_<i> / seg_largest_<i>: masks2segments([case i], strategy)[0] for every case of contours_synth.cases();
  * merge<j>_n, merge<j>_in<k>, merge<j>_out: merge_multi_segment on lists of random integer segments, the pieces concatenated;
  * masks<j>_idx / _orig / _xy / _xyn / _len: Masks(stack of the cases idx, orig).xy and .xyn, concatenated, with their lengths.
Runs only where the reference exists.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]

import _ref_import  # noqa: E402

_ref_import.setup()

import numpy as np  # noqa: E402
import torch  # noqa: E402

import contours_ref as ref  # noqa: E402
import contours_synth as cs  # noqa: E402
import cv2  # noqa: E402  (the stand-in)
from ultralytics.data.converter import merge_multi_segment  # noqa: E402
from ultralytics.engine.results import Masks  # noqa: E402
from ultralytics.utils import ops as rops  # noqa: E402


def find_contours(x, mode, method):
    assert x.dtype == np.uint8 and x.ndim == 2
    return tuple(c.reshape(-1, 1, 2) for c in ref.find_contours(x)), None


cv2.findContours = find_contours

# (indices into contours_synth.cases() of one shape, orig_shape): the mask's own shape, a proportional one, and two that letterbox
MASK_SETS = (("blobs_64x96", (64, 96)), ("blobs_64x96", (128, 192)), ("blobs_64x96", (120, 200)), ("blobs_64x96", (50, 60)), ("noise_33x65", (70, 130)),
             ("c_", (16, 20)))


def mask_set(prefix):
    return [i for i, (name, _) in enumerate(cs.cases()) if name.startswith(prefix)]


if __name__ == "__main__":
    d = {}
    for i, (name, m) in enumerate(cs.cases()):
        for strategy in ("all", "largest"):
            seg = rops.masks2segments(torch.tensor(m.astype(np.float32))[None], strategy)
            assert len(seg) == 1 and seg[0].dtype == np.float32 and seg[0].ndim == 2 and seg[0].shape[1] == 2
            d[f"seg_{strategy}_{i}"] = seg[0]
        print(name, len(cs.expected(i)), d[f"seg_all_{i}"].shape, d[f"seg_largest_{i}"].shape)
    rng = np.random.default_rng(5)
    for j, n in enumerate((2, 3, 4, 5, 3, 6)):
        segs = [rng.integers(0, 40, (int(rng.integers(1, 9)), 2)).astype(np.int32) for _ in range(n)]
        d[f"merge{j}_n"] = np.int32(n)
        for k, s in enumerate(segs):
            d[f"merge{j}_in{k}"] = s
        d[f"merge{j}_out"] = np.concatenate(merge_multi_segment([s.copy() for s in segs]))
    for j, (prefix, orig) in enumerate(MASK_SETS):
        idx = mask_set(prefix)
        stack = torch.tensor(np.stack([cs.cases()[i][1] for i in idx]).astype(np.float32))
        xy, xyn = Masks(stack.clone(), orig).xy, Masks(stack.clone(), orig).xyn
        assert len(xy) == len(xyn) == len(idx)
        d[f"masks{j}_idx"], d[f"masks{j}_orig"] = np.asarray(idx, np.int32), np.asarray(orig, np.int32)
        d[f"masks{j}_len"] = np.asarray([len(a) for a in xy], np.int32)
        d[f"masks{j}_xy"], d[f"masks{j}_xyn"] = np.concatenate(xy), np.concatenate(xyn)
        assert d[f"masks{j}_xy"].dtype == np.float32 and d[f"masks{j}_len"].sum() > 0
        print(prefix, orig, d[f"masks{j}_len"])
    path = os.path.join(HERE, "contours_ops.npz")
    np.savez_compressed(path, **d)
    print("contours_ops", len(d), os.path.getsize(path))
    assert os.path.getsize(path) < 1 << 20
