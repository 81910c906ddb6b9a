"""Segment utilities of the reference's ultralytics/data/converter.py that results need: `min_index` (:517-529) and `merge_multi_segment`
(:532-579), restated.  Host numpy: the data is a few hundred points per mask."""
import numpy as np

__all__ = ("min_index", "merge_multi_segment")


def min_index(arr1, arr2):
    """(i, j): the points arr1[i], arr2[j] of two (N, 2) / (M, 2) arrays with the shortest distance (the first such pair in row-major order)."""
    dis = ((arr1[:, None, :] - arr2[None, :, :]) ** 2).sum(-1)
    return np.unravel_index(np.argmin(dis, axis=None), dis.shape)


def merge_multi_segment(segments):
    """Several segments -> a list of pieces that, concatenated, is one closed line through all of them: neighbouring segments are joined
    at their closest points by a thin line that is walked forth (first round) and back (second round)."""
    s = []
    segments = [np.array(i).reshape(-1, 2) for i in segments]
    idx_list = [[] for _ in range(len(segments))]
    for i in range(1, len(segments)):  # the closest pair of points between each segment and the next
        idx1, idx2 = min_index(segments[i - 1], segments[i])
        idx_list[i - 1].append(idx1)
        idx_list[i].append(idx2)
    for k in range(2):
        if k == 0:  # forth
            for i, idx in enumerate(idx_list):
                if len(idx) == 2 and idx[0] > idx[1]:  # a middle segment has two joints: walk it from the lower one
                    idx = idx[::-1]
                    segments[i] = segments[i][::-1, :]
                segments[i] = np.roll(segments[i], -idx[0], axis=0)
                segments[i] = np.concatenate([segments[i], segments[i][:1]])
                if i in {0, len(idx_list) - 1}:  # the first and the last segment are walked whole
                    s.append(segments[i])
                else:
                    idx = [0, idx[1] - idx[0]]
                    s.append(segments[i][idx[0]:idx[1] + 1])
        else:  # back: the rest of every middle segment
            for i in range(len(idx_list) - 1, -1, -1):
                if i not in {0, len(idx_list) - 1}:
                    idx = idx_list[i]
                    nidx = abs(idx[1] - idx[0])
                    s.append(segments[i][nidx:])
    return s
