"""The named masks of the contour tests, all tiny, fixed seeds: cases() -> list of (name, uint8 (h, w) mask); expected(i) -> the
restatement's contours of case i (computed once); by_shape() -> {(h, w): [case indices]} for batched calls."""
import functools

import numpy as np

import contours_ref as ref


def _m(rows):
    return np.array([[c in "#" for c in r] for r in rows], np.uint8)


def _blobs(h, w, seed):
    """blurred noise, thresholded: a few smooth blobs with holes."""
    from scipy import ndimage
    rng = np.random.default_rng(seed)
    f = ndimage.gaussian_filter(rng.standard_normal((h, w)), 3.0)
    return (f > 0.02).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def cases():
    out = [("empty_5x9", np.zeros((5, 9), np.uint8)), ("empty_1x1", np.zeros((1, 1), np.uint8))]
    for name, (y, x) in {"tl": (0, 0), "tr": (0, 8), "bl": (4, 0), "br": (4, 8), "interior": (2, 4)}.items():
        m = np.zeros((5, 9), np.uint8)
        m[y, x] = 1
        out.append((f"pixel_{name}", m))
    for h, w in ((1, 1), (1, 7), (7, 1), (5, 9)):
        out.append((f"ones_{h}x{w}", np.ones((h, w), np.uint8)))
    m = np.zeros((8, 10), np.uint8)
    m[2:6, 3:8] = 255  # (any non-zero value is set)
    out.append(("rectangle", m))
    m = np.zeros((5, 9), np.uint8); m[2, 1:8] = 1
    out.append(("line_h", m))
    m = np.zeros((9, 5), np.uint8); m[1:8, 2] = 1
    out.append(("line_v", m))
    out.append(("line_diag", np.eye(7, dtype=np.uint8)))
    out.append(("line_antidiag", np.eye(7, dtype=np.uint8)[::-1].copy()))
    out.append(("squares_touching", _m(["......", ".##...", ".##...", "...##.", "...##.", "......"])))
    out.append(("ring", _m([".......", ".#####.", ".#...#.", ".#...#.", ".#...#.", ".#####.", "......."])))
    out.append(("ring_island", _m([".......", ".#####.", ".#...#.", ".#.#.#.", ".#...#.", ".#####.", "......."])))
    out.append(("ring_thick_island", _m(["#########", "#########", "##.....##", "##.###.##", "##.###.##", "##.....##", "#########", "#########"])))
    out.append(("nested_twice", _m(["###########", "#.........#", "#.#######.#", "#.#.....#.#", "#.#.###.#.#", "#.#.#.#.#.#", "#.#.###.#.#", "#.#.....#.#",
                                    "#.#######.#", "#.........#", "###########"])))
    out.append(("c_right_blob", _m(["........", ".######.", ".#......", ".#..##..", ".#..##..", ".#......", ".######.", "........"])))
    out.append(("c_left_blob", _m(["........", ".######.", "......#.", "..##..#.", "..##..#.", "......#.", ".######.", "........"])))
    out.append(("spur", _m([".......", ".###...", ".###...", ".######", ".###...", ".###...", "......."])))
    out.append(("spur_up", _m(["...#...", "...#...", ".#####.", ".#####.", "......."])))
    out.append(("east_unexamined", EAST_UNEXAMINED[0]))
    yy, xx = np.mgrid[:9, :9]
    out.append(("checkerboard_9x9", ((yy + xx) % 2 == 0).astype(np.uint8)))
    for h, w in ((16, 16), (33, 65)):
        for p in (0.3, 0.5, 0.7, 0.9):
            rng = np.random.default_rng(1000 * h + int(100 * p))
            out.append((f"noise_{h}x{w}_p{p}", (rng.random((h, w)) < p).astype(np.uint8)))
    for seed in (0, 1, 2):
        out.append((f"blobs_64x96_{seed}", _blobs(64, 96, seed)))
    return out


# a pixel whose east neighbour is 0 but is not examined when the border passes: the left wall, one pixel thick, of a ring.  The outer
# border runs down the wall: it comes from N (2), the search for the next neighbour goes 3 = NW, 4 = W, 5 = SW and finds 6 = S, so east (the
# hole) is never reached and the label is 2, not -2.  That positive label is what tells the scan that it is inside a hole.
EAST_UNEXAMINED = (_m(["......", ".####.", ".#..#.", ".#..#.", ".#..#.", ".####.", "......"]), (3, 1))


@functools.lru_cache(maxsize=None)
def expected(i):
    return ref.find_contours(cases()[i][1])


def by_shape():
    d = {}
    for i, (_, m) in enumerate(cases()):
        d.setdefault(m.shape, []).append(i)
    return d


def same(got, want):
    """two lists of contours are the same integers in the same order."""
    return len(got) == len(want) and all(g.shape == w.shape and g.dtype == w.dtype and np.array_equal(g, w) for g, w in zip(got, want))


def decode(info, lens, verts):
    """one mask's raw outputs (info[4], lens[contour_cap], verts[vertex_cap][2]) -> its contours, last found first."""
    nc, nv = int(info[0]), int(info[1])
    assert nc <= len(lens) and nv <= len(verts) and int(np.sum(lens[:nc])) == nv
    off = np.concatenate([[0], np.cumsum(lens[:nc])])
    return [np.ascontiguousarray(verts[off[k]:off[k + 1]], np.int32) for k in range(nc - 1, -1, -1)]
