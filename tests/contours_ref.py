"""Restatement of cv2.findContours(mask, RETR_EXTERNAL, CHAIN_APPROX_SIMPLE) in plain numpy and Python: OpenCV's classical border following
(Suzuki & Abe 1985, algorithm 1, as OpenCV's findContours implements it), the definition ey_mask_contours is tested against (cv2 is not
installed where the suite runs; DESIGN.md 7s records what that leaves unpinned).  And checks of what such a result must satisfy that do
not depend on the restatement: the contour count against scipy's labelling of the hole-filled mask, the raster-first start of each
contour, the descending order of the starts, and the re-expanded 8-connected chain, filled, against the hole-filled component."""
import numpy as np

# directions counter-clockwise from east: 0=E 1=NE 2=N 3=NW 4=W 5=SW 6=S 7=SE, as (dy, dx)
DIRS = ((0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1), (1, 0), (1, 1))


def find_contours(mask, return_labels=False):
    """-> list of (k, 2) int32 arrays of (x, y), last found first.  return_labels: also the (h, w) label plane after the scan."""
    mask = np.asarray(mask)
    h, w = mask.shape
    lab = np.zeros((h + 2, w + 2), np.int32)  # everything outside the mask is 0
    lab[1:-1, 1:-1] = mask != 0
    found = []
    for y in range(1, h + 1):
        prev, lx = 0, 0  # lx: column 0 is the frame, label 0
        for x in range(1, w + 1):
            p = int(lab[y, x])
            if p == prev:
                continue
            if prev == 0 and p == 1 and not lab[y, lx] > 0:
                found.append(_trace(lab, y, x))
            p = int(lab[y, x])
            prev = p
            if p not in (0, 1):
                lx = x
    out = [np.asarray(c, np.int32).reshape(-1, 2) - 1 for c in reversed(found)]
    return (out, lab[1:-1, 1:-1].copy()) if return_labels else out


def _trace(lab, y0, x0):
    pts = []
    i0 = (y0, x0)
    s, i1 = 4, None
    while True:
        s = (s - 1) & 7
        q = (y0 + DIRS[s][0], x0 + DIRS[s][1])
        if lab[q] != 0:
            i1 = q
            break
        if s == 4:
            break
    if i1 is None:
        lab[i0] = -2
        return [(x0, y0)]
    i3, prev_s = i0, s ^ 4
    bound = 8 * lab.size + 8
    for _ in range(bound):
        s_end = s
        while True:
            s += 1
            i4 = (i3[0] + DIRS[s & 7][0], i3[1] + DIRS[s & 7][1])
            if lab[i4] != 0:
                break
            assert s < s_end + 8
        s &= 7
        if ((s - 1) & 0xFFFFFFFF) < s_end:
            lab[i3] = -2
        elif lab[i3] == 1:
            lab[i3] = 2
        if s != prev_s:
            pts.append((i3[1], i3[0]))
            prev_s = s
        if i4 == i0 and i3 == i1:
            return pts
        i3 = i4
        s = (s + 4) & 7
    raise AssertionError("border following did not end")


# ------------------------------------------------------------------------------------------------------------------------------------
# properties that do not depend on the restatement

def filled_components(mask):
    """(labels, count) of the 8-connected components of the hole-filled mask: one per external contour."""
    from scipy import ndimage
    return ndimage.label(ndimage.binary_fill_holes(np.asarray(mask) != 0), structure=np.ones((3, 3)))


def expand_chain(c):
    """the vertices of a CHAIN_APPROX_SIMPLE contour -> every pixel of the closed 8-connected chain (consecutive vertices lie on a
    horizontal, vertical or diagonal line)."""
    px = []
    for a, b in zip(c, np.roll(c, -1, axis=0)):
        d = b - a
        n = int(np.abs(d).max())
        assert n == 0 or (abs(int(d[0])) in (0, n) and abs(int(d[1])) in (0, n)), (a, b)
        step = d // max(n, 1)
        px += [a + k * step for k in range(max(n, 1))]
    return np.asarray(px)


def check_properties(mask, contours):
    """count, raster-first starts in descending order, and chain + fill == the hole-filled component, for every contour."""
    from scipy import ndimage
    mask = np.asarray(mask) != 0
    lab, n = filled_components(mask)
    assert len(contours) == n, (len(contours), n)
    starts = []
    for c in contours:
        assert c.dtype == np.int32 and c.ndim == 2 and c.shape[1] == 2 and len(c) >= 1
        x, y = int(c[0, 0]), int(c[0, 1])
        k = int(lab[y, x])
        assert k > 0
        ys, xs = np.nonzero(lab == k)
        assert (y, x) == (int(ys[0]), int(xs[ys == ys[0]].min())), "a contour starts at the raster-first pixel of its component"
        starts.append(y * mask.shape[1] + x)
        chain = expand_chain(c)
        assert mask[chain[:, 1], chain[:, 0]].all()
        border = np.zeros_like(mask)
        border[chain[:, 1], chain[:, 0]] = True
        np.testing.assert_array_equal(ndimage.binary_fill_holes(border), lab == k)
    assert starts == sorted(starts, reverse=True) and len(set(starts)) == len(starts)
