"""Edge cases of the selection kernels (csrc/head_nms.hip: ey_nms, ey_e2e_topk; csrc/nms_fast.inc.h), shared by
tests/test_nms_edges_cpu.py (the oracle's own answers must satisfy each case's conditions, so that no case silently becomes vacuous) and
by the -m gpu files test_gpu_nms_edges.py / test_gpu_e2e_topk_exact.py (kernel == oracle, bit for bit).  Everything is drawn from seeded
generators keyed by the case name.

An NMS case is `Case(pred, kw, variants, check, quiet)`: the oracle / the kernel run once per entry of `variants` (keyword overrides on
`kw`), and `check(results)` asserts the case's conditions on the oracle's `[(rows per image, anchor indices per image), ...]`.
A top-k case is `TopkCase(pred, ks, check)` with `check(k, rows, index)` on `topk_ref`'s answer."""
import collections
import functools
import zlib

import numpy as np

from oracle import nms as onms

F32 = np.float32
NF_KMAX = 2048  # csrc/nms_fast.inc.h: the most candidates the fast path selects; max_nms below it switches the fast path off
NMS_CAP = 4096  # csrc/head_nms.hip: the most keys one chunk of the radix descent takes
DEFAULTS = dict(conf_thres=0.25, iou_thres=0.45, classes=None, agnostic=False, multi_label=False, max_det=300, max_nms=30000, max_wh=7680.0)

Case = collections.namedtuple("Case", "pred kw variants check quiet")
TopkCase = collections.namedtuple("TopkCase", "pred ks check")


def _rng(tag, seed=0):
    return np.random.default_rng([zlib.crc32(tag.encode()), seed])


def full_kw(case, variant):
    return {**DEFAULTS, **case.kw, **variant}


def fast_eligible(kw, nc):
    """nms_select_launch: the predict-mode fast path runs for single-label calls with max_det <= 1024 and max_nms >= NF_KMAX."""
    return not (kw["multi_label"] and nc > 1) and kw["max_det"] <= 1024 and kw["max_nms"] >= NF_KMAX


def fast_meta(raw, B, A):
    """(n_sel, n_total, done) per image from the bytes of ey_nms's workspace (layout: nms_fast.inc.h, nf_image_bytes / nf_meta)."""
    P = (A + 255) // 256 * 256
    keys_bytes = (B * P * 12 + 255) // 256 * 256
    ntiles = (NF_KMAX // 64) * (NF_KMAX // 64 + 1) // 2
    img = (NF_KMAX * 28 + ntiles * 512 + 16 + 255) // 256 * 256
    out = []
    for b in range(B):
        off = keys_bytes + b * img + NF_KMAX * 28 + ntiles * 512
        out.append(tuple(int(v) for v in raw[off:off + 12].view(np.int32)))
    return out


def clustered(rng, B, nc, A, nclusters, sigma, size, lo=0.26, hi=0.99, one_class=False):
    """Boxes scattered (sigma) around `nclusters` centres, log-normal sizes around `size`, one scored class per anchor (a cluster holds
    two classes)."""
    pred = np.zeros((B, 4 + nc, A), F32)
    for b in range(B):
        centres = rng.uniform(40, 600, (nclusters, 2))
        which = rng.integers(0, nclusters, A)
        pred[b, 0:2] = (centres[which] + rng.normal(0, sigma, (A, 2))).T
        pred[b, 2:4] = rng.lognormal(np.log(size), 0.25, (2, A))
        cls = np.zeros(A, np.int64) if one_class else (which * 7 + rng.integers(0, 2, A)) % nc
        pred[b, 4 + cls, np.arange(A)] = rng.uniform(lo, hi, A)
    return pred


def run_oracle(case):
    """[(rows per image, anchor indices per image)] per variant."""
    out = []
    for v in case.variants:
        with np.errstate(all="ignore" if case.quiet else "warn"):
            out.append(onms.non_max_suppression(case.pred, **full_kw(case, v), return_idx=True))
    return out


def _counts(results, b=0):
    return [int(r[0][b].shape[0]) for r in results]


def _differ(ra, rb):
    return any(a.shape != b.shape or not np.array_equal(a, b, equal_nan=True) for a, b in zip(ra[0], rb[0]))


# ------------------------------------------------------------------------------------------------------------------------ ey_nms
MAX_NMS_LIST = (1, 100, 1000, 2047, 2048, 2049, 3000)


def _max_nms_single(max_det):
    """Every one of the 4096 anchors is a candidate, so each max_nms of the list cuts the sorted list somewhere else: below NF_KMAX only
    the general kernel's `processed + n > max_nms` cut runs, from NF_KMAX up (max_det <= 1024) the fast path's `nsel >= max_nms`."""
    def build():
        pred = clustered(_rng("max_nms_single"), 1, 4, 4096, 100, 4.0, 40.0)
        kw = dict(conf_thres=0.25, iou_thres=0.6, max_det=max_det)

        def check(results):
            counts = _counts(results)
            assert int((pred[0, 4:].max(0) > F32(0.25)).sum()) == 4096
            assert len(set(counts)) >= 4, counts
            assert counts == sorted(counts), counts
            assert any(m >= NF_KMAX and n < max_det for m, n in zip(MAX_NMS_LIST, counts)), counts  # the cap, not max_det, ends the image
            assert counts[-1] > counts[MAX_NMS_LIST.index(2049)], counts  # ... and it still bites above NF_KMAX
        return Case(pred, kw, [dict(max_nms=m) for m in MAX_NMS_LIST], check, False)
    return build


def _ml_pred():
    """Six tight clusters on a diagonal, 100 apart in x and in y, ~4.5 labels per anchor: with max_wh = 100 the class offsets (0, 200, 500
    for the classes 0, 2, 5) put boxes of different classes and clusters on top of each other, with 7680 they never meet."""
    rng = _rng("multi_label")
    A = 1500
    pred = np.zeros((1, 4 + 6, A), F32)
    which = rng.integers(0, 6, A)
    pred[0, 0:2] = (60.0 + 100.0 * which + rng.normal(0, 3.0, (2, A)))
    pred[0, 2:4] = rng.lognormal(np.log(50.0), 0.25, (2, A))
    pred[0, 4:] = rng.uniform(0.002, 0.9, (6, A)) * (rng.random((6, A)) < 0.75)
    return pred


def _max_nms_multi_label():
    pred = _ml_pred()
    kw = dict(conf_thres=0.001, iou_thres=0.6, multi_label=True, max_det=1000)

    def check(results):
        ncand = int((pred[0, 4:] > F32(0.001)).sum())
        counts = _counts(results)
        assert 4000 < ncand < 30000, ncand
        assert counts[0] < counts[1] < counts[2] < 1000, counts  # both caps cut, and cut differently; the uncapped run sees every pair
        assert np.bincount(results[2][1][0]).max() > 1  # some anchor is kept under two labels
    return Case(pred, kw, [dict(max_nms=m) for m in (500, 4000, 30000)], check, False)


def _multi_label_filter():
    pred = _ml_pred()
    kw = dict(conf_thres=0.001, iou_thres=0.6, multi_label=True, max_det=300, classes=[0, 2, 5])
    variants = [dict(agnostic=a, max_wh=w) for a in (False, True) for w in (100.0, 7680.0)]

    def check(results):
        for rows, _ in results:
            assert rows[0].shape[0] > 20 and set(np.unique(rows[0][:, 5]).tolist()) == {0.0, 2.0, 5.0}
        assert _differ(results[0], results[1])      # per class: at max_wh = 100 boxes of different classes overlap after the offset
        assert not _differ(results[2], results[3])  # agnostic: max_wh is not used
        assert _differ(results[1], results[3])
    return Case(pred, kw, variants, check, False)


def _scalar_score(A):
    def build():
        assert A % 4 != 0  # nms_run: the vector score kernel needs A % 4 == 0; these go through nms_score_kernel
        pred = clustered(_rng(f"scalar_score{A}"), 2, 6, A, max(8, A // 20), 5.0, 40.0, lo=0.05)
        pred[:, 4:] = np.maximum(pred[:, 4:], _rng(f"scalar_score{A}", 1).uniform(0.0, 0.04, pred[:, 4:].shape).astype(F32))
        pred[:, :4, A - 1] = np.asarray([3000.0, 300.0, 40.0, 40.0], F32)[None]  # the last anchor, alone out there: always kept
        pred[:, 4:, A - 1] = 0.0
        pred[:, 4 + 1, A - 1] = 0.995
        kw = dict(conf_thres=0.25, iou_thres=0.6, max_det=300)

        def check(results):
            for b in range(2):
                assert _counts(results, b)[0] > 5 and _counts(results, b)[1] > 2
                assert set(np.unique(results[1][0][b][:, 5]).tolist()) <= {1.0, 4.0}
                assert A - 1 in results[0][1][b] and A - 1 in results[1][1][b]  # the last, partly filled block of the score kernel's grid counts
            assert _differ(results[0], results[1])
        return Case(pred, kw, [dict(classes=None), dict(classes=[1, 4])], check, False)
    return build


DEGENERATE_KINDS = ("zero_w", "zero_h", "neg_w", "huge", "nan_cx", "inf_w")


def _degenerate(nc, nclusters, ndeg, late):
    """Boxes the IoU code treats apart: iou_gt's NaN branch, nf_mask_kernel's `sane` ballot (areas outside (1e-30, 1e30) -> the exact
    division), the partitioned greedy's NaN / extent fallback.  None of them overlaps anything by the reference's arithmetic, so all are
    kept; a handful of exact duplicates with a denormal area (1e-40) have IoU exactly 1 and must collapse to one, while a partly overlapping
    pair of the same size must not.
    late: the non-finite kinds score below everything else, so the general kernel's first chunks of ~512 candidates hold finite boxes
    only (16 classes, ~32 candidates per owner wave: the class-partitioned greedy may run) and its last chunk brings the fallback."""
    def build():
        rng = _rng(f"degenerate{nc}")
        A = 1200
        pred = clustered(rng, 1, nc, A, nclusters, 5.0, 40.0)
        kind = np.full(A, -1)
        sel = rng.permutation(A)[:ndeg]
        kind[sel] = np.arange(ndeg) % len(DEGENERATE_KINDS)
        if late:
            nonfinite = np.isin(kind, (3, 4, 5))[None, :] & (pred[0, 4:] > 0)
            pred[0, 4:] = np.where(nonfinite, rng.uniform(0.26, 0.30, pred[0, 4:].shape), np.where(pred[0, 4:] > 0, np.maximum(pred[0, 4:], 0.32), 0.0))
        with np.errstate(all="ignore"):
            pred[0, 2, kind == 0] = 0.0
            pred[0, 3, kind == 1] = 0.0
            pred[0, 2, kind == 2] *= -1.0
            pred[0, 2:4, kind == 3] = 3e19
            pred[0, 0, kind == 4] = np.nan
            pred[0, 2, kind == 5] = np.inf
        tiny = np.nonzero(kind == -1)[0][:6]
        kind[tiny] = 100
        pred[0, :, tiny] = 0.0
        pred[0, 2:4, tiny] = 1e-20
        pred[0, 4, tiny] = np.linspace(0.98, 0.93, 6, dtype=F32)
        # ... and two such boxes shifted by 0.3 of their width (IoU 0.54 < iou_thres, union 1.3e-40): both stay.  The reciprocal of that
        # union is not representable, so a pre-test on inter * rcp(union) would call it an overlap
        pair = np.nonzero(kind == -1)[0][:2]
        kind[pair] = 101
        pred[0, :, pair] = 0.0
        pred[0, 0, pair] = np.asarray([1e-18, 1e-18 + 3e-21], F32)
        pred[0, 2:4, pair] = 1e-20
        pred[0, 4, pair] = np.asarray([0.925, 0.92], F32)
        kw = dict(conf_thres=0.25, iou_thres=0.6)
        # max_det = 512: the class-partitioned greedy is eligible (and, unless `late`, the list is cut); 1024: every survivor is returned
        variants = [dict(agnostic=a, max_det=m) for a in (False, True) for m in (512, 1024)]

        def check(results):
            nordinary = int((kind == -1).sum())
            if late:
                s, bad = pred[0, 4:].max(0), np.isin(kind, (3, 4, 5))
                assert s[bad].max() < 0.31 < s[~bad].min()
                assert (~bad).sum() > 1024  # two clean chunks before the first non-finite box
            for v, (rows, idx) in zip(variants, results):
                k = kind[idx[0]]
                for q in range(len(DEGENERATE_KINDS)):
                    assert (k == q).sum() > 0, (v, DEGENERATE_KINDS[q])
                assert (k == 100).sum() == 1 and tiny[0] in idx[0], v
                assert (k == 101).sum() == 2, v
                if v["max_det"] == 1024 or late:
                    assert rows[0].shape[0] < v["max_det"]
                    assert (k >= 0).sum() == ndeg + 1 + 2, v  # every degenerate box is kept
                    assert (k == -1).sum() * 3 <= nordinary * 2, ((k == -1).sum(), nordinary)  # at least a third of the ordinary ones go
                else:
                    assert rows[0].shape[0] == 512
        return Case(pred, kw, variants, check, True)
    return build


def _iou_thres():
    """60 groups of {box, exact duplicate, edge-touching neighbour (intersection 0), partner shifted by 12 of 40 (IoU 0.54)} and 20 pairs
    of 400 x 400 boxes of different classes sharing a 0.25 x 0.25 corner (IoU 2e-7: an overlap at iou_thres 0.0, none at 5e-7; 7680
    apart in per-class NMS).  Integer / quarter coordinates: exact in fp32 with and without the class offset."""
    rng = _rng("iou_thres")
    rows = []
    for g in range(60):
        cx, cy, c = 100.0 + 120.0 * (g % 10), 100.0 + 100.0 * (g // 10), g % 2
        s = rng.uniform(0.5, 0.9)
        rows += [(cx, cy, 40.0, 40.0, s, c), (cx, cy, 40.0, 40.0, s - 0.05, c), (cx + 40.0, cy, 40.0, 40.0, s - 0.1, c), (cx + 12.0, cy, 40.0, 40.0, s - 0.15, c)]
    for g in range(20):
        x, y = 450.0 + 900.0 * (g % 6), 1400.0 + 900.0 * (g // 6)
        s = rng.uniform(0.5, 0.9)
        rows += [(x, y, 400.0, 400.0, s, 0), (x + 399.75, y + 399.75, 400.0, 400.0, s - 0.2, 1)]
    order = rng.permutation(len(rows))
    pred = np.zeros((1, 4 + 2, len(rows)), F32)
    for dst, src in enumerate(order):
        r = rows[src]
        pred[0, :4, dst] = r[:4]
        pred[0, 4 + r[5], dst] = r[4]
    kw = dict(conf_thres=0.25, max_det=1024)
    variants = [dict(iou_thres=t, agnostic=a) for a in (False, True) for t in (0.0, 5e-7, 1.0)]
    src_of = np.asarray(order)

    def check(results):
        npass = int((pred[0, 4:].max(0) > F32(0.25)).sum())
        assert npass == len(rows)
        for v, (out, idx) in zip(variants, results):
            kept = set(src_of[idx[0]].tolist())
            if v["iou_thres"] == 1.0:
                assert len(kept) == npass, v  # IoU never exceeds 1.0: duplicates included
                continue
            for g in range(60):
                assert 4 * g in kept and 4 * g + 2 in kept and 4 * g + 1 not in kept and 4 * g + 3 not in kept, (v, g)  # touching stays
        for a in (0, 3):  # per class the corner pairs are 7680 apart; agnostic they overlap by 3e-8
            n0, n1 = _counts(results)[a], _counts(results)[a + 1]
            assert (n1 - n0) == (0 if a == 0 else 20), (a, n0, n1)
    return Case(pred, kw, variants, check, False)


def _conf_thres():
    """Strict `>`: scores of exactly 0.0 do not pass conf 0.0 (denormal ones do), scores of exactly 1.0 do not pass conf 1.0."""
    rng = _rng("conf_thres")
    A = 501
    pred = clustered(rng, 1, 3, A, 60, 4.0, 30.0, lo=0.01)
    zero = np.arange(A) % 3 == 0
    pred[0, 4:, zero] = 0.0
    one = np.arange(A) % 7 == 1
    pred[0, 4:, one] = np.where(pred[0, 4:, one] > 0, F32(1.0), F32(0.0))
    den = np.nonzero(~zero & ~one)[0][:5]
    pred[0, 0, den] = 3000.0 + 100.0 * np.arange(5)  # far from everything: never suppressed
    pred[0, 4:, den] = 0.0
    pred[0, 4 + 1, den] = 1e-40
    kw = dict(iou_thres=0.6, max_det=1024)

    def check(results):
        (rows0, idx0), (rows1, _) = results
        assert rows1[0].shape[0] == 0 and int((pred[0, 4:] == 1.0).sum()) > 30
        assert rows0[0].shape[0] > 100 and not zero[idx0[0]].any() and zero.sum() > 100
        assert set(den.tolist()) <= set(idx0[0].tolist()) and (rows0[0][:, 4] < 1e-38).sum() == 5
        assert rows0[0].shape[0] < 1024
    return Case(pred, kw, [dict(conf_thres=0.0), dict(conf_thres=1.0)], check, False)


def _mixed_batch():
    """One launch, four regimes: nothing passes | more than max_det survivors | five candidates | a tie group larger than NF_KMAX, which
    the fast path's threshold select cannot split (it takes the 100 keys above it and leaves the image to the general kernel)."""
    rng = _rng("mixed_batch")
    A, nc = 4096, 2
    pred = np.zeros((4, 4 + nc, A), F32)
    pred[:, 0:2] = rng.uniform(0, 640, (4, 2, A))
    pred[:, 2:4] = 30.0
    pred[0, 4:] = rng.uniform(0.0, 0.2, (nc, A))
    pred[1, 0] = 20.0 + 40.0 * (np.arange(A) % 64)  # a grid of disjoint boxes: everything survives
    pred[1, 1] = 20.0 + 40.0 * (np.arange(A) // 64)
    pred[1, 4 + np.arange(A) % 2, np.arange(A)] = rng.uniform(0.26, 0.99, A)
    pred[2, 4:] = rng.uniform(0.0, 0.2, (nc, A))
    five = rng.permutation(A)[:5]
    pred[2, 0, five] = 100.0 + 100.0 * np.arange(5)
    pred[2, 4, five] = rng.uniform(0.5, 0.9, 5)
    pred[3, 4, :100] = rng.uniform(0.6, 0.9, 100)
    pred[3, 4, 100:3100] = 0.5
    pred[3, 5, 3100:] = rng.uniform(0.26, 0.45, A - 3100)
    kw = dict(conf_thres=0.25, iou_thres=0.5, max_det=300)

    def check(results):
        rows, idx = results[0]
        assert [r.shape[0] for r in rows[:3]] == [0, 300, 5] and rows[3].shape[0] > 100
        assert int((rows[3][:, 4] == F32(0.5)).sum()) > 50  # the tie group is reached and contributes rows
        tie = idx[3][rows[3][:, 4] == F32(0.5)]
        assert (np.diff(tie) > 0).all()
    return Case(pred, kw, [dict()], check, False)


MAX_DET_LIST = (1, 512, 513, 1024, 1025, 1500)


def _max_det():
    """512 / 513: chunk cap 1024 -> 4096 and the class partition off; 1024 / 1025: the fast path off.  More than 1500 boxes survive, so
    every run is cut by max_det."""
    pred = clustered(_rng("max_det"), 1, 4, 4096, 3000, 2.0, 7.0)
    kw = dict(conf_thres=0.25, iou_thres=0.6)

    def check(results):
        assert _counts(results) == list(MAX_DET_LIST), _counts(results)
        full = results[-1]
        for (rows, idx), m in zip(results, MAX_DET_LIST):
            np.testing.assert_array_equal(idx[0], full[1][0][:m])
    return Case(pred, kw, [dict(max_det=m) for m in MAX_DET_LIST], check, False)


def _nc252():
    """The YOLO-World limit: class offsets up to 251 * 7680 = 1.9e6, where fp32 coordinates step by 0.125, and 16 classes per owner wave
    of the partitioned greedy."""
    pred = clustered(_rng("nc252"), 2, 252, 2000, 30, 3.0, 50.0)
    kw = dict(conf_thres=0.25, iou_thres=0.6, max_det=300)

    def check(results):
        for b in range(2):
            n = _counts(results, b)
            assert n[0] > 50 and n[1] > 20 and n[0] > n[1], n
            assert (results[0][0][b][:, 5] >= 200).sum() > 5
            assert len(np.unique(results[0][0][b][:, 5])) > 40
    return Case(pred, kw, [dict(agnostic=False), dict(agnostic=True)], check, False)


NMS_CASES = {
    "max_nms_det1024": _max_nms_single(1024), "max_nms_det1500": _max_nms_single(1500), "max_nms_multi_label": _max_nms_multi_label,
    "multi_label_filter": _multi_label_filter, "scalar_score_315": _scalar_score(315), "scalar_score_1001": _scalar_score(1001),
    "scalar_score_8399": _scalar_score(8399), "degenerate_nc3": _degenerate(3, 30, 480, False), "degenerate_nc16": _degenerate(16, 12, 180, True), "iou_thres": _iou_thres,
    "conf_thres": _conf_thres, "mixed_batch": _mixed_batch, "max_det": _max_det, "nc252": _nc252,
}


@functools.lru_cache(maxsize=None)
def nms_reference(name):
    """(case, the oracle's results per variant): computed once per process, shared by every test that needs it; do not modify."""
    case = NMS_CASES[name]()
    return case, run_oracle(case)


# ------------------------------------------------------------------------------------------------------------------------ ey_e2e_topk
def topk_ref(pred, k):
    """Detect.postprocess with the documented tie rule (include/edgeyolo_hip.h: "equal scores: lower anchor, then lower class first"):
    per image the first k (anchor, class) pairs by (score descending, pair index a*nc+c ascending).
    pred (B, 4+nc, A) fp32 with x1y1x2y2 rows -> (rows (B, k, 6) fp32 = [x1,y1,x2,y2,score,class], anchor_index (B, k) int32)."""
    pred = np.asarray(pred, F32)
    B, no, A = pred.shape
    nc = no - 4
    rows = np.zeros((B, k, 6), F32)
    index = np.zeros((B, k), np.int32)
    for b in range(B):
        s = pred[b, 4:].T.reshape(-1)  # pair index a*nc+c
        order = np.lexsort((np.arange(A * nc), -s.astype(np.float64)))[:k]
        a, c = order // nc, order % nc
        rows[b, :, :4] = pred[b, :4, a]
        rows[b, :, 4] = s[order]
        rows[b, :, 5] = c
        index[b] = a
    return rows, index


def _boxes(rng, B, A):
    xy = rng.uniform(0, 600, (B, 2, A))
    return np.concatenate([xy, xy + rng.uniform(2, 60, (B, 2, A))], 1).astype(F32)


def _distinct(rng, n, lo, hi):
    """n distinct fp32 values in [lo, hi), in random order."""
    b0, b1 = int(np.asarray(lo, F32).view(np.uint32)), int(np.asarray(hi, F32).view(np.uint32))
    return (b0 + rng.choice(b1 - b0, n, replace=False)).astype(np.uint32).view(F32)


def _top_digit(s):
    return np.asarray(s, F32).view(np.uint32) >> 19  # the first 12-bit digit of the 64-bit key (score bits << 32)


def _topk_tie_free(B, nc, A, ks):
    def build():
        rng = _rng(f"topk_tie_free{nc}x{A}")
        pred = np.zeros((B, 4 + nc, A), F32)
        pred[:, :4] = _boxes(rng, B, A)
        for b in range(B):
            pred[b, 4:] = _distinct(rng, nc * A, 0.001, 0.999).reshape(nc, A)

        def check(k, rows, index):
            for b in range(B):
                assert len(np.unique(pred[b, 4:])) == nc * A
                assert (np.diff(rows[b, :, 4]) < 0).all()
        return TopkCase(pred, ks, check)
    return build


def _heavy_pred(tag, one_score):
    rng = _rng(tag)
    nc, A = 8, 1024
    s = np.empty(nc * A, F32)
    s[:300] = _distinct(rng, 300, 0.6, 0.9)
    s[300:6300] = F32(0.5) if one_score else _distinct(rng, 6000, 0.5, 0.53125)
    s[6300:] = _distinct(rng, nc * A - 6300, 0.01, 0.4)
    pred = np.zeros((1, 4 + nc, A), F32)
    pred[:, :4] = _boxes(rng, 1, A)
    pred[0, 4:] = rng.permutation(s).reshape(nc, A)
    return pred


def _topk_heavy(one_score):
    def build():
        pred = _heavy_pred("topk_heavy_one" if one_score else "topk_heavy_distinct", one_score)

        def check(k, rows, index):
            s = pred[0, 4:]
            heavy = _top_digit(s) == _top_digit(0.5)
            assert heavy.sum() == 6000 > NMS_CAP and (s >= 0.53125).sum() == 300 < k  # the first round yields < k; then the bin is opened
            assert ((s == F32(0.5)).sum() == 6000) == one_score
            if one_score:
                pair = index[0, 300:].astype(np.int64) * 8 + rows[0, 300:, 5].astype(np.int64)
                assert (rows[0, 300:, 4] == F32(0.5)).all() and (np.diff(pair) > 0).all()
        return TopkCase(pred, (1000,), check)
    return build


def _topk_all_equal():
    rng = _rng("topk_all_equal")
    nc, A = 9, 1024
    pred = np.zeros((1, 4 + nc, A), F32)
    pred[:, :4] = _boxes(rng, 1, A)
    pred[0, 4:] = 0.5

    def check(k, rows, index):
        pair = np.arange(k)
        np.testing.assert_array_equal(index[0], pair // nc)
        np.testing.assert_array_equal(rows[0, :, 5], (pair % nc).astype(F32))
    return TopkCase(pred, (1, 777, 1024), check)


def _zero_tail_pred(tag):
    rng = _rng(tag)
    nc, A = 8, 1024
    pred = np.zeros((1, 4 + nc, A), F32)
    pred[:, :4] = _boxes(rng, 1, A)
    s = np.zeros(nc * A, F32)
    s[rng.permutation(nc * A)[:50]] = _distinct(rng, 50, 0.1, 0.9)
    pred[0, 4:] = s.reshape(nc, A)
    return pred


def _topk_zero_tail():
    pred = _zero_tail_pred("topk_zero_tail")

    def check(k, rows, index):
        assert (pred[0, 4:] > 0).sum() == 50 and (pred[0, 4:] == 0).sum() == 8 * 1024 - 50
        assert (rows[0, :50, 4] > 0).all() and (rows[0, 50:, 4] == 0).all()
        pair = index[0, 50:].astype(np.int64) * 8 + rows[0, 50:, 5].astype(np.int64)
        assert (np.diff(pair) > 0).all()
    return TopkCase(pred, (400,), check)


def _topk_mixed():
    rng = _rng("topk_mixed")
    nc, A = 8, 1024
    pred = np.zeros((3, 4 + nc, A), F32)
    pred[:, :4] = _boxes(rng, 3, A)
    pred[0, 4:] = _distinct(rng, nc * A, 0.001, 0.999).reshape(nc, A)
    pred[1, 4:] = _heavy_pred("topk_mixed_heavy", True)[0, 4:]
    pred[2, 4:] = _zero_tail_pred("topk_mixed_zero")[0, 4:]

    def check(k, rows, index):
        assert (np.diff(rows[0, :, 4]) < 0).all()
        assert (rows[1, :, 4] == F32(0.5)).sum() == k - 300
        assert (rows[2, :, 4] == 0).sum() == k - 50
    return TopkCase(pred, (400, 1000), check)


TOPK_CASES = {
    "tie_free": _topk_tie_free(2, 7, 333, (1, 50, 333)), "nc1_a333": _topk_tie_free(2, 1, 333, (1, 300, 333)),
    "nc1_a1024": _topk_tie_free(2, 1, 1024, (1, 300, 1024)), "heavy_distinct": _topk_heavy(False), "heavy_one_score": _topk_heavy(True),
    "all_equal": _topk_all_equal, "zero_tail": _topk_zero_tail, "mixed_batch": _topk_mixed,
}
TIE_FREE = ("tie_free", "nc1_a333", "nc1_a1024")  # here torch.topk's order is determined, so oracle.model.e2e_postprocess applies too


@functools.lru_cache(maxsize=None)
def topk_reference(name):
    """(case, {k: (rows, index)}), computed once per process; do not modify."""
    case = TOPK_CASES[name]()
    return case, {k: topk_ref(case.pred, k) for k in case.ks}
