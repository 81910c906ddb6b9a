"""Deterministic tracking sequences for the ByteTrack tests (tests/fp64_track_ref.py restates the step they exercise).
A case is {"name", "frames": [float32 (n, 6) rows x1,y1,x2,y2,score,cls per frame], "args": tracker settings, "max_tracks"}.
The seeds are picked so that every decision of every frame keeps a margin of 1e-4 (see `margins`); no frame is dropped to get there."""
import functools

import numpy as np

import fp64_track_ref as ref

F32 = np.float32


def scene(seed, nobj, width, height, frames=40):
    """nobj objects in linear motion of up to +-6 px/frame, box jitter sigma 1.5 px, ~8 % misses, ~12 % demoted to scores 0.12-0.22, ~3 % below
    0.1, 0-2 clutter boxes per frame, rows shuffled."""
    rng = np.random.default_rng(seed)
    pos = rng.uniform([0.1 * width, 0.1 * height], [0.9 * width, 0.9 * height], (nobj, 2))
    vel = rng.uniform(-6.0, 6.0, (nobj, 2))
    size = np.stack([rng.uniform(30, 90, nobj), rng.uniform(50, 140, nobj)], 1)
    cls = rng.integers(0, 5, nobj)
    out = []
    for f in range(frames):
        rows = []
        for o in range(nobj):
            c = pos[o] + vel[o] * f
            b = np.concatenate([c - size[o] / 2, c + size[o] / 2]) + rng.normal(0.0, 1.5, 4)
            u = rng.random()
            if u < 0.08:
                continue
            s = rng.uniform(0.12, 0.22) if u < 0.20 else rng.uniform(0.02, 0.08) if u < 0.23 else rng.uniform(0.35, 0.95)
            rows.append([*b, s, cls[o]])
        for _ in range(int(rng.integers(0, 3))):
            c = rng.uniform([0, 0], [width, height])
            wh = rng.uniform([20, 20], [120, 120])
            rows.append([*(c - wh / 2), *(c + wh / 2), rng.uniform(0.3, 0.9), int(rng.integers(0, 5))])
        rows = np.asarray(rows, dtype=F32).reshape(-1, 6)
        out.append(rows[rng.permutation(len(rows))])
    return out


def _box(cx, cy, w=80.0, h=120.0, score=0.9, cls=0.0):
    return [cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2, score, cls]


def occlusion(a_from=1):
    """A rests at (300, 240) from frame `a_from` on; B walks 12 px/frame onto A, arrives at frame 10, is undetected for frames 10-17 and is
    detected again from frame 18, moving away.  a_from = 1: A is the older track when B's lost track lands on it; a_from = 3: the younger."""
    out = []
    for f in range(1, 31):
        rows = []
        if f >= a_from:
            rows.append(_box(300.0, 240.0, score=0.9, cls=1.0))
        if f < 10:
            rows.append(_box(300.0 - 12.0 * (10 - f), 240.0, score=0.85, cls=2.0))
        elif f >= 18:
            rows.append(_box(300.0 + 12.0 * (f - 10), 240.0, score=0.85, cls=2.0))
        out.append(np.asarray(rows, dtype=F32).reshape(-1, 6))
    return out


def leave_and_return(gap, frames=26):
    """an anchor object that is always seen and a second one that is missing for `gap` frames from frame 6 on."""
    out = []
    for f in range(1, frames + 1):
        rows = [_box(100.0 + 2.0 * f, 100.0, score=0.8, cls=0.0)]
        if f < 6 or f >= 6 + gap:
            rows.append(_box(420.0 - 3.0 * f, 330.0, w=60.0, h=90.0, score=0.7, cls=3.0))
        out.append(np.asarray(rows, dtype=F32).reshape(-1, 6))
    return out


def with_empty(frames, at):
    return [np.zeros((0, 6), F32) if i in at else f for i, f in enumerate(frames)]


SEED_12, SEED_40 = 0, 1


@functools.lru_cache(maxsize=None)
def cases():
    s12, s40 = scene(SEED_12, 12, 640, 480), scene(SEED_40, 40, 1280, 960)
    short = {"track_buffer": 5}
    return [  # cases with the same settings and max_tracks run as the streams of ONE tracker in the GPU test (GROUPS)
        {"name": "scene12", "frames": s12, "args": {}, "max_tracks": 128},
        {"name": "scene40", "frames": s40, "args": {}, "max_tracks": 128},
        {"name": "empty_in_middle", "frames": with_empty(s12[:20], {0, 7, 8}), "args": {}, "max_tracks": 128},
        {"name": "occlusion_a_older", "frames": occlusion(1), "args": short, "max_tracks": 16},
        {"name": "occlusion_a_younger", "frames": occlusion(3), "args": short, "max_tracks": 16},
        {"name": "expire_and_return", "frames": leave_and_return(9), "args": short, "max_tracks": 16},
        {"name": "overflow8", "frames": s12[:24], "args": {}, "max_tracks": 8},
        {"name": "return_in_buffer", "frames": leave_and_return(3), "args": {}, "max_tracks": 8},
        {"name": "scene12_new_thresh", "frames": s12, "args": {"new_track_thresh": 0.6, "track_buffer": 8}, "max_tracks": 64},
    ]


GROUPS = ((0, 1, 2), (3, 4, 5), (6, 7), (8,))


def run_ref(case, ft=np.float64):
    """-> (tracker, per frame (output rows, snapshot))."""
    tr = ref.RefTracker(case["args"], max_tracks=case["max_tracks"], ft=ft)
    return tr, [(tr.update(rows), tr.snapshot()) for rows in case["frames"]]


@functools.lru_cache(maxsize=None)
def ref_run(i, long=False):
    """the restatement's run of case i, computed once and shared (read-only) by the tests."""
    return run_ref(cases()[i], np.longdouble if long else np.float64)


def margins(tracker):
    """least distances of a finished RefTracker's decisions from flipping: costs from their thresholds, scores from high / low / new, duplicate
    distances from 0.15, each assignment's optimum from its best alternative."""
    m = {"cost": np.inf, "score": np.inf, "dup": np.inf, "assign": np.inf}
    for rec in tracker.log:
        for cost, thresh in rec["assign"]:
            c = cost[np.isfinite(cost)].astype(np.float64)
            if c.size:
                m["cost"] = min(m["cost"], float(np.abs(c - thresh).min()))
            m["assign"] = min(m["assign"], ref.assignment_gap(cost, thresh))
        for s in rec["scores"]:
            m["score"] = min(m["score"], *(abs(s - float(t)) for t in (tracker.high, tracker.low, tracker.newt)))
        for d in rec["dups"]:
            m["dup"] = min(m["dup"], abs(d - float(F32(0.15))))
    return m


# ---- comparing a run of the kernel (or of its host build) with the restatement

def rounding_level():
    """d: the largest deviation, over every case, frame and live slot, between the restatement in float64 and in longdouble, of a mean or a
    covariance relative to its own largest entry -- the algorithm's own float64 rounding level."""
    d = 0.0
    for i in range(len(cases())):
        for (_, (si, _, kf, _)), (_, (sil, _, kfl, _)) in zip(ref_run(i)[1], ref_run(i, True)[1]):
            assert (si == sil).all()
            for t in np.nonzero(si[:, 0])[0]:
                for sl in (slice(0, 8), slice(8, 72)):
                    d = max(d, float(np.abs(kf[t, sl] - kfl[t, sl]).max() / np.abs(kfl[t, sl]).max()))
    return d


def compare_frame(what, want_rows, snap, cnt, rows, ids, hdr, si, sf, kf, kf_bar):
    """one frame of one stream against the restatement: the output count, the set of (id, idx, score, cls), the per-slot life-cycle fields and
    the header exactly; each box coordinate within one float32 ulp of the row's largest coordinate; means and covariances within kf_bar of the
    restatement's, relative to the largest entry of each.  -> the largest relative deviation of a mean or covariance seen."""
    wsi, wsf, wkf, whdr = snap
    assert cnt == len(want_rows), f"{what}: {cnt} rows, restatement {len(want_rows)}"
    assert tuple(int(v) for v in hdr[:3]) == tuple(whdr), f"{what}: header {hdr[:3]} vs {whdr}"
    assert (si[:, 0] == wsi[:, 0]).all(), f"{what}: slot states"
    live = wsi[:, 0] != 0
    assert (si[live, :7] == wsi[live]).all(), f"{what}: slot life-cycle fields"
    assert (sf[live].view(np.uint32) == wsf[live].view(np.uint32)).all(), f"{what}: slot score / cls"
    worst = 0.0
    for t in np.nonzero(live)[0]:
        for sl in (slice(0, 8), slice(8, 72)):
            worst = max(worst, float(np.abs(kf[t, sl] - wkf[t, sl]).max() / np.abs(wkf[t, sl]).max()))
    assert worst <= kf_bar, f"{what}: state deviates by {worst:.3e} of its largest entry, bar {kf_bar:.3e}"
    if cnt:
        got = rows[:cnt]
        assert (got[:, 4:].view(np.uint32) == want_rows[:, 4:].view(np.uint32)).all(), f"{what}: (id, score, cls, idx) of the rows"
        assert (ids[:cnt] == want_rows[:, 4].astype(np.int64)).all(), f"{what}: ids"
        ulp = np.spacing(np.abs(want_rows[:, :4]).max(1).astype(F32))[:, None]
        assert (np.abs(got[:, :4].astype(np.float64) - want_rows[:, :4].astype(np.float64)) <= ulp).all(), f"{what}: boxes beyond one ulp"
    return worst


# ---- assignment problems

def _gap_ok(cost, thresh, need=1e-5):
    return ref.assignment_gap(cost, thresh) >= need


def _random_cost(n, m, thresh, tag):
    """float32 costs in [0, 1] whose optimum beats every alternative by 1e-5: the first seed that gives one."""
    for seed in range(64):
        c = np.random.default_rng([seed, n, m, tag]).random((n, m)).astype(F32)
        if n == 0 or m == 0 or _gap_ok(c, thresh):
            return c
    raise AssertionError("no seed gives a unique optimum")


def staircase(n=128):
    """c[i][i] and c[i][i+1] small, the last row reaches column 0 only: rows 0 .. n-2 first sit on their diagonal, then the last row's
    augmenting path shifts every one of them to the right -- a path of length n."""
    c = np.full((n, n), 0.95, F32)
    r = np.random.default_rng(7)
    for i in range(n - 1):
        c[i, i] = 0.10 + 1e-3 * r.random()
        c[i, i + 1] = 0.102 + 1e-3 * r.random()
    c[n - 1, n - 1] = 0.95
    c[n - 1, 0] = 0.05
    return c


@functools.lru_cache(maxsize=None)
def assignment_cases():
    """[(name, cost float32 (n, m), thresh)] whose optimum is unique by 1e-5 (asserted): the matching must equal scipy's."""
    shapes = [(1, 1), (1, 5), (5, 1), (3, 3), (17, 9), (64, 65), (65, 64), (130, 300), (300, 130), (0, 4), (4, 0)]
    out = []
    for k, (n, m) in enumerate(shapes):
        th = (0.8, 0.5, 0.7)[k % 3]
        out.append((f"random_{n}x{m}_t{th}", _random_cost(n, m, th, k), th))
    out.append(("all_above", (0.85 + 0.15 * np.random.default_rng(3).random((9, 11))).astype(F32), 0.8))
    out.append(("staircase128", staircase(), 0.8))
    bad = _random_cost(12, 10, 0.8, 99).copy()
    bad[np.random.default_rng(5).random(bad.shape) < 0.25] = np.nan
    bad[3, :] = np.inf
    bad[:, 4] = -np.inf
    out.append(("nan_inf", bad, 0.8))
    for name, c, th in out:
        if c.size:
            assert _gap_ok(c, th), name
    return out


def tie_cases():
    """[(name, cost, thresh)] with many optima: any valid matching whose objective equals the optimum within 1e-9 passes."""
    r = np.random.default_rng(11).random((6, 9)).astype(F32)
    return [("all_equal", np.full((7, 5), 0.25, F32), 0.8), ("duplicated_rows", np.concatenate([r, r, r[:2]]), 0.7),
            ("equal_to_thresh", np.full((4, 4), 0.5, F32), 0.5)]


def check_matching(name, cost, thresh, r2c, c2r, exact):
    """r2c / c2r int arrays of the live range.  exact: identical to scipy's; else valid and optimal within 1e-9."""
    n, m = cost.shape
    want, best = ref.solve_rect(cost, float(F32(thresh)))
    r2c, c2r = np.asarray(r2c, np.int64), np.asarray(c2r, np.int64)
    assert r2c.shape == (n,) and c2r.shape == (m,), name
    assert ((r2c >= -1) & (r2c < m)).all() and ((c2r >= -1) & (c2r < n)).all(), name
    for i in np.nonzero(r2c >= 0)[0]:
        assert c2r[r2c[i]] == i, f"{name}: row {i} and column {r2c[i]} disagree"
        c = float(cost[i, r2c[i]])
        assert np.isfinite(c) and c <= float(F32(thresh)), f"{name}: pair above the threshold or not finite"
    assert (c2r >= 0).sum() == (r2c >= 0).sum(), name
    if exact:
        assert (r2c == want).all(), f"{name}: matching differs from scipy's"
    else:
        obj = sum(float(cost[i, r2c[i]]) - float(F32(thresh)) for i in np.nonzero(r2c >= 0)[0])
        assert abs(obj - best) <= 1e-9, f"{name}: objective {obj} vs optimum {best}"
