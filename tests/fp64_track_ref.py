"""Restatement of one ByteTrack frame step per stream (reference trackers/byte_tracker.py BYTETracker.update, STrack,
trackers/utils/kalman_filter.py KalmanFilterXYAH, trackers/utils/matching.py, utils/metrics.py bbox_ioa) in numpy: the Kalman filter in `ft`
(float64, or longdouble to measure the algorithm's own rounding level), boxes / IoU / costs in float32 one operation at a time, the assignment
by scipy.optimize.linear_sum_assignment on the rectangular form (row i has a private dummy column of cost 0, a pair costs c - thresh, pairs
above thresh are forbidden).  Nothing of the reference's trackers package is imported.

Slots: `max_tracks` per stream; a new track takes the lowest free slot.  A slot freed by the unconfirmed round (step 5) of a frame is free
for the new tracks (step 6) of the same frame; a slot freed by expiry (step 7) or as a duplicate (step 8) is free from the next frame on.

The tracker counts how often each path is taken (`counters`) and logs every decision (`log`) for the margin tests."""
import numpy as np
from scipy.optimize import linear_sum_assignment

FREE, TRACKED, LOST = 0, 1, 2
DEFAULTS = {"tracker_type": "bytetrack", "track_high_thresh": 0.25, "track_low_thresh": 0.1, "new_track_thresh": 0.25, "track_buffer": 30,
            "match_thresh": 0.8, "fuse_score": True}
PATHS = ("first_match", "second_match", "unconfirmed_match", "refound", "lost", "expired", "dup_drop_tracked", "dup_drop_lost", "new",
         "new_below_thresh", "empty_frame", "overflow", "unconfirmed_removed")
F32 = np.float32
_FORBID = 1e6


def solve_rect(cost, thresh, forbid=()):
    """-> (row_to_col int array (-1 = dummy), objective).  cost (n, m) any float; forbid: (i, j) pairs to exclude, j = -1 for row i's dummy."""
    cost = np.asarray(cost, dtype=np.float64)
    n, m = cost.shape
    r2c = -np.ones(n, dtype=np.int64)
    if n == 0:
        return r2c, 0.0
    ok = np.isfinite(cost) & (cost <= thresh) if np.isfinite(thresh) else np.zeros((n, m), bool)
    W = np.full((n, m + n), _FORBID)
    W[:, :m][ok] = (cost - thresh)[ok]
    W[np.arange(n), m + np.arange(n)] = 0.0
    for i, j in forbid:
        W[i, (m + i) if j < 0 else j] = _FORBID
    ri, ci = linear_sum_assignment(W)
    for r, c in zip(ri, ci):
        if c < m:
            r2c[r] = c
    return r2c, float(W[ri, ci].sum())


def assignment_gap(cost, thresh):
    """objective of the best assignment that differs from the optimum in at least one chosen edge, minus the optimum (inf: no alternative)."""
    r2c, best = solve_rect(cost, thresh)
    gap = np.inf
    for i, j in enumerate(r2c):
        alt = solve_rect(cost, thresh, forbid=[(i, int(j))])[1]
        if alt < _FORBID / 2:
            gap = min(gap, alt - best)
    return gap


def det_convert(rows):
    """rows (n, >=4) float32 xyxy -> (xyxy' , xyah) float32, op by op as Boxes.xywh, xywh2ltwh, STrack.xyxy and tlwh_to_xyah."""
    r = np.asarray(rows, dtype=F32)
    two = F32(2)
    cx, cy, w, h = (r[:, 0] + r[:, 2]) / two, (r[:, 1] + r[:, 3]) / two, r[:, 2] - r[:, 0], r[:, 3] - r[:, 1]
    l, t = cx - w / two, cy - h / two
    with np.errstate(all="ignore"):
        xyah = np.stack([l + w / two, t + h / two, w / h, h], 1).astype(F32)
    return np.stack([l, t, w + l, h + t], 1).astype(F32), xyah


def track_box(mean):
    """state mean (ft) -> tlwh -> xyxy in ft, then float32."""
    w, h = mean[2] * mean[3], mean[3]
    l, t = mean[0] - w / 2, mean[1] - h / 2
    return np.array([l, t, w + l, h + t]).astype(F32)


def iou_f32(a, b):
    """bbox_ioa(a, b, iou=True) in float32: (n, 4) x (m, 4) -> (n, m)."""
    a, b = np.asarray(a, F32).reshape(-1, 4), np.asarray(b, F32).reshape(-1, 4)
    with np.errstate(all="ignore"):
        iw = (np.minimum(a[:, None, 2], b[None, :, 2]) - np.maximum(a[:, None, 0], b[None, :, 0])).clip(0)
        ih = (np.minimum(a[:, None, 3], b[None, :, 3]) - np.maximum(a[:, None, 1], b[None, :, 1])).clip(0)
        inter = iw * ih
        area2 = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
        area1 = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
        area = (area2[None, :] + area1[:, None]) - inter
        out = inter / (area + F32(1e-7))
    assert out.dtype == F32
    return out


def costs_f32(tboxes, dboxes, scores=None):
    """1 - IoU; with scores fuse_score's 1 - (1 - (1 - IoU)) * score, float32 op by op.  A track box with a NaN / Inf coordinate matches nothing."""
    c = F32(1) - iou_f32(tboxes, dboxes)
    if scores is not None:
        c = F32(1) - (F32(1) - c) * np.asarray(scores, F32)[None, :]
    bad = ~np.isfinite(np.asarray(tboxes, F32).reshape(-1, 4).sum(1))
    c[bad] = np.inf
    return c


class Kalman:
    """KalmanFilterXYAH in the float type `ft`; the constants are the float64 ones in every type."""

    def __init__(self, ft):
        self.ft = ft
        self.wp, self.wv = ft(1.0 / 20.0), ft(1.0 / 160.0)
        self.c2, self.c5, self.c1 = ft(1e-2), ft(1e-5), ft(1e-1)

    def initiate(self, z):
        ft = self.ft
        z = np.asarray(z, F32).astype(ft)
        mean = np.concatenate([z, np.zeros(4, ft)])
        sp, sv = (ft(2.0) * self.wp) * z[3], (ft(10.0) * self.wv) * z[3]
        std = np.array([sp, sp, self.c2, sp, sv, sv, self.c5, sv], dtype=ft)
        return mean, np.diag(std * std)

    def predict(self, mean, cov):
        ft = self.ft
        sp, sv = self.wp * mean[3], self.wv * mean[3]
        std = np.array([sp, sp, self.c2, sp, sv, sv, self.c5, sv], dtype=ft)
        mean = mean.copy()
        mean[:4] = mean[:4] + mean[4:]
        cov = cov.copy()
        cov[:4, :] = cov[:4, :] + cov[4:, :]
        cov[:, :4] = cov[:, :4] + cov[:, 4:]
        cov[np.arange(8), np.arange(8)] += std * std
        return mean, cov

    def update(self, mean, cov, z):
        ft = self.ft
        z = np.asarray(z, F32).astype(ft)
        w = self.wp * mean[3]
        S = cov[:4, :4].copy()
        S[np.arange(4), np.arange(4)] += np.array([w * w, w * w, self.c1 * self.c1, w * w], dtype=ft)
        L = np.zeros((4, 4), ft)
        for j in range(4):
            d = S[j, j]
            for k in range(j):
                d = d - L[j, k] * L[j, k]
            L[j, j] = np.sqrt(d)
            for i in range(j + 1, 4):
                e = S[i, j]
                for k in range(j):
                    e = e - L[i, k] * L[j, k]
                L[i, j] = e / L[j, j]
        K = np.zeros((8, 4), ft)
        for i in range(8):
            y = np.zeros(4, ft)
            for k in range(4):
                e = cov[i, k]
                for l in range(k):
                    e = e - L[k, l] * y[l]
                y[k] = e / L[k, k]
            for k in range(3, -1, -1):
                e = y[k]
                for l in range(k + 1, 4):
                    e = e - L[l, k] * K[i, l]
                K[i, k] = e / L[k, k]
        inn = z - mean[:4]
        new_mean = mean + K @ inn
        new_cov = cov - (K @ S) @ K.T
        return new_mean.astype(ft), new_cov.astype(ft)


class Slot:
    __slots__ = ("mean", "cov", "state", "act", "id", "idx", "frame", "start", "tlen", "score", "cls")


class RefTracker:
    """One stream.  update(rows) -> (k, 8) float32 rows [x1, y1, x2, y2, id, score, cls, idx] in ascending id."""

    def __init__(self, args=None, max_tracks=1024, ft=np.float64):
        a = dict(DEFAULTS)
        a.update(args or {})
        self.high, self.low, self.newt, self.match = (F32(a[k]) for k in ("track_high_thresh", "track_low_thresh", "new_track_thresh", "match_thresh"))
        self.max_time_lost = int(30 / 30.0 * a["track_buffer"])
        self.fuse = bool(a["fuse_score"])
        self.T, self.ft, self.kf = int(max_tracks), ft, Kalman(ft)
        self.slots = [None] * self.T
        self.frame_id, self.last_id, self.overflow = 0, 0, 0
        self.counters = {k: 0 for k in PATHS}
        self.log = []  # per frame: {"assign": [(cost, thresh)], "scores": [...], "dups": [...]}

    # -- helpers
    def _box(self, t):
        return track_box(self.slots[t].mean)

    def _assign(self, rows_t, cols_d, dbox, dscore, fuse, thresh, rec):
        if not rows_t or not cols_d:
            return -np.ones(len(rows_t), dtype=np.int64)
        cost = costs_f32(np.stack([self._box(t) for t in rows_t]), dbox[cols_d], dscore[cols_d] if fuse else None)
        rec["assign"].append((cost, float(thresh)))
        return solve_rect(cost, float(thresh))[0]

    def _match(self, t, d, rows, xyah):
        s = self.slots[t]
        s.mean, s.cov = self.kf.update(s.mean, s.cov, xyah[d])
        if s.state == TRACKED:
            s.tlen += 1
        else:
            s.tlen = 0
            self.counters["refound"] += 1
        s.state, s.act, s.frame, s.idx, s.score, s.cls = TRACKED, 1, self.frame_id, d, F32(rows[d, 4]), F32(rows[d, 5])

    def update(self, rows):
        rows = np.asarray(rows, dtype=F32).reshape(-1, 6)
        n = len(rows)
        if n == 0:  # step 0
            self.counters["empty_frame"] += 1
            return np.zeros((0, 8), F32)
        rec = {"assign": [], "scores": [], "dups": []}
        self.log.append(rec)
        self.frame_id += 1
        S = self.slots
        # step 1
        dbox, xyah = det_convert(rows)
        score = rows[:, 4]
        ok = np.isfinite(rows[:, :5]).all(1)
        kind = np.zeros(n, int)
        kind[ok & (score >= self.high)] = 1
        kind[ok & (score > self.low) & (score < self.high)] = 2
        rec["scores"] = [float(v) for v in score[ok]]
        # step 2
        pool = [t for t in range(self.T) if S[t] is not None and (S[t].state == LOST or (S[t].state == TRACKED and S[t].act))]
        for t in pool:
            m = S[t].mean.copy()
            if S[t].state != TRACKED:
                m[7] = 0
            S[t].mean, S[t].cov = self.kf.predict(m, S[t].cov)
        # step 3
        high = [j for j in range(n) if kind[j] == 1]
        r2c = self._assign(pool, high, dbox, score, self.fuse, self.match, rec)
        for r, c in enumerate(r2c):
            if c >= 0:
                self._match(pool[r], high[c], rows, xyah)
                kind[high[c]] = 3
                self.counters["first_match"] += 1
        # step 4
        rest = [pool[r] for r, c in enumerate(r2c) if c < 0 and S[pool[r]].state == TRACKED]
        second = [j for j in range(n) if kind[j] == 2]
        r2c = self._assign(rest, second, dbox, score, False, F32(0.5), rec)
        for r, c in enumerate(r2c):
            if c >= 0:
                self._match(rest[r], second[c], rows, xyah)
                kind[second[c]] = 3
                self.counters["second_match"] += 1
            else:
                S[rest[r]].state = LOST
                self.counters["lost"] += 1
        # step 5
        unconf = [t for t in range(self.T) if S[t] is not None and S[t].state == TRACKED and not S[t].act]
        high = [j for j in range(n) if kind[j] == 1]
        r2c = self._assign(unconf, high, dbox, score, self.fuse, F32(0.7), rec)
        for r, c in enumerate(r2c):
            if c >= 0:
                self._match(unconf[r], high[c], rows, xyah)
                kind[high[c]] = 3
                self.counters["unconfirmed_match"] += 1
            else:
                S[unconf[r]] = None
                self.counters["unconfirmed_removed"] += 1
        # step 6
        t = 0
        for j in range(n):
            if kind[j] != 1:
                continue
            if score[j] < self.newt:
                self.counters["new_below_thresh"] += 1
                continue
            while t < self.T and S[t] is not None:
                t += 1
            if t >= self.T:
                self.overflow += 1
                self.counters["overflow"] += 1
                continue
            s = Slot()
            s.mean, s.cov = self.kf.initiate(xyah[j])
            self.last_id += 1
            s.state, s.act, s.id, s.idx, s.frame, s.start, s.tlen = TRACKED, int(self.frame_id == 1), self.last_id, j, self.frame_id, self.frame_id, 0
            s.score, s.cls = F32(rows[j, 4]), F32(rows[j, 5])
            S[t] = s
            t += 1
            self.counters["new"] += 1
        # step 7
        for t in range(self.T):
            if S[t] is not None and S[t].state == LOST and self.frame_id - S[t].frame > self.max_time_lost:
                S[t] = None
                self.counters["expired"] += 1
        # step 8
        tr = [t for t in range(self.T) if S[t] is not None and S[t].state == TRACKED]
        lo = [t for t in range(self.T) if S[t] is not None and S[t].state == LOST]
        drop = set()
        if tr and lo:
            A, Bx = np.stack([self._box(t) for t in tr]), np.stack([self._box(t) for t in lo])
            dist = F32(1) - iou_f32(A, Bx)
            fine = np.isfinite(A.sum(1))[:, None] & np.isfinite(Bx.sum(1))[None, :]
            rec["dups"] = [float(v) for v in dist[fine]]
            for a, p in enumerate(tr):
                for b, q in enumerate(lo):
                    if fine[a, b] and dist[a, b] < F32(0.15):
                        if S[p].frame - S[p].start > S[q].frame - S[q].start:
                            drop.add(q)
                        else:
                            drop.add(p)
        for t in drop:
            self.counters["dup_drop_tracked" if S[t].state == TRACKED else "dup_drop_lost"] += 1
            S[t] = None
        # step 9
        outs = sorted((S[t] for t in range(self.T) if S[t] is not None and S[t].state == TRACKED and S[t].act), key=lambda s: s.id)
        return np.array([[*track_box(s.mean), s.id, s.score, s.cls, s.idx] for s in outs], dtype=F32).reshape(-1, 8)

    def snapshot(self):
        """(slot_i (T, 7) int: state, act, id, idx, frame, start, tlen -- zeros but the state for a free slot; slot_f (T, 2) float32;
        kf (T, 72) in ft; hdr (frame_id, last id, overflow))."""
        si, sf, kf = np.zeros((self.T, 7), np.int64), np.zeros((self.T, 2), F32), np.zeros((self.T, 72), self.ft)
        for t, s in enumerate(self.slots):
            if s is not None:
                si[t] = (s.state, s.act, s.id, s.idx, s.frame, s.start, s.tlen)
                sf[t] = (s.score, s.cls)
                kf[t, :8], kf[t, 8:] = s.mean, s.cov.reshape(-1)
        return si, sf, kf, (self.frame_id, self.last_id, self.overflow)
