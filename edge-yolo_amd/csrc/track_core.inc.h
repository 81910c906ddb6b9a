// ByteTrack frame step and thresholded linear assignment, written once for the device (track.hip: one workgroup per stream / problem)
// and for the host (tests/track_host_main.cpp: one lane).  Everything here is stated against a tiny lane abstraction `L`:
//   ln.id() / ln.count()    this lane and the number of lanes that walk the same problem
//   ln.barrier()            every lane arrives; the writes made before it are visible to every lane after it
//   ln.argmin(v, j)         (v, j) becomes the lexicographic minimum over all lanes, the same in every lane (contains a barrier)
// Control flow is uniform: every lane of a problem takes every branch that contains a barrier together.  Every loop has a bound that is
// known before it starts (n, m, n + 1, T, cap); no comparison on a value computed from the data decides whether a loop goes on.
// Definition and phases: DESIGN.md section 7r.
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifndef TRK_HD
#define TRK_HD
#endif

namespace trk {

enum { FREE = 0, TRACKED = 1, LOST = 2 };
// per-slot int32 table [T][SI_N], per-slot fp32 table [T][SF_N], per-slot fp64 table [T][KF_N] (mean[8], covariance[8][8]), stream header [H_N]
enum { SI_STATE = 0, SI_ACT, SI_ID, SI_IDX, SI_FRAME, SI_START, SI_TLEN, SI_PAD, SI_N = 8 };
enum { SF_SCORE = 0, SF_CLS, SF_N = 2 };
enum { KF_N = 72 };
enum { H_FRAME = 0, H_LAST_ID, H_OVERFLOW, H_PAD, H_N = 4 };
enum { D_NONE = 0, D_HIGH = 1, D_SECOND = 2, D_USED = 3 };

#define TRK_BIG 1e300 /* "no edge": larger than any sum of 2 * (n + m) reduced costs of size <= 2 + |thresh| */

TRK_HD inline bool fin(float x) { return x - x == 0.0f; }
TRK_HD inline float fmin2(float a, float b) { return a < b ? a : b; }
TRK_HD inline float fmax2(float a, float b) { return a > b ? a : b; }

// ---------------------------------------------------------------------------------------------------------------------------------
// Thresholded linear assignment: the partial matching M of rows 0..n-1 and columns 0..m-1 that minimises sum over M of (c_ij - thresh),
// pairs with c_ij > thresh (or a NaN / Inf cost) excluded.  Stated as a rectangular problem: row i may also take a private dummy column
// of cost 0.  Shortest augmenting paths, one row at a time, with fp64 duals u (rows) and v (columns); a dummy column is free for as
// long as it exists (only its own row can take it), so it always ends a path and the whole set of dummies is carried as one
// candidate (dmin, drow) beside the columns' minv[].
// Column j is owned by lane j % count: minv, way, used and v of a column are touched by its owner only.
struct SolveScratch {
  double* u;     // [n]
  double* v;     // [m]
  double* minv;  // [m]
  int* way;      // [m]  the column through whose row this column was reached; -1: from the root row
  int* used;     // [m]
};

template <class L, class Cost>
TRK_HD void solve(L& ln, int n, int m, const Cost& cost, double thresh, const SolveScratch& s, int* row_col, int* col_row) {
  const int lane = ln.id(), nl = ln.count();
  if (n < 0) n = 0;
  if (m < 0) m = 0;
  for (int i = lane; i < n; i += nl) { row_col[i] = -1; s.u[i] = 0.0; }
  for (int j = lane; j < m; j += nl) { col_row[j] = -1; s.v[j] = 0.0; }
  ln.barrier();
  if (!(thresh - thresh == 0.0)) return;  // a NaN / Inf threshold admits no pair (uniform: thresh is the same in every lane)
  for (int i = 0; i < n; ++i) {           // bound: n augmentations
    for (int j = lane; j < m; j += nl) { s.minv[j] = TRK_BIG; s.way[j] = -1; s.used[j] = 0; }
    double dmin = TRK_BIG;
    int drow = -1, dcol = -1, i0 = i, j0 = -1, sink = -1;
    bool to_dummy = false;
    for (int step = 0; step <= n; ++step) {  // bound: a path enters at most n matched columns, then ends
      const double ui = s.u[i0];
      double best = TRK_BIG;
      int bj = 0x7fffffff;
      for (int j = lane; j < m; j += nl) {
        if (s.used[j]) continue;
        const float c = cost(i0, j);
        if (fin(c) && (double)c <= thresh) {
          const double cur = ((double)c - thresh) - ui - s.v[j];
          if (cur < s.minv[j]) { s.minv[j] = cur; s.way[j] = j0; }
        }
        if (s.minv[j] < best) { best = s.minv[j]; bj = j; }
      }
      const double cand = 0.0 - ui;  // the dummy column of row i0
      if (cand < dmin) { dmin = cand; drow = i0; dcol = j0; }
      ln.argmin(best, bj);
      const bool dummy = !(best < dmin);  // a tie goes to the dummy: the shorter matching
      const double delta = dummy ? dmin : best;
      for (int j = lane; j < m; j += nl) {
        if (s.used[j]) { s.u[col_row[j]] += delta; s.v[j] -= delta; }
        else if (s.minv[j] < TRK_BIG) s.minv[j] -= delta;
      }
      if (lane == 0) s.u[i] += delta;
      dmin -= delta;
      ln.barrier();
      if (dummy) { to_dummy = true; break; }
      j0 = bj;
      if (col_row[j0] < 0) { sink = j0; break; }
      if (j0 % nl == lane) s.used[j0] = 1;
      i0 = col_row[j0];
    }
    ln.barrier();  // every lane has read col_row[j0] before lane 0 rewrites the path
    if (lane == 0) {
      int j = sink;
      if (to_dummy) { row_col[drow] = -1; j = dcol; }
      for (int k = 0; k <= n && j >= 0; ++k) {  // bound: the path's columns
        const int jp = s.way[j];
        const int r = jp < 0 ? i : col_row[jp];
        col_row[j] = r;
        row_col[r] = j;
        j = jp;
      }
    }
    ln.barrier();
  }
}

// cost matrix in memory (ey_linear_assignment)
struct MatrixCost {
  const float* c;
  long ld;
  TRK_HD float operator()(int i, int j) const { return c[(long)i * ld + j]; }
};

// ---------------------------------------------------------------------------------------------------------------------------------
// boxes, in fp32 one operation at a time (the file is compiled without FMA contraction)

// detection row x1,y1,x2,y2 -> Boxes.xywh -> xywh2ltwh -> STrack.xyxy (xyxy) and tlwh_to_xyah (xyah)
TRK_HD inline void det_convert(const float* r, float* xyxy, float* xyah) {
  const float cx = (r[0] + r[2]) / 2.0f, cy = (r[1] + r[3]) / 2.0f, w = r[2] - r[0], h = r[3] - r[1];
  const float l = cx - w / 2.0f, t = cy - h / 2.0f;
  if (xyxy) { xyxy[0] = l; xyxy[1] = t; xyxy[2] = w + l; xyxy[3] = h + t; }
  if (xyah) { xyah[0] = l + w / 2.0f; xyah[1] = t + h / 2.0f; xyah[2] = w / h; xyah[3] = h; }
}

// fp64 state -> tlwh -> xyxy, then fp32
TRK_HD inline void track_box(const double* mean, float* xyxy) {
  const double w = mean[2] * mean[3], h = mean[3];
  const double l = mean[0] - w / 2.0, t = mean[1] - h / 2.0;
  xyxy[0] = (float)l; xyxy[1] = (float)t; xyxy[2] = (float)(w + l); xyxy[3] = (float)(h + t);
}

// bbox_ioa(a, b, iou=True), eps 1e-7
TRK_HD inline float box_iou(const float* a, const float* b) {
  float iw = fmin2(a[2], b[2]) - fmax2(a[0], b[0]);
  float ih = fmin2(a[3], b[3]) - fmax2(a[1], b[1]);
  iw = iw > 0.0f ? iw : 0.0f;
  ih = ih > 0.0f ? ih : 0.0f;
  const float inter = iw * ih;
  const float area2 = (b[2] - b[0]) * (b[3] - b[1]);
  const float area1 = (a[2] - a[0]) * (a[3] - a[1]);
  const float area = (area2 + area1) - inter;
  return inter / (area + 1e-7f);
}

// a NaN / Inf coordinate makes a box that matches nothing
TRK_HD inline bool box_ok(const float* a) { return fin(a[0] + a[1] + a[2] + a[3]); }

// rows: slots through rowlist, columns: detections through collist; 1 - IoU, or fuse_score's 1 - (1 - (1 - IoU)) * score
struct BoxCost {
  const float* tbox;
  const float* dbox;
  const float* dscore;
  const int* rowlist;
  const int* collist;
  int fuse;
  TRK_HD float operator()(int i, int j) const {
    const int d = collist[j];
    const float* a = tbox + 4 * rowlist[i];
    if (!box_ok(a)) return a[0] + a[1] + a[2] + a[3] + __builtin_inff();  // NaN or Inf: "no edge" to the solver
    const float iou = box_iou(a, dbox + 4 * d);
    const float c = 1.0f - iou;
    if (!fuse) return c;
    const float sim = 1.0f - c;
    const float f = sim * dscore[d];
    return 1.0f - f;
  }
};

// ---------------------------------------------------------------------------------------------------------------------------------
// KalmanFilterXYAH in fp64; kf = mean[8] then covariance[8][8]

TRK_HD inline void kf_initiate(double* kf, const float* z) {
  double* m = kf;
  double* P = kf + 8;
  for (int i = 0; i < 4; ++i) { m[i] = (double)z[i]; m[4 + i] = 0.0; }
  const double h = (double)z[3];
  const double sp = (2.0 * (1.0 / 20.0)) * h, sv = (10.0 * (1.0 / 160.0)) * h;
  const double sd[8] = {sp, sp, 1e-2, sp, sv, sv, 1e-5, sv};
  for (int i = 0; i < 64; ++i) P[i] = 0.0;
  for (int i = 0; i < 8; ++i) P[i * 9] = sd[i] * sd[i];
}

// mean = F mean, cov = (F cov) F^T + Q with F = [[I, I], [0, I]]; zero_vh: a track that is not Tracked forgets its height velocity first
TRK_HD inline void kf_predict(double* kf, bool zero_vh) {
  double* m = kf;
  double* P = kf + 8;
  if (zero_vh) m[7] = 0.0;
  const double sp = (1.0 / 20.0) * m[3], sv = (1.0 / 160.0) * m[3];
  const double sd[8] = {sp, sp, 1e-2, sp, sv, sv, 1e-5, sv};
  for (int i = 0; i < 4; ++i) m[i] = m[i] + m[4 + i];
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 8; ++j) P[i * 8 + j] = P[i * 8 + j] + P[(i + 4) * 8 + j];
  for (int i = 0; i < 8; ++i)
    for (int j = 0; j < 4; ++j) P[i * 8 + j] = P[i * 8 + j] + P[i * 8 + j + 4];
  for (int i = 0; i < 8; ++i) P[i * 9] += sd[i] * sd[i];
}

// project, Cholesky solve of the 4x4 innovation covariance, correction
TRK_HD inline void kf_update(double* kf, const float* z) {
  double* m = kf;
  double* P = kf + 8;
  const double w = (1.0 / 20.0) * m[3];
  double S[4][4], Lc[4][4], K[8][4];
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) { S[i][j] = P[i * 8 + j]; Lc[i][j] = 0.0; }
  S[0][0] += w * w; S[1][1] += w * w; S[2][2] += 1e-1 * 1e-1; S[3][3] += w * w;
  for (int j = 0; j < 4; ++j) {
    double d = S[j][j];
    for (int k = 0; k < j; ++k) d -= Lc[j][k] * Lc[j][k];
    Lc[j][j] = __builtin_sqrt(d);
    for (int i = j + 1; i < 4; ++i) {
      double e = S[i][j];
      for (int k = 0; k < j; ++k) e -= Lc[i][k] * Lc[j][k];
      Lc[i][j] = e / Lc[j][j];
    }
  }
  for (int i = 0; i < 8; ++i) {  // K[i][:] = S^-1 (cov H^T)[i][:]
    double y[4];
    for (int k = 0; k < 4; ++k) {
      double e = P[i * 8 + k];
      for (int l = 0; l < k; ++l) e -= Lc[k][l] * y[l];
      y[k] = e / Lc[k][k];
    }
    for (int k = 3; k >= 0; --k) {
      double e = y[k];
      for (int l = k + 1; l < 4; ++l) e -= Lc[l][k] * K[i][l];
      K[i][k] = e / Lc[k][k];
    }
  }
  double inn[4];
  for (int k = 0; k < 4; ++k) inn[k] = (double)z[k] - m[k];
  for (int i = 0; i < 8; ++i) {
    double a = 0.0;
    for (int k = 0; k < 4; ++k) a += inn[k] * K[i][k];
    m[i] = m[i] + a;
  }
  double KS[8][4];
  for (int i = 0; i < 8; ++i)
    for (int k = 0; k < 4; ++k) {
      double a = 0.0;
      for (int l = 0; l < 4; ++l) a += K[i][l] * S[l][k];
      KS[i][k] = a;
    }
  for (int i = 0; i < 8; ++i)
    for (int j = 0; j < 8; ++j) {
      double a = 0.0;
      for (int k = 0; k < 4; ++k) a += KS[i][k] * K[j][k];
      P[i * 8 + j] = P[i * 8 + j] - a;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
struct Params {
  float high, low, newt, match;
  int max_time_lost, fuse;
};

struct Stream {
  int cap, T;          // detection rows per stream, track slots per stream
  const float* rows;   // [cap][6] x1,y1,x2,y2,score,cls
  int count;
  double* kf;          // [T][KF_N]
  int* si;             // [T][SI_N]
  float* sf;           // [T][SF_N]
  int* hdr;            // [H_N]
  float* out_rows;     // [cap][8]
  int* out_ids;        // [cap]
  int* out_count;      // [1]
  // scratch: nothing in it lives from one frame to the next
  float* tbox;         // [T][4]    (LDS on the device)
  float* dbox;         // [cap][4]  (LDS)
  float* dscore;       // [cap]     (LDS)
  int* dkind;          // [cap]     (LDS)
  int* rowlist;        // [T]
  int* rowlist2;       // [T]
  int* collist;        // [cap]
  int* row_col;        // [T]
  int* col_row;        // [cap]
  int* flag;           // [T]
  int* cnts;           // [4]
  SolveScratch ss;     // u [T]; v, minv, way, used [cap]
};

// a matched pair: STrack.update / re_activate
template <class S>
TRK_HD inline void apply_match(const S& st, int t, int d, int frame) {
  float z[4];
  det_convert(st.rows + 6 * d, nullptr, z);
  kf_update(st.kf + (long)t * KF_N, z);
  int* si = st.si + t * SI_N;
  si[SI_TLEN] = si[SI_STATE] == TRACKED ? si[SI_TLEN] + 1 : 0;
  si[SI_STATE] = TRACKED;
  si[SI_ACT] = 1;
  si[SI_FRAME] = frame;
  si[SI_IDX] = d;
  st.sf[t * SF_N + SF_SCORE] = st.rows[6 * d + 4];
  st.sf[t * SF_N + SF_CLS] = st.rows[6 * d + 5];
  st.dkind[d] = D_USED;
}

// One ByteTrack frame of one stream (steps 0-9 of DESIGN.md 7r).
template <class L>
TRK_HD void frame_step(L& ln, const Params& P, const Stream& st) {
  const int lane = ln.id(), nl = ln.count();
  const int T = st.T;
  int cnt = st.count;
  if (cnt > st.cap) cnt = st.cap;
  if (cnt <= 0) {  // step 0: an empty frame touches nothing but its own output count
    if (lane == 0) st.out_count[0] = 0;
    return;
  }
  // ---- step 1: frame count, detection split
  const int frame = st.hdr[H_FRAME] + 1;
  for (int j = lane; j < cnt; j += nl) {
    const float* r = st.rows + 6 * j;
    const float s = r[4];
    int kind = D_NONE;
    if (fin(r[0]) && fin(r[1]) && fin(r[2]) && fin(r[3]) && fin(s)) {
      if (s >= P.high) kind = D_HIGH;
      else if (s > P.low && s < P.high) kind = D_SECOND;
    }
    det_convert(r, st.dbox + 4 * j, nullptr);
    st.dscore[j] = s;
    st.dkind[j] = kind;
  }
  // ---- step 2: predict the pool (activated tracked + lost); boxes of every live slot
  for (int t = lane; t < T; t += nl) {
    const int* si = st.si + t * SI_N;
    st.flag[t] = 0;
    if (si[SI_STATE] == FREE) continue;
    if (si[SI_STATE] == LOST || si[SI_ACT]) kf_predict(st.kf + (long)t * KF_N, si[SI_STATE] != TRACKED);
    track_box(st.kf + (long)t * KF_N, st.tbox + 4 * t);
  }
  ln.barrier();
  if (lane == 0) {
    st.hdr[H_FRAME] = frame;
    int nr = 0, nc = 0;
    for (int t = 0; t < T; ++t) {
      const int* si = st.si + t * SI_N;
      if (si[SI_STATE] == LOST || (si[SI_STATE] == TRACKED && si[SI_ACT])) st.rowlist[nr++] = t;
    }
    for (int j = 0; j < cnt; ++j)
      if (st.dkind[j] == D_HIGH) st.collist[nc++] = j;
    st.cnts[0] = nr;
    st.cnts[1] = nc;
  }
  ln.barrier();
  // ---- step 3: first association, pool x high detections
  int nr = st.cnts[0], nc = st.cnts[1];
  {
    const BoxCost cost = {st.tbox, st.dbox, st.dscore, st.rowlist, st.collist, P.fuse};
    solve(ln, nr, nc, cost, (double)P.match, st.ss, st.row_col, st.col_row);
  }
  for (int r = lane; r < nr; r += nl)
    if (st.row_col[r] >= 0) apply_match(st, st.rowlist[r], st.collist[st.row_col[r]], frame);
  ln.barrier();
  // ---- step 4: second association, unmatched pool tracks in state Tracked x second-round detections, plain IoU, 0.5
  if (lane == 0) {
    int n2 = 0, c2 = 0;
    for (int r = 0; r < nr; ++r)
      if (st.row_col[r] < 0 && st.si[st.rowlist[r] * SI_N + SI_STATE] == TRACKED) st.rowlist2[n2++] = st.rowlist[r];
    for (int j = 0; j < cnt; ++j)
      if (st.dkind[j] == D_SECOND) st.collist[c2++] = j;
    st.cnts[0] = n2;
    st.cnts[1] = c2;
  }
  ln.barrier();
  nr = st.cnts[0];
  nc = st.cnts[1];
  {
    const BoxCost cost = {st.tbox, st.dbox, st.dscore, st.rowlist2, st.collist, 0};
    solve(ln, nr, nc, cost, 0.5, st.ss, st.row_col, st.col_row);
  }
  for (int r = lane; r < nr; r += nl) {
    if (st.row_col[r] >= 0) apply_match(st, st.rowlist2[r], st.collist[st.row_col[r]], frame);
    else st.si[st.rowlist2[r] * SI_N + SI_STATE] = LOST;
  }
  ln.barrier();
  // ---- step 5: unconfirmed tracks x the high detections left over, fused, 0.7
  if (lane == 0) {
    int n3 = 0, c3 = 0;
    for (int t = 0; t < T; ++t) {
      const int* si = st.si + t * SI_N;
      if (si[SI_STATE] == TRACKED && !si[SI_ACT]) st.rowlist[n3++] = t;
    }
    for (int j = 0; j < cnt; ++j)
      if (st.dkind[j] == D_HIGH) st.collist[c3++] = j;
    st.cnts[0] = n3;
    st.cnts[1] = c3;
  }
  ln.barrier();
  nr = st.cnts[0];
  nc = st.cnts[1];
  {
    const BoxCost cost = {st.tbox, st.dbox, st.dscore, st.rowlist, st.collist, P.fuse};
    solve(ln, nr, nc, cost, 0.7, st.ss, st.row_col, st.col_row);
  }
  for (int r = lane; r < nr; r += nl) {
    if (st.row_col[r] >= 0) apply_match(st, st.rowlist[r], st.collist[st.row_col[r]], frame);
    else st.si[st.rowlist[r] * SI_N + SI_STATE] = FREE;
  }
  ln.barrier();
  // ---- step 6: new tracks, ascending detection index, into the lowest free slots (a slot freed by step 5 is free here already)
  if (lane == 0) {
    int nn = 0, t = 0, last = st.hdr[H_LAST_ID], over = 0;
    for (int j = 0; j < cnt; ++j) {
      if (st.dkind[j] != D_HIGH || st.dscore[j] < P.newt) continue;
      while (t < T && st.si[t * SI_N + SI_STATE] != FREE) ++t;  // bound: t only grows, to T
      if (t >= T) { ++over; continue; }
      st.rowlist[nn] = t++;
      st.collist[nn] = j;
      st.row_col[nn] = ++last;
      ++nn;
    }
    st.hdr[H_LAST_ID] = last;
    st.hdr[H_OVERFLOW] += over;
    st.cnts[0] = nn;
  }
  ln.barrier();
  nr = st.cnts[0];
  for (int k = lane; k < nr; k += nl) {
    const int t = st.rowlist[k], d = st.collist[k];
    float z[4];
    det_convert(st.rows + 6 * d, nullptr, z);
    kf_initiate(st.kf + (long)t * KF_N, z);
    int* si = st.si + t * SI_N;
    si[SI_STATE] = TRACKED;
    si[SI_ACT] = frame == 1;
    si[SI_ID] = st.row_col[k];
    si[SI_IDX] = d;
    si[SI_FRAME] = frame;
    si[SI_START] = frame;
    si[SI_TLEN] = 0;
    si[SI_PAD] = 0;
    st.sf[t * SF_N + SF_SCORE] = st.rows[6 * d + 4];
    st.sf[t * SF_N + SF_CLS] = st.rows[6 * d + 5];
  }
  ln.barrier();
  // ---- step 7: expiry; boxes as they are now, for step 8
  for (int t = lane; t < T; t += nl) {
    int* si = st.si + t * SI_N;
    if (si[SI_STATE] == LOST && frame - si[SI_FRAME] > P.max_time_lost) si[SI_STATE] = FREE;
    if (si[SI_STATE] != FREE) track_box(st.kf + (long)t * KF_N, st.tbox + 4 * t);
  }
  ln.barrier();
  // ---- step 8: duplicates, every (tracked, lost) pair on its own
  if (lane == 0) {
    int na = 0, nb = 0;
    for (int t = 0; t < T; ++t) {
      const int s = st.si[t * SI_N + SI_STATE];
      if (s == TRACKED) st.rowlist[na++] = t;
      else if (s == LOST) st.rowlist2[nb++] = t;
    }
    st.cnts[0] = na;
    st.cnts[1] = nb;
  }
  ln.barrier();
  nr = st.cnts[0];
  nc = st.cnts[1];
  for (int a = lane; a < nr; a += nl) {
    const int p = st.rowlist[a];
    const int timep = st.si[p * SI_N + SI_FRAME] - st.si[p * SI_N + SI_START];
    for (int b = 0; b < nc; ++b) {
      const int q = st.rowlist2[b];
      if (!box_ok(st.tbox + 4 * p) || !box_ok(st.tbox + 4 * q)) continue;
      const float dist = 1.0f - box_iou(st.tbox + 4 * p, st.tbox + 4 * q);
      if (!(dist < 0.15f)) continue;  // (a NaN distance is no duplicate)
      const int timeq = st.si[q * SI_N + SI_FRAME] - st.si[q * SI_N + SI_START];
      st.flag[timep > timeq ? q : p] = 1;  // (several lanes may write the same 1)
    }
  }
  ln.barrier();
  for (int t = lane; t < T; t += nl)
    if (st.flag[t]) st.si[t * SI_N + SI_STATE] = FREE;
  ln.barrier();
  // ---- step 9: one row per tracked, activated track, ascending id
  if (lane == 0) {
    int no = 0;
    for (int t = 0; t < T; ++t)
      if (st.si[t * SI_N + SI_STATE] == TRACKED && st.si[t * SI_N + SI_ACT]) st.rowlist[no++] = t;
    st.cnts[0] = no;
    st.out_count[0] = no < st.cap ? no : st.cap;
  }
  ln.barrier();
  nr = st.cnts[0];
  for (int k = lane; k < nr; k += nl) {
    const int t = st.rowlist[k];
    const int id = st.si[t * SI_N + SI_ID];
    int rank = 0;
    for (int o = 0; o < nr; ++o) rank += st.si[st.rowlist[o] * SI_N + SI_ID] < id;
    if (rank >= st.cap) continue;  // (cannot happen: every such track holds a detection of its own)
    float* o = st.out_rows + 8 * rank;
    track_box(st.kf + (long)t * KF_N, o);
    o[4] = (float)id;
    o[5] = st.sf[t * SF_N + SF_SCORE];
    o[6] = st.sf[t * SF_N + SF_CLS];
    o[7] = (float)st.si[t * SI_N + SI_IDX];
    st.out_ids[rank] = id;
  }
}

// bytes of the per-stream scratch that is not LDS, and its carving (shared by the device launcher and the host program)
TRK_HD inline size_t scratch_bytes(int cap, int T) {
  return ((size_t)T * (8 + 4 * 4) + (size_t)cap * (8 + 8 + 4 * 4) + 16 + 15) / 16 * 16;
}
TRK_HD inline void carve(Stream& st, char* p) {
  const int T = st.T, cap = st.cap;
  st.ss.u = (double*)p; p += (size_t)T * 8;
  st.ss.v = (double*)p; p += (size_t)cap * 8;
  st.ss.minv = (double*)p; p += (size_t)cap * 8;
  st.ss.way = (int*)p; p += (size_t)cap * 4;
  st.ss.used = (int*)p; p += (size_t)cap * 4;
  st.collist = (int*)p; p += (size_t)cap * 4;
  st.col_row = (int*)p; p += (size_t)cap * 4;
  st.rowlist = (int*)p; p += (size_t)T * 4;
  st.rowlist2 = (int*)p; p += (size_t)T * 4;
  st.row_col = (int*)p; p += (size_t)T * 4;
  st.flag = (int*)p; p += (size_t)T * 4;
  st.cnts = (int*)p;
}

}  // namespace trk
