// Host build of the tracker's core (edge-yolo_amd/csrc/track_core.inc.h) with ONE lane: the same text the HIP kernels run, as a plain
// program that reads a case file and writes results and state, so that the frame step and the solver can be compared with the float64
// restatement (tests/fp64_track_ref.py) and run under AddressSanitizer / UBSan without a GPU.  Every array is an allocation of its own,
// of exactly the size the kernels are promised, so that an index past any of them is reported.
//
//   track_host_main <case file> <result file>
// case file (little endian): int32 head[8] = mode, a, b, c, d, e, 0, 0; float32 thr[4]; payload
//   mode 1 (ByteTrack): a = cap, b = max_tracks, c = frames, d = max_time_lost, e = fuse_score; thr = high, low, new, match;
//       per frame: int32 count, float32 rows[cap][6]
//     result, per frame: int32 out_count, float32 out_rows[cap][8], int32 out_ids[cap], int32 hdr[4], int32 slot_i[T][8], float32 slot_f[T][2],
//       float64 kf[T][72]
//   mode 2 (assignment): a = n, b = m, c = ld; thr[0] = thresh; float32 cost[n][ld];  result: int32 row_to_col[n], col_to_row[m]
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../edge-yolo_amd/csrc/track_core.inc.h"

struct HostLanes {
  int id() const { return 0; }
  int count() const { return 1; }
  void barrier() {}
  void argmin(double&, int&) {}
};

template <class T>
static bool get(FILE* f, T* p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }
template <class T>
static void put(FILE* f, const T* p, size_t n) { if (n) fwrite(p, sizeof(T), n, f); }

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) return 2;
  int head[8];
  float thr[4];
  if (!get(in, head, 8) || !get(in, thr, 4)) return 3;
  HostLanes ln;
  if (head[0] == 2) {
    const int n = head[1], m = head[2], ld = head[3];
    if (n < 0 || m < 0 || ld < m) return 3;
    std::vector<float> cost((size_t)n * ld);
    if (!get(in, cost.data(), cost.size())) return 3;
    std::vector<double> u(n), v(m), minv(m);
    std::vector<int> way(m), used(m), rc(n, -7), cr(m, -7);
    const trk::SolveScratch s = {u.data(), v.data(), minv.data(), way.data(), used.data()};
    const trk::MatrixCost c = {cost.data(), ld};
    trk::solve(ln, n, m, c, (double)thr[0], s, rc.data(), cr.data());
    put(out, rc.data(), rc.size());
    put(out, cr.data(), cr.size());
  } else if (head[0] == 1) {
    const int cap = head[1], T = head[2], frames = head[3];
    if (cap < 1 || T < 1 || frames < 0) return 3;
    const trk::Params P = {thr[0], thr[1], thr[2], thr[3], head[4], head[5] != 0};
    std::vector<float> rows((size_t)cap * 6), sf((size_t)T * trk::SF_N, 0.f), orow((size_t)cap * 8, 0.f), tbox((size_t)T * 4), dbox((size_t)cap * 4), dscore(cap);
    std::vector<double> kf((size_t)T * trk::KF_N, 0.0), u(T), v(cap), minv(cap);
    std::vector<int> si((size_t)T * trk::SI_N, 0), hdr(trk::H_N, 0), oid(cap, 0), ocnt(1, 0), dkind(cap), rl(T), rl2(T), cl(cap), rc(T), cr(cap), flag(T), cnts(4),
        way(cap), used(cap);
    for (int f = 0; f < frames; ++f) {
      int count;
      if (!get(in, &count, 1) || !get(in, rows.data(), rows.size())) return 3;
      trk::Stream st;
      st.cap = cap; st.T = T; st.rows = rows.data(); st.count = count;
      st.kf = kf.data(); st.si = si.data(); st.sf = sf.data(); st.hdr = hdr.data();
      st.out_rows = orow.data(); st.out_ids = oid.data(); st.out_count = ocnt.data();
      st.tbox = tbox.data(); st.dbox = dbox.data(); st.dscore = dscore.data(); st.dkind = dkind.data();
      st.rowlist = rl.data(); st.rowlist2 = rl2.data(); st.collist = cl.data(); st.row_col = rc.data(); st.col_row = cr.data();
      st.flag = flag.data(); st.cnts = cnts.data();
      st.ss.u = u.data(); st.ss.v = v.data(); st.ss.minv = minv.data(); st.ss.way = way.data(); st.ss.used = used.data();
      trk::frame_step(ln, P, st);
      put(out, ocnt.data(), 1);
      put(out, orow.data(), orow.size());
      put(out, oid.data(), oid.size());
      put(out, hdr.data(), hdr.size());
      put(out, si.data(), si.size());
      put(out, sf.data(), sf.size());
      put(out, kf.data(), kf.size());
    }
  } else {
    return 3;
  }
  fclose(in);
  return fclose(out) == 0 ? 0 : 4;
}
