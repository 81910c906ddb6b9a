// Host build of the matching core (edge-yolo_amd/csrc/match_core.inc.h) with ONE lane: the same text the HIP kernel runs, as a plain program
// that reads a batch from a file and writes its true positives and confusion matrix, so that it can be compared with the reference's
// recorded results and run under AddressSanitizer / UBSan without a GPU.  Every array is an allocation of its own, of exactly the size the
// kernel is promised (the rows of an image end at its count), so that an index past any of them is reported.
//
//   match_host_main <case file> <result file>
// case file (little endian): int32 head[12] = B, stride, T, nc, has_xform, matrix_mode, want_tp, want_matrix, 0, 0, 0, 0; float cm_conf, cm_iou;
//   float iouv[T]; int32 count[B]; int32 gt_off[B+1]; float rows[sum count][stride]; float xform[B][5] when has_xform; float gt[M][4] unless
//   matrix_mode; int32 gt_cls[M]; float iou[sum_b G_b * count_b] when matrix_mode (image after image, row-major [G_b][count_b])
// result: uint8 tp[sum count][T] when want_tp (bytes nobody wrote hold 9); int32 matrix[(nc+1)^2] when want_matrix
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../edge-yolo_amd/csrc/match_core.inc.h"

struct HostLanes {
  int id() const { return 0; }
  int count() const { return 1; }
  void barrier() {}
  void amin(int* p, int v) { if (v < *p) *p = v; }
  void amax(mtc::u64* p, mtc::u64 v) { if (v > *p) *p = v; }
  void gadd(int* p) { ++*p; }
};

template <class T>
static bool get(FILE* f, std::vector<T>& v) { return v.empty() || fread(v.data(), sizeof(T), v.size(), f) == v.size(); }
template <class T>
static void put(FILE* f, const std::vector<T>& v) { if (!v.empty()) fwrite(v.data(), sizeof(T), v.size(), f); }

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) return 2;
  std::vector<int> head(12);
  std::vector<float> cm(2);
  if (!get(in, head) || !get(in, cm)) return 3;
  const int B = head[0], stride = head[1], T = head[2], nc = head[3];
  const bool has_xform = head[4], matrix_mode = head[5], want_tp = head[6], want_matrix = head[7];
  if (B < 0 || stride < 6 || T < 1 || T > mtc::MAX_T || nc < 1) return 3;
  std::vector<float> iouv(T);
  std::vector<int> count(B), gt_off(B + 1);
  if (!get(in, iouv) || !get(in, count) || !get(in, gt_off)) return 3;
  std::vector<std::vector<float>> rows(B), xform(B), gbox(B), iou(B);
  std::vector<std::vector<int>> gcls(B);
  for (int b = 0; b < B; ++b) {
    if (count[b] < 0 || gt_off[b + 1] < gt_off[b]) return 3;
    rows[b].resize((size_t)count[b] * stride);
    if (!get(in, rows[b])) return 3;
  }
  for (int b = 0; b < B && has_xform; ++b) {
    xform[b].resize(5);
    if (!get(in, xform[b])) return 3;
  }
  for (int b = 0; b < B && !matrix_mode; ++b) {
    gbox[b].resize((size_t)(gt_off[b + 1] - gt_off[b]) * 4);
    if (!get(in, gbox[b])) return 3;
  }
  for (int b = 0; b < B; ++b) {
    gcls[b].resize(gt_off[b + 1] - gt_off[b]);
    if (!get(in, gcls[b])) return 3;
  }
  for (int b = 0; b < B && matrix_mode; ++b) {
    iou[b].resize((size_t)(gt_off[b + 1] - gt_off[b]) * count[b]);
    if (!get(in, iou[b])) return 3;
  }
  std::vector<int> matrix(want_matrix ? (size_t)(nc + 1) * (nc + 1) : 0, 0);
  HostLanes ln;
  for (int b = 0; b < B; ++b) {
    const int D = count[b], G = gt_off[b + 1] - gt_off[b];
    std::vector<unsigned char> tp(want_tp ? (size_t)D * T : 0, 9);
    std::vector<float> lbox(matrix_mode ? 0 : (size_t)G * 4, -7.f), db(want_tp ? D : 0, -7.f);
    std::vector<int> lcls(G, -7), taker(want_tp ? (size_t)G * T : 0, -7), dg(want_tp ? D : 0, -7), cg(want_matrix ? D : 0, -7);
    std::vector<mtc::u64> cmkey(want_matrix ? G : 0, 7);
    mtc::Job J;
    J.D = D; J.G = G; J.T = T; J.nc = nc; J.stride = stride;
    J.rows = rows[b].data();
    J.xform = has_xform && !matrix_mode ? xform[b].data() : nullptr;
    J.gbox = matrix_mode ? nullptr : gbox[b].data();
    J.gcls = gcls[b].data();
    J.iou = matrix_mode ? iou[b].data() : nullptr;
    J.ld = D;
    J.iouv = iouv.data();
    J.cm_conf = cm[0]; J.cm_iou = cm[1];
    J.tp = want_tp ? tp.data() : nullptr;
    J.matrix = want_matrix ? matrix.data() : nullptr;
    J.lbox = lbox.data(); J.lcls = lcls.data(); J.taker = taker.data(); J.cmkey = cmkey.data(); J.dg = dg.data(); J.db = db.data(); J.cg = cg.data();
    mtc::match(ln, J);
    put(out, tp);
  }
  put(out, matrix);
  fclose(in);
  return fclose(out) == 0 ? 0 : 4;
}
