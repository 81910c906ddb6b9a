// Object tracking (reference trackers/byte_tracker.py, trackers/utils/{kalman_filter,matching}.py): ey_linear_assignment and
// ey_bytetrack_update.  The algorithm text is track_core.inc.h, shared with the host program of the tests; this file gives it the
// workgroup's lanes (256 threads = 4 waves per stream / problem) and launches it.  DESIGN.md section 7r.
#include "common.h"
#define TRK_HD __device__ __host__
#include "track_core.inc.h"

#define TRK_THREADS 256

namespace {

struct DevLanes {
  double* rv;  // LDS [2][4]: the waves' minima, double-buffered so that one barrier per argmin is enough
  int* ri;
  int par;
  __device__ int id() const { return (int)threadIdx.x; }
  __device__ int count() const { return (int)blockDim.x; }
  __device__ void barrier() { __syncthreads(); }
  __device__ void argmin(double& v, int& j) {
#pragma unroll
    for (int o = 32; o; o >>= 1) {
      const double ov = __shfl_xor(v, o, 64);
      const int oj = __shfl_xor(j, o, 64);
      if (ov < v || (ov == v && oj < j)) { v = ov; j = oj; }
    }
    const int w = (int)threadIdx.x >> 6, nw = (int)blockDim.x >> 6;
    if ((threadIdx.x & 63) == 0) { rv[par * 4 + w] = v; ri[par * 4 + w] = j; }
    __syncthreads();
    v = rv[par * 4];
    j = ri[par * 4];
    for (int k = 1; k < nw; ++k) {
      const double ov = rv[par * 4 + k];
      const int oj = ri[par * 4 + k];
      if (ov < v || (ov == v && oj < j)) { v = ov; j = oj; }
    }
    par ^= 1;
  }
};

__global__ __launch_bounds__(TRK_THREADS) void linear_assignment_kernel(const long* __restrict__ desc, const float* __restrict__ thresh, int nmax, int mmax,
                                                                         int* row_to_col, int ldr, int* col_to_row, int ldc, char* ws, size_t ws_stride) {
  __shared__ double rv[8];
  __shared__ int ri[8];
  DevLanes ln = {rv, ri, 0};
  const int b = (int)blockIdx.x;
  const long* d = desc + 4 * (long)b;
  long n = d[1], m = d[2];
  n = n < 0 ? 0 : (n > nmax ? nmax : n);  // never past the outputs or the workspace
  m = m < 0 ? 0 : (m > mmax ? mmax : m);
  char* p = ws + ws_stride * b;
  trk::SolveScratch s;
  s.u = (double*)p; p += (size_t)nmax * 8;
  s.v = (double*)p; p += (size_t)mmax * 8;
  s.minv = (double*)p; p += (size_t)mmax * 8;
  s.way = (int*)p; p += (size_t)mmax * 4;
  s.used = (int*)p;
  const trk::MatrixCost cost = {(const float*)d[0], d[3]};
  trk::solve(ln, (int)n, (int)m, cost, (double)thresh[b], s, row_to_col + (long)b * ldr, col_to_row + (long)b * ldc);
}

__global__ __launch_bounds__(TRK_THREADS) void bytetrack_update_kernel(int cap, int T, trk::Params P, const float* __restrict__ rows, const int* __restrict__ count,
                                                                        double* kf, int* si, float* sf, int* hdr, float* out_rows, int* out_ids,
                                                                        int* out_count, char* ws, size_t ws_stride) {
  extern __shared__ float lds[];
  __shared__ double rv[8];
  __shared__ int ri[8];
  DevLanes ln = {rv, ri, 0};
  const long b = (long)blockIdx.x;
  trk::Stream st;
  st.cap = cap;
  st.T = T;
  st.rows = rows + b * cap * 6;
  st.count = count[b];
  st.kf = kf + b * T * trk::KF_N;
  st.si = si + b * T * trk::SI_N;
  st.sf = sf + b * T * trk::SF_N;
  st.hdr = hdr + b * trk::H_N;
  st.out_rows = out_rows + b * cap * 8;
  st.out_ids = out_ids + b * cap;
  st.out_count = out_count + b;
  st.tbox = lds;
  st.dbox = lds + 4 * (size_t)T;
  st.dscore = st.dbox + 4 * (size_t)cap;
  st.dkind = (int*)(st.dscore + cap);
  trk::carve(st, ws + ws_stride * b);
  trk::frame_step(ln, P, st);
}

size_t la_stride(int nmax, int mmax) { return ((size_t)nmax * 8 + (size_t)mmax * 24 + 15) / 16 * 16; }
size_t bt_lds(int cap, int T) { return (size_t)T * 16 + (size_t)cap * 24; }

}  // namespace

extern "C" {

size_t ey_linear_assignment_workspace_bytes(int B, int nmax, int mmax) {
  if (B < 0 || nmax < 0 || mmax < 0) return 0;
  return la_stride(nmax, mmax) * (size_t)B + 16;
}

int ey_linear_assignment(int B, const long* desc, const float* thresh, int nmax, int mmax, int* row_to_col, int ldr, int* col_to_row, int ldc,
                         void* workspace, size_t workspace_bytes, ey_stream_t stream) {
  EY_CHECK(B >= 0 && nmax >= 0 && mmax >= 0, "ey_linear_assignment: bad sizes B=%d nmax=%d mmax=%d", B, nmax, mmax);
  if (B == 0) return EY_OK;
  EY_CHECK(desc && thresh && row_to_col && col_to_row && workspace, "ey_linear_assignment: null pointer");
  EY_CHECK(ldr >= nmax && ldc >= mmax, "ey_linear_assignment: output strides (%d, %d) below (nmax, mmax) = (%d, %d)", ldr, ldc, nmax, mmax);
  EY_CHECK(ey_aligned(workspace, 16) && workspace_bytes >= ey_linear_assignment_workspace_bytes(B, nmax, mmax),
           "ey_linear_assignment: workspace of %zu bytes, 16-byte aligned, needed", ey_linear_assignment_workspace_bytes(B, nmax, mmax));
  linear_assignment_kernel<<<B, TRK_THREADS, 0, (hipStream_t)stream>>>(desc, thresh, nmax, mmax, row_to_col, ldr, col_to_row, ldc, (char*)workspace,
                                                                         la_stride(nmax, mmax));
  EY_LAUNCH_CHECK("linear_assignment_kernel");
  return EY_OK;
}

size_t ey_bytetrack_workspace_bytes(int B, int cap, int max_tracks) {
  if (B < 0 || cap < 0 || max_tracks < 0) return 0;
  return trk::scratch_bytes(cap, max_tracks) * (size_t)B + 16;
}

int ey_bytetrack_update(int B, int cap, int max_tracks, float track_high_thresh, float track_low_thresh, float new_track_thresh, float match_thresh,
                        int max_time_lost, int fuse_score, const float* rows, const int* count, double* kf, int* slot_i, float* slot_f, int* hdr,
                        float* out_rows, int* out_ids, int* out_count, void* workspace, size_t workspace_bytes, ey_stream_t stream) {
  EY_CHECK(B >= 0 && cap >= 1 && max_tracks >= 1, "ey_bytetrack_update: bad sizes B=%d cap=%d max_tracks=%d", B, cap, max_tracks);
  if (B == 0) return EY_OK;
  EY_CHECK(rows && count && kf && slot_i && slot_f && hdr && out_rows && out_ids && out_count && workspace, "ey_bytetrack_update: null pointer");
  if (bt_lds(cap, max_tracks) > 64 * 1024)
    return ey_set_error(EY_EUNSUPPORTED, "ey_bytetrack_update: 16 * max_tracks + 24 * cap = %zu bytes of boxes exceed the 64 KiB of LDS a stream gets",
                        bt_lds(cap, max_tracks));
  EY_CHECK(ey_aligned(workspace, 16) && workspace_bytes >= ey_bytetrack_workspace_bytes(B, cap, max_tracks),
           "ey_bytetrack_update: workspace of %zu bytes, 16-byte aligned, needed", ey_bytetrack_workspace_bytes(B, cap, max_tracks));
  const trk::Params P = {track_high_thresh, track_low_thresh, new_track_thresh, match_thresh, max_time_lost, fuse_score != 0};
  bytetrack_update_kernel<<<B, TRK_THREADS, bt_lds(cap, max_tracks), (hipStream_t)stream>>>(cap, max_tracks, P, rows, count, kf, slot_i, slot_f, hdr, out_rows,
                                                                                           out_ids, out_count, (char*)workspace,
                                                                                           trk::scratch_bytes(cap, max_tracks));
  EY_LAUNCH_CHECK("bytetrack_update_kernel");
  return EY_OK;
}

}  // extern "C"
