// Mask polygons (reference utils/ops.py masks2segments: cv2.findContours(x, RETR_EXTERNAL, CHAIN_APPROX_SIMPLE) per mask): ey_mask_contours.
// The algorithm text is contours_core.inc.h, shared with the host program of the tests; this file gives it the workgroup's lanes
// (256 threads = 4 waves per mask) and launches it.  DESIGN.md section 7s.
#include "common.h"
#define CTR_HD __device__ __host__
#include "contours_core.inc.h"

#define CTR_THREADS 256

namespace {

struct DevLanes {
  int* r;  // LDS [2][4]: the waves' minima, double-buffered so that one barrier per imin is enough
  int par;
  __device__ int id() const { return (int)threadIdx.x; }
  __device__ int count() const { return (int)blockDim.x; }
  __device__ void barrier() { __syncthreads(); }
  __device__ int imin(int v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) {
      const int ov = __shfl_xor(v, o, 64);
      v = ov < v ? ov : v;
    }
    const int w = (int)threadIdx.x >> 6, nw = (int)blockDim.x >> 6;
    if ((threadIdx.x & 63) == 0) r[par * 4 + w] = v;
    __syncthreads();
    v = r[par * 4];
    for (int k = 1; k < nw; ++k) {
      const int ov = r[par * 4 + k];
      v = ov < v ? ov : v;
    }
    par ^= 1;
    return v;
  }
};

__device__ inline int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__global__ __launch_bounds__(CTR_THREADS) void mask_contours_kernel(int h, int w, const unsigned char* __restrict__ masks, const int* __restrict__ windows,
                                                                     int ccap, int vcap, int* lens, int* verts, int* info, signed char* ws, size_t ws_stride) {
  __shared__ int red[8];
  __shared__ int sh[1];
  DevLanes ln = {red, 0};
  const size_t b = blockIdx.x;
  ctr::Job J;
  J.mask = masks + b * (size_t)h * (size_t)w;
  J.ld = w;
  int x0 = 0, y0 = 0, x1 = w, y1 = h;
  if (windows) {  // never outside the mask, whatever the caller computed
    x0 = clampi(windows[4 * b], 0, w);
    y0 = clampi(windows[4 * b + 1], 0, h);
    x1 = clampi(windows[4 * b + 2], x0, w);
    y1 = clampi(windows[4 * b + 3], y0, h);
  }
  J.x0 = x0;
  J.y0 = y0;
  J.ww = x1 - x0;
  J.wh = y1 - y0;
  J.lbl = ws + ws_stride * b;
  J.ccap = ccap;
  J.vcap = vcap;
  J.lens = lens + b * (size_t)ccap;
  J.verts = verts + 2 * b * (size_t)vcap;
  J.info = info + ctr::I_N * b;
  J.sh = sh;
  ctr::contours(ln, J);
}

}  // namespace

extern "C" {

size_t ey_mask_contours_workspace_bytes(int n, int h, int w) {
  if (n < 0 || h < 1 || w < 1) return 0;
  return ctr::plane_bytes(h, w) * (size_t)n + 16;
}

int ey_mask_contours(int n, int h, int w, const uint8_t* masks, const int* windows, int contour_cap, int vertex_cap, int* lens, int* verts, int* info,
                     void* workspace, size_t workspace_bytes, ey_stream_t stream) {
  EY_CHECK(n >= 0 && h >= 1 && w >= 1, "ey_mask_contours: bad sizes n=%d h=%d w=%d", n, h, w);
  EY_CHECK(((size_t)h + 2) * ((size_t)w + 2) <= ((size_t)1 << 30), "ey_mask_contours: a mask of %d x %d pixels is past the 2^30 labels a plane indexes", h, w);
  EY_CHECK(contour_cap >= 1 && vertex_cap >= 1, "ey_mask_contours: capacities (%d contours, %d vertices) below 1", contour_cap, vertex_cap);
  if (n == 0) return EY_OK;
  EY_CHECK(masks && lens && verts && info && workspace, "ey_mask_contours: null pointer");
  EY_CHECK(ey_aligned(workspace, 16) && workspace_bytes >= ey_mask_contours_workspace_bytes(n, h, w),
           "ey_mask_contours: workspace of %zu bytes, 16-byte aligned, needed", ey_mask_contours_workspace_bytes(n, h, w));
  mask_contours_kernel<<<n, CTR_THREADS, 0, (hipStream_t)stream>>>(h, w, masks, windows, contour_cap, vertex_cap, lens, verts, info, (signed char*)workspace,
                                                                   ctr::plane_bytes(h, w));
  EY_LAUNCH_CHECK("mask_contours_kernel");
  return EY_OK;
}

}  // extern "C"
