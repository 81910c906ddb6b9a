// Pose estimation (reference ultralytics/nn/modules/head.py:402-451 Pose / kpts_decode, utils/metrics.py:156-175 kpt_iou).
//
// ey_kpts_decode_levels: the keypoint rows of the eval-mode prediction tensor, all pyramid levels in one launch.  A workgroup owns a tile
//   of consecutive anchors of one level of one image: the tile's pixels (contiguous in the NHWC map) are read along the channels with
//   16-byte loads (scalar loads for a window that is not 16-byte aligned) into LDS, and written back along the anchors, one channel row
//   of the tile per wave, so both sides run along their contiguous axis.
// ey_kpts_decode_rows: the keypoints of the kept rows only: one wave per NMS row, lanes along the nk channels of that anchor's pixel
//   (contiguous in the map and in the (B, max_det, nkpt, ndim) output).  Rows beyond the count, negative anchors and anchors outside
//   [0, A_total) are written as zeros; the pixel address is formed only after that check.
// ey_kpt_iou: OKS of every [ground truth x prediction] pair of a batch in one launch.  A workgroup owns 64 predictions x 16 ground truths
//   of one image: the predictions' x / y are staged in LDS (read contiguously), a wave walks its ground truths, a lane owns a prediction.
//
// Arithmetic: compiled without FMA contraction.  x = (v * 2 + gx) * stride has one rounding (v * 2 is exact, so is the product with a
// power-of-two stride), hence equals the reference's fp32 (v * 2.0 + (anchor - 0.5)) * stride bit for bit; exp is evaluated in double and
// rounded to fp32.  kp_decode() is the one place both decode kernels take a value from.
#include "common.h"

#define KP_MAXL 4
#define KP_MAXC 256   // nkpt * ndim
#define KP_THREADS 256
#define KP_IOU_MAXB 128
#define KP_IOU_MAXK 64
#define KP_IOU_TN 64  // predictions per workgroup (= lanes)
#define KP_IOU_TM 16  // ground truths per workgroup (4 per wave)
#define KP_EPS 1e-7f

__device__ __forceinline__ float kp_expf(float v) { return (float)exp((double)v); }
__device__ __forceinline__ float kp_sigmoidf(float v) { return 1.f / (1.f + kp_expf(-v)); }

// channel c = (keypoint, d) with d = c % ndim: x, y, visibility logit (ndim == 3)
__device__ __forceinline__ float kp_decode(float v, int d, float gx, float gy, float stride) {
  if (d == 0) return (v * 2.f + gx) * stride;
  if (d == 1) return (v * 2.f + gy) * stride;
  return kp_sigmoidf(v);
}

struct KpLevels {
  int nl;
  int H[KP_MAXL], W[KP_MAXL], cs[KP_MAXL], a_off[KP_MAXL], blk0[KP_MAXL + 1];
  float stride[KP_MAXL];
  const void* map[KP_MAXL];
};

// ---------------------------------------------------------------------------------------------------------------- full decode
// LDS tile [tp pixels][pitch], pitch = nk | 1 (odd: the anchor-major read-out walks the banks)
template <typename T>
__global__ __launch_bounds__(KP_THREADS) void kpts_decode_levels_kernel(KpLevels lv, int nk, int ndim, float* __restrict__ out, long out_bstride, int A, int vec, int tp) {
  extern __shared__ float kp_tile[];
  int l = 0;
#pragma unroll
  for (int i = 1; i < KP_MAXL; ++i)
    if (i < lv.nl && (int)blockIdx.x >= lv.blk0[i]) l = i;
  const int H = lv.H[l], W = lv.W[l], cs = lv.cs[l];
  const int HW = H * W;
  const int tiles = (HW + tp - 1) / tp;
  const int bi = (int)blockIdx.x - lv.blk0[l];
  const int b = bi / tiles, p0 = (bi - b * tiles) * tp;
  const int np = min(tp, HW - p0);
  const int pitch = nk | 1;
  const int tid = threadIdx.x;
  const T* src = (const T*)lv.map[l] + ((long)b * HW + p0) * cs;
  if (vec) {
    const int nch = (nk + 7) >> 3;
    for (int i = tid; i < np * nch; i += KP_THREADS) {
      const int p = i / nch, c0 = (i - p * nch) * 8;
      const T* s = src + (long)p * cs + c0;
      if (c0 + 8 <= nk) {
        Vec8<T> v;
        v.load(s);
#pragma unroll
        for (int j = 0; j < 8; ++j) kp_tile[p * pitch + c0 + j] = v.get(j);
      } else {  // the pixel's last, partial chunk: nothing beyond the window is read
        for (int j = 0; c0 + j < nk; ++j) kp_tile[p * pitch + c0 + j] = to_f(s[j]);
      }
    }
  } else {
    for (int i = tid; i < np * nk; i += KP_THREADS) {
      const int p = i / nk, c = i - p * nk;
      kp_tile[p * pitch + c] = to_f(src[(long)p * cs + c]);
    }
  }
  __syncthreads();
  const float stride = lv.stride[l];
  float* o = out + (long)b * out_bstride + lv.a_off[l] + p0;
  for (int i = tid; i < nk * tp; i += KP_THREADS) {
    const int c = i / tp, p = i - c * tp;
    if (p >= np) continue;
    const int a = p0 + p;
    const int gy = a / W, gx = a - gy * W;
    o[(long)c * A + p] = kp_decode(kp_tile[p * pitch + c], c % ndim, (float)gx, (float)gy, stride);
  }
}

// fills lv from the host arrays; returns EY_OK or the error already set
static int kp_levels(const char* who, int dtype, int B, int nlevels, const int* H, const int* W, const float* stride, const void* const* kpt, const int* kpt_cstride,
                     int nkpt, int ndim, int A_total, const int* a_off, KpLevels* lv, int* vec) {
  EY_CHECK(dtype == EY_F16 || dtype == EY_F32, "%s: bad dtype", who);
  if (nlevels < 1 || nlevels > KP_MAXL) return ey_set_error(EY_EUNSUPPORTED, "%s: %d levels (1 to %d are built)", who, nlevels, KP_MAXL);
  if (ndim != 2 && ndim != 3) return ey_set_error(EY_EUNSUPPORTED, "%s: ndim=%d (2 and 3 are built)", who, ndim);
  EY_CHECK(nkpt > 0, "%s: nkpt=%d", who, nkpt);
  if ((long)nkpt * ndim > KP_MAXC) return ey_set_error(EY_EUNSUPPORTED, "%s: nkpt*ndim=%ld (up to %d channels are built)", who, (long)nkpt * ndim, KP_MAXC);
  EY_CHECK(B > 0 && A_total > 0, "%s: B=%d A=%d", who, B, A_total);
  EY_CHECK(H && W && stride && kpt && kpt_cstride && a_off, "%s: null pointer", who);
  const int nk = nkpt * ndim;
  const size_t es = dtype == EY_F16 ? 2 : 4;
  lv->nl = nlevels;
  *vec = 1;
  for (int l = 0; l < KP_MAXL; ++l) {
    const bool on = l < nlevels;
    if (on) {
      EY_CHECK(kpt[l] && H[l] > 0 && W[l] > 0 && kpt_cstride[l] >= nk, "%s: level %d is empty", who, l);
      EY_CHECK(a_off[l] >= 0 && (long)a_off[l] + (long)H[l] * W[l] <= A_total, "%s: level %d anchors [%d, +%ld) exceed A=%d", who, l, a_off[l], (long)H[l] * W[l], A_total);
      if ((long)B * H[l] * W[l] * kpt_cstride[l] >= (1L << 31)) return ey_set_error(EY_EUNSUPPORTED, "%s: level %d too large", who, l);
      if (!ey_aligned(kpt[l], 16) || ((size_t)kpt_cstride[l] * es) % 16) *vec = 0;
    }
    lv->H[l] = on ? H[l] : 0; lv->W[l] = on ? W[l] : 0;
    lv->cs[l] = on ? kpt_cstride[l] : 0;
    lv->a_off[l] = on ? a_off[l] : 0;
    lv->stride[l] = on ? stride[l] : 0.f;
    lv->map[l] = on ? kpt[l] : nullptr;
    lv->blk0[l] = 0;
  }
  lv->blk0[KP_MAXL] = 0;
  return EY_OK;
}

extern "C" int ey_kpts_decode_levels(int dtype, int B, int nlevels, const int* H, const int* W, const float* stride, const void* const* kpt, const int* kpt_cstride,
                                     int nkpt, int ndim, float* out, long out_bstride, int A_total, const int* a_off, ey_stream_t stream) {
  KpLevels lv;
  int vec;
  const int rc = kp_levels("kpts_decode_levels", dtype, B, nlevels, H, W, stride, kpt, kpt_cstride, nkpt, ndim, A_total, a_off, &lv, &vec);
  if (rc != EY_OK) return rc;
  const int nk = nkpt * ndim;
  EY_CHECK(out && out_bstride >= (long)nk * A_total, "kpts_decode_levels: out=%p batch stride %ld (needs %ld)", (void*)out, out_bstride, (long)nk * A_total);
  if ((long)B * out_bstride >= (1L << 40)) return ey_set_error(EY_EUNSUPPORTED, "kpts_decode_levels: output too large");
  const int tp = nk <= 128 ? 64 : 32;  // anchors per tile: the LDS tile stays below 33 KiB
  long blocks = 0;
  for (int l = 0; l < KP_MAXL; ++l) {
    lv.blk0[l] = (int)blocks;
    if (l < nlevels) blocks += (long)B * ey_cdiv((long)H[l] * W[l], tp);
  }
  lv.blk0[KP_MAXL] = (int)blocks;
  if (blocks >= (1L << 31)) return ey_set_error(EY_EUNSUPPORTED, "kpts_decode_levels: %ld workgroups", blocks);
  const size_t lds = (size_t)tp * (nk | 1) * sizeof(float);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == EY_F16) hipLaunchKernelGGL((kpts_decode_levels_kernel<f16>), dim3((unsigned)blocks), dim3(KP_THREADS), lds, st, lv, nk, ndim, out, out_bstride, A_total, vec, tp);
  else hipLaunchKernelGGL((kpts_decode_levels_kernel<float>), dim3((unsigned)blocks), dim3(KP_THREADS), lds, st, lv, nk, ndim, out, out_bstride, A_total, vec, tp);
  EY_LAUNCH_CHECK("ey_kpts_decode_levels");
  return EY_OK;
}

// ---------------------------------------------------------------------------------------------------------------- kept rows
template <typename T>
__global__ __launch_bounds__(KP_THREADS) void kpts_decode_rows_kernel(KpLevels lv, int nk, int ndim, int A, int max_det, const int* __restrict__ index,
                                                                      const int* __restrict__ count, float* __restrict__ out) {
  const int b = blockIdx.y, lane = threadIdx.x & 63;
  const int r = blockIdx.x * (KP_THREADS / 64) + (threadIdx.x >> 6);
  if (r >= max_det) return;  // (wave-uniform; no barrier below)
  float* o = out + ((long)b * max_det + r) * nk;
  const int idx = r < count[b] ? index[(long)b * max_det + r] : -1;
  int l = -1;
  if (idx >= 0 && idx < A) {
#pragma unroll
    for (int i = 0; i < KP_MAXL; ++i)
      if (i < lv.nl && idx >= lv.a_off[i] && idx - lv.a_off[i] < lv.H[i] * lv.W[i]) l = i;
  }
  if (l < 0) {  // beyond the count, no anchor, or an anchor no level holds: zeros, and no address is formed from idx
    for (int c = lane; c < nk; c += 64) o[c] = 0.f;
    return;
  }
  const int W = lv.W[l];
  const int a = idx - lv.a_off[l];
  const int gy = a / W, gx = a - gy * W;
  const float stride = lv.stride[l];
  const T* src = (const T*)lv.map[l] + ((long)b * lv.H[l] * W + a) * lv.cs[l];
  for (int c = lane; c < nk; c += 64) o[c] = kp_decode(to_f(src[c]), c % ndim, (float)gx, (float)gy, stride);
}

extern "C" int ey_kpts_decode_rows(int dtype, int B, int nlevels, const int* H, const int* W, const float* stride, const void* const* kpt, const int* kpt_cstride,
                                   int nkpt, int ndim, int A_total, const int* a_off, int max_det, const int32_t* index, const int32_t* count, float* out,
                                   ey_stream_t stream) {
  KpLevels lv;
  int vec;
  const int rc = kp_levels("kpts_decode_rows", dtype, B, nlevels, H, W, stride, kpt, kpt_cstride, nkpt, ndim, A_total, a_off, &lv, &vec);
  if (rc != EY_OK) return rc;
  EY_CHECK(max_det > 0 && index && count && out, "kpts_decode_rows: max_det=%d or a null pointer", max_det);
  const int nk = nkpt * ndim;
  if (B > 65535 || (long)B * max_det * nk >= (1L << 40)) return ey_set_error(EY_EUNSUPPORTED, "kpts_decode_rows: output too large");
  const dim3 grid(ey_cdiv(max_det, KP_THREADS / 64), B);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == EY_F16) hipLaunchKernelGGL((kpts_decode_rows_kernel<f16>), grid, dim3(KP_THREADS), 0, st, lv, nk, ndim, A_total, max_det, index, count, out);
  else hipLaunchKernelGGL((kpts_decode_rows_kernel<float>), grid, dim3(KP_THREADS), 0, st, lv, nk, ndim, A_total, max_det, index, count, out);
  EY_LAUNCH_CHECK("ey_kpts_decode_rows");
  return EY_OK;
}

// ---------------------------------------------------------------------------------------------------------------- OKS
struct KpIouTab {
  int B;
  int pred_off[KP_IOU_MAXB + 1];
  int gt_off[KP_IOU_MAXB + 1];
  long out_off[KP_IOU_MAXB];
};

__global__ __launch_bounds__(KP_THREADS) void kpt_iou_kernel(KpIouTab tab, int K, int ndim, const float* __restrict__ pred, const float* __restrict__ gt,
                                                             const float* __restrict__ area, const float* __restrict__ sigma, float* __restrict__ out) {
  __shared__ float px[KP_IOU_MAXK * KP_IOU_TN], py[KP_IOU_MAXK * KP_IOU_TN];
  const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int N = tab.pred_off[b + 1] - tab.pred_off[b], M = tab.gt_off[b + 1] - tab.gt_off[b];
  if (N <= 0 || M <= 0) return;  // (workgroup-uniform)
  const int ntn = (N + KP_IOU_TN - 1) / KP_IOU_TN, ntm = (M + KP_IOU_TM - 1) / KP_IOU_TM;
  if ((int)blockIdx.x >= ntn * ntm) return;  // (workgroup-uniform)
  const int tm = blockIdx.x / ntn, tn = blockIdx.x - tm * ntn;
  const int n0 = tn * KP_IOU_TN, m0 = tm * KP_IOU_TM;
  const int nn = min(KP_IOU_TN, N - n0);
  // the tile's predictions are nn * K * ndim consecutive floats: read them in order, keep x and y keypoint-major
  const int per = K * ndim;
  const float* ps = pred + (long)(tab.pred_off[b] + n0) * per;
  for (int i = tid; i < nn * per; i += KP_THREADS) {
    const int n = i / per, rem = i - n * per;
    const int k = rem / ndim, d = rem - k * ndim;
    const float v = ps[i];
    if (d == 0) px[k * KP_IOU_TN + n] = v;
    else if (d == 1) py[k * KP_IOU_TN + n] = v;
  }
  __syncthreads();
  if (lane >= nn) return;
  for (int mi = wave; mi < KP_IOU_TM; mi += KP_THREADS / 64) {
    const int m = m0 + mi;
    if (m >= M) break;
    const float* g = gt + (long)(tab.gt_off[b] + m) * K * 3;
    const float ar = area[tab.gt_off[b] + m] + KP_EPS;
    float sum = 0.f;
    int vis = 0;
    for (int k = 0; k < K; ++k) {
      const float dx = g[k * 3] - px[k * KP_IOU_TN + lane], dy = g[k * 3 + 1] - py[k * KP_IOU_TN + lane];
      const float d = dx * dx + dy * dy;
      const float s2 = 2.f * sigma[k];
      const float e = d / (s2 * s2 * ar * 2.f);
      const bool on = g[k * 3 + 2] != 0.f;
      sum += kp_expf(-e) * (on ? 1.f : 0.f);
      vis += on ? 1 : 0;
    }
    out[tab.out_off[b] + (long)m * N + n0 + lane] = sum / ((float)vis + KP_EPS);
  }
}

extern "C" int ey_kpt_iou(int B, int K, int ndim, const float* pred, const int* pred_off, const float* gt, const int* gt_off, const float* area, const float* sigma,
                          const long* out_off, float* out, ey_stream_t stream) {
  EY_CHECK(B >= 0 && K > 0, "kpt_iou: B=%d K=%d", B, K);
  if (B > KP_IOU_MAXB) return ey_set_error(EY_EUNSUPPORTED, "kpt_iou: B=%d (up to %d images are built)", B, KP_IOU_MAXB);
  if (K > KP_IOU_MAXK) return ey_set_error(EY_EUNSUPPORTED, "kpt_iou: K=%d (up to %d keypoints are built)", K, KP_IOU_MAXK);
  if (ndim != 2 && ndim != 3) return ey_set_error(EY_EUNSUPPORTED, "kpt_iou: ndim=%d (2 and 3 are built)", ndim);
  if (B == 0) return EY_OK;
  EY_CHECK(pred_off && gt_off && out_off, "kpt_iou: null offset table");
  EY_CHECK(pred_off[0] == 0 && gt_off[0] == 0, "kpt_iou: pred_off[0]=%d gt_off[0]=%d must be 0", pred_off[0], gt_off[0]);
  KpIouTab tab;
  tab.B = B;
  tab.pred_off[0] = tab.gt_off[0] = 0;
  long tiles = 0;
  for (int b = 0; b < KP_IOU_MAXB; ++b) {
    const bool on = b < B;
    const long nb = on ? (long)pred_off[b + 1] - pred_off[b] : 0, mb = on ? (long)gt_off[b + 1] - gt_off[b] : 0;
    EY_CHECK(nb >= 0 && mb >= 0, "kpt_iou: offsets of image %d decrease", b);
    EY_CHECK(!(nb && mb) || out_off[b] >= 0, "kpt_iou: out_off[%d]=%ld", b, on ? out_off[b] : 0L);
    tab.pred_off[b + 1] = on ? pred_off[b + 1] : tab.pred_off[b];
    tab.gt_off[b + 1] = on ? gt_off[b + 1] : tab.gt_off[b];
    tab.out_off[b] = on ? out_off[b] : 0;
    if (nb && mb) {
      const long t = (long)ey_cdiv(nb, KP_IOU_TN) * ey_cdiv(mb, KP_IOU_TM);
      tiles = t > tiles ? t : tiles;
    }
  }
  if (tiles == 0) return EY_OK;
  if (tiles >= (1L << 31)) return ey_set_error(EY_EUNSUPPORTED, "kpt_iou: %ld tiles in one image", tiles);
  EY_CHECK(pred && gt && area && sigma && out, "kpt_iou: null pointer");
  hipLaunchKernelGGL(kpt_iou_kernel, dim3((unsigned)tiles, B), dim3(KP_THREADS), 0, (hipStream_t)stream, tab, K, ndim, pred, gt, area, sigma, out);
  EY_LAUNCH_CHECK("ey_kpt_iou");
  return EY_OK;
}
