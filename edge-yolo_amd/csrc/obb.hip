// Oriented boxes (reference ultralytics/nn/modules/head.py:372-399 OBB, utils/tal.py:366-385 dist2rbox, utils/metrics.py:178-195,244-275
// _get_covariance_matrix / batch_probiou, utils/ops.py:146-164,230-297 nms_rotated / non_max_suppression(rotated=True)).
//
// ey_obb_decode_levels: thread = one anchor of one pyramid level: DFL expectation, dist2rbox with the anchor's angle, class sigmoids and
//   the angle row, all levels in one launch, written coalesced to pred (B, 4+nc+1, A).
// ey_probiou: the (N, M) ProbIoU matrix; a workgroup owns 256 columns x 64 rows, the rows' Gaussians staged in LDS.
// ey_nms_rotated: fast-NMS on ProbIoU, five launches, no host synchronisation:
//   obb_init    counters = 0, column minima = +inf
//   obb_score   per anchor the best class; candidates (score > conf, class filter) are compacted with one atomic slot each:
//               key = score_bits << 32 | ~anchor, unique per image, so the slot order does not matter
//   obb_rank    rank of a candidate = number of larger keys (all pairs of 8-byte compares through LDS, no sort): the rank is the
//               position in score order (ties: lower anchor first); ranks below max_nms write the candidate's Gaussian record there
//   obb_pair    grid = column tiles x row chunks x images over the strict upper triangle: a thread owns a column j, walks the rows
//               i < j of its chunk from LDS and keeps the MINIMUM Bhattacharyya distance bd(i, j); one atomic min per column and chunk
//   obb_resolve one workgroup per image: iou = 1 - sqrt(1 - exp(-bd_min) + eps) per column, the keep rule, a block scan for the output
//               position, the first max_det kept rows
// The reference takes max_i iou(i, j); iou is a non-increasing function of the clamped distance (exp, the subtraction, sqrt and the
// final subtraction are each monotone in fp32), so max_i iou(i, j) = iou(min_i bd(i, j)) bit for bit and the exp / sqrt tail runs once
// per column instead of once per pair.  The minimum is order independent: the result is the same run to run.
// ey_nms_rotated_ml: the validation regime (every (anchor, class) score above conf is a candidate): a radix select cuts them to max_nms, the
//   survivors go through obb_pair and obb_resolve as above; see the section at the end of the file.
// ey_probiou_batch: ey_probiou's tile body for every image of a batch in one launch, through per-image offset tables.
//
// Arithmetic: this file is compiled without FMA contraction and follows the reference's fp32 expressions operation by operation
// (division and sqrt are IEEE here).  exp / log / sin / cos are evaluated in double and rounded to fp32, i.e. correctly rounded but for
// the rare double rounding, so the chain is an IEEE fp32 evaluation of the reference's formula.
#include "common.h"

#define OBB_EPS 1e-7f
#define OBB_MAXL 4
#define OBB_DEC 128    // anchors per decode workgroup
#define OBB_TILE 256   // columns per workgroup (= threads) of the pair and ProbIoU kernels
#define OBB_ROWS 256   // rows per chunk of the pair kernel
#define OBB_PROWS 64   // rows per workgroup of the ProbIoU kernel
#define OBB_INF 0x7f800000u  // column minimum "no earlier row"; 0 = a NaN distance was seen (real distances are >= eps > 0)

__device__ __forceinline__ float obb_expf(float v) { return (float)exp((double)v); }
__device__ __forceinline__ float obb_logf(float v) { return (float)log((double)v); }
__device__ __forceinline__ float obb_sinf(float v) { return (float)sin((double)v); }
__device__ __forceinline__ float obb_cosf(float v) { return (float)cos((double)v); }
__device__ __forceinline__ float obb_sigmoidf(float v) { return 1.f / (1.f + obb_expf(-v)); }

// ---------------------------------------------------------------------------------------------------------------- ProbIoU
// centre + covariance terms of the box's Gaussian (_get_covariance_matrix) + d = clamp(a b - c^2, 0), computed once per box
struct ObbGauss {
  float x, y, a, b, c, d;
};

__device__ __forceinline__ ObbGauss obb_gauss(float x, float y, float w, float h, float r) {
  const float a = w * w / 12.f, b = h * h / 12.f;
  const float cs = obb_cosf(r), sn = obb_sinf(r);
  const float cos2 = cs * cs, sin2 = sn * sn;
  ObbGauss g;
  g.x = x;
  g.y = y;
  g.a = a * cos2 + b * sin2;
  g.b = a * sin2 + b * cos2;
  g.c = (a - b) * cs * sn;
  g.d = fmaxf(g.a * g.b - g.c * g.c, 0.f);
  return g;
}

// The pair arithmetic of batch_probiou (p = a row of obb1, q = a column of obb2) up to bd = (t1 + t2 + t3).clamp(eps, 100); NaN stays NaN.
__device__ __forceinline__ float obb_pair_bd(const ObbGauss& p, const ObbGauss& q) {
  const float sa = p.a + q.a, sb = p.b + q.b, sc = p.c + q.c;
  const float dy = p.y - q.y, dx = p.x - q.x;
  const float det = sa * sb - sc * sc;
  const float den = det + OBB_EPS;
  const float t1 = ((sa * (dy * dy) + sb * (dx * dx)) / den) * 0.25f;
  const float t2 = ((sc * (q.x - p.x) * dy) / den) * 0.5f;
  const float t3 = obb_logf(det / (4.f * sqrtf(p.d * q.d) + OBB_EPS) + OBB_EPS) * 0.5f;
  const float bd = t1 + t2 + t3;
  return bd != bd ? bd : fminf(fmaxf(bd, OBB_EPS), 100.f);
}
// ... and its tail: 1 - sqrt(1 - exp(-bd) + eps)
__device__ __forceinline__ float obb_bd_iou(float bd) { return 1.f - sqrtf(1.f - obb_expf(-bd) + OBB_EPS); }
__device__ __forceinline__ float obb_pair_iou(const ObbGauss& p, const ObbGauss& q) { return obb_bd_iou(obb_pair_bd(p, q)); }

// one workgroup's share of an (N, M) matrix: column tile bx, row chunk by (both inside the matrix); rows = the LDS stage of the chunk's Gaussians
__device__ __forceinline__ void obb_probiou_tile(int N, int M, const float* __restrict__ o1, const float* __restrict__ o2, float* __restrict__ out, int bx, int by, ObbGauss* rows) {
  const int tid = threadIdx.x;
  const int i0 = by * OBB_PROWS, j = bx * OBB_TILE + tid;
  const int nr = min(OBB_PROWS, N - i0);
  if (tid < nr) {
    const float* p = o1 + (long)(i0 + tid) * 5;
    rows[tid] = obb_gauss(p[0], p[1], p[2], p[3], p[4]);
  }
  __syncthreads();
  if (j >= M) return;
  const float* p = o2 + (long)j * 5;
  const ObbGauss q = obb_gauss(p[0], p[1], p[2], p[3], p[4]);
  for (int i = 0; i < nr; ++i) out[(long)(i0 + i) * M + j] = obb_pair_iou(rows[i], q);
}

__global__ __launch_bounds__(OBB_TILE) void obb_probiou_kernel(int N, int M, const float* __restrict__ o1, const float* __restrict__ o2, float* __restrict__ out) {
  __shared__ ObbGauss rows[OBB_PROWS];
  obb_probiou_tile(N, M, o1, o2, out, blockIdx.x, blockIdx.y, rows);
}

// every image's [ground truth x prediction] matrix in one launch: grid.y = image, grid.x = the image's tiles (column tile fastest)
#define OBB_PB_MAXB 128
struct ObbPairTab {
  int pred_off[OBB_PB_MAXB + 1];
  int gt_off[OBB_PB_MAXB + 1];
  long out_off[OBB_PB_MAXB];
};
__global__ __launch_bounds__(OBB_TILE) void obb_probiou_batch_kernel(ObbPairTab tab, const float* __restrict__ pred, const float* __restrict__ gt, float* __restrict__ out) {
  __shared__ ObbGauss rows[OBB_PROWS];
  const int b = blockIdx.y;
  const int N = tab.pred_off[b + 1] - tab.pred_off[b], M = tab.gt_off[b + 1] - tab.gt_off[b];
  if (N <= 0 || M <= 0) return;  // (workgroup-uniform)
  const int ntx = (N + OBB_TILE - 1) / OBB_TILE, nty = (M + OBB_PROWS - 1) / OBB_PROWS;
  if ((int)blockIdx.x >= ntx * nty) return;  // (workgroup-uniform)
  const int by = blockIdx.x / ntx, bx = blockIdx.x - by * ntx;
  obb_probiou_tile(M, N, gt + (long)tab.gt_off[b] * 5, pred + (long)tab.pred_off[b] * 5, out + tab.out_off[b], bx, by, rows);
}

extern "C" int ey_probiou_batch(int B, const float* pred, const int* pred_off, const float* gt, const int* gt_off, float* out, const long* out_off, ey_stream_t stream) {
  EY_CHECK(B >= 0, "probiou_batch: B=%d", B);
  if (B > OBB_PB_MAXB) return ey_set_error(EY_EUNSUPPORTED, "probiou_batch: B=%d (up to %d images are built)", B, OBB_PB_MAXB);
  if (B == 0) return EY_OK;
  EY_CHECK(pred_off && gt_off && out_off, "probiou_batch: null offset table");
  EY_CHECK(pred_off[0] == 0 && gt_off[0] == 0, "probiou_batch: pred_off[0]=%d gt_off[0]=%d must be 0", pred_off[0], gt_off[0]);
  ObbPairTab tab;
  tab.pred_off[0] = tab.gt_off[0] = 0;
  long tiles = 0;
  for (int b = 0; b < OBB_PB_MAXB; ++b) {
    const bool on = b < B;
    const long nb = on ? (long)pred_off[b + 1] - pred_off[b] : 0, mb = on ? (long)gt_off[b + 1] - gt_off[b] : 0;
    EY_CHECK(nb >= 0 && mb >= 0, "probiou_batch: offsets of image %d decrease", b);
    EY_CHECK(!(nb && mb) || out_off[b] >= 0, "probiou_batch: out_off[%d]=%ld", b, on ? out_off[b] : 0L);
    tab.pred_off[b + 1] = on ? pred_off[b + 1] : tab.pred_off[b];
    tab.gt_off[b + 1] = on ? gt_off[b + 1] : tab.gt_off[b];
    tab.out_off[b] = on ? out_off[b] : 0;
    if (nb && mb) {
      const long t = (long)ey_cdiv(nb, OBB_TILE) * ey_cdiv(mb, OBB_PROWS);
      tiles = t > tiles ? t : tiles;
    }
  }
  if (tiles == 0) return EY_OK;
  if (tiles >= (1L << 31)) return ey_set_error(EY_EUNSUPPORTED, "probiou_batch: %ld tiles in one image", tiles);
  EY_CHECK(pred && gt && out, "probiou_batch: null pointer");
  hipLaunchKernelGGL(obb_probiou_batch_kernel, dim3((unsigned)tiles, B), dim3(OBB_TILE), 0, (hipStream_t)stream, tab, pred, gt, out);
  EY_LAUNCH_CHECK("ey_probiou_batch");
  return EY_OK;
}

extern "C" int ey_probiou(int N, int M, const float* obb1, const float* obb2, float* out, ey_stream_t stream) {
  EY_CHECK(N >= 0 && M >= 0, "probiou: N=%d M=%d", N, M);
  if (N == 0 || M == 0) return EY_OK;
  EY_CHECK(obb1 && obb2 && out, "probiou: null pointer");
  if (ey_cdiv(N, OBB_PROWS) > 65535) return ey_set_error(EY_EUNSUPPORTED, "probiou: N=%d (up to %d rows are built)", N, 65535 * OBB_PROWS);
  hipLaunchKernelGGL(obb_probiou_kernel, dim3(ey_cdiv(M, OBB_TILE), ey_cdiv(N, OBB_PROWS)), dim3(OBB_TILE), 0, (hipStream_t)stream, N, M, obb1, obb2, out);
  EY_LAUNCH_CHECK("ey_probiou");
  return EY_OK;
}

// ---------------------------------------------------------------------------------------------------------------- head decode
struct ObbLevels {
  int nl;
  int H[OBB_MAXL], W[OBB_MAXL], boxCs[OBB_MAXL], clsCs[OBB_MAXL], angCs[OBB_MAXL], a_off[OBB_MAXL], blk0[OBB_MAXL + 1];
  float stride[OBB_MAXL];
  const void* box[OBB_MAXL];
  const void* cls[OBB_MAXL];
  const void* ang[OBB_MAXL];
};

template <typename T>
__global__ __launch_bounds__(OBB_DEC) void obb_decode_kernel(int B, ObbLevels lv, int nc, float* __restrict__ pred, int A, int vec) {
  int l = 0;
#pragma unroll
  for (int i = 1; i < OBB_MAXL; ++i)
    if (i < lv.nl && (int)blockIdx.x >= lv.blk0[i]) l = i;
  const int H = lv.H[l], W = lv.W[l];
  const long HW = (long)H * W;
  const long idx = (long)((int)blockIdx.x - lv.blk0[l]) * OBB_DEC + threadIdx.x;
  if (idx >= (long)B * HW) return;
  const int b = (int)(idx / HW), a = (int)(idx - (long)b * HW);
  const int ay = a / W, ax = a - ay * W;
  const float stride = lv.stride[l];
  const T* bp = (const T*)lv.box[l] + idx * lv.boxCs[l];
  const T* cp = (const T*)lv.cls[l] + idx * lv.clsCs[l];
  // DFL (block.py:87-90): softmax over the 16 bins of each side, expectation with the weights 0..15
  float dist[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    float v[16];
    if (vec) {
      Vec8<T> v0, v1;
      v0.load(bp + s * 16);
      v1.load(bp + s * 16 + 8);
#pragma unroll
      for (int i = 0; i < 8; ++i) { v[i] = v0.get(i); v[8 + i] = v1.get(i); }
    } else {
#pragma unroll
      for (int i = 0; i < 16; ++i) v[i] = to_f(bp[s * 16 + i]);
    }
    float mx = v[0];
#pragma unroll
    for (int i = 1; i < 16; ++i) mx = fmaxf(mx, v[i]);
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) { v[i] = obb_expf(v[i] - mx); sum += v[i]; }
    float e = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) e += (v[i] / sum) * (float)i;
    dist[s] = e;
  }
  // angle = (sigmoid(logit) - 0.25) * pi (head.py:388); dist2rbox (tal.py:379-385): lt = dist[0:2], rb = dist[2:4]
  const float ang = (obb_sigmoidf(to_f(((const T*)lv.ang[l])[idx * lv.angCs[l]])) - 0.25f) * 3.14159265358979323846f;
  const float cs = obb_cosf(ang), sn = obb_sinf(ang);
  const float xf = (dist[2] - dist[0]) / 2.f, yf = (dist[3] - dist[1]) / 2.f;
  const float x = xf * cs - yf * sn + ((float)ax + 0.5f), y = xf * sn + yf * cs + ((float)ay + 0.5f);
  float* pp = pred + (long)b * (4 + nc + 1) * A + lv.a_off[l] + a;
  pp[0] = x * stride;
  pp[(long)A] = y * stride;
  pp[2L * A] = (dist[0] + dist[2]) * stride;
  pp[3L * A] = (dist[1] + dist[3]) * stride;
  for (int c = 0; c < nc; ++c) pp[(long)(4 + c) * A] = obb_sigmoidf(to_f(cp[c]));
  pp[(long)(4 + nc) * A] = ang;
}

extern "C" int ey_obb_decode_levels(int dtype, int B, int nlevels, const int* H, const int* W, const float* stride, const void* const* box, const int* box_cstride,
                                    const void* const* cls, const int* cls_cstride, const void* const* angle, const int* angle_cstride, int nc, float* pred,
                                    int A_total, const int* a_off, ey_stream_t stream) {
  EY_CHECK(dtype == EY_F16 || dtype == EY_F32, "obb_decode: bad dtype");
  if (nlevels < 1 || nlevels > OBB_MAXL) return ey_set_error(EY_EUNSUPPORTED, "obb_decode: %d levels (1 to %d are built)", nlevels, OBB_MAXL);
  EY_CHECK(B > 0 && nc > 0 && A_total > 0, "obb_decode: B=%d nc=%d A=%d", B, nc, A_total);
  EY_CHECK(H && W && stride && box && box_cstride && cls && cls_cstride && angle && angle_cstride && pred && a_off, "obb_decode: null pointer");
  if ((long)B * (4 + nc + 1) * A_total >= (1L << 40)) return ey_set_error(EY_EUNSUPPORTED, "obb_decode: prediction tensor too large");
  const size_t es = dtype == EY_F16 ? 2 : 4;
  ObbLevels lv;
  lv.nl = nlevels;
  int vec = 1;
  long blocks = 0;
  for (int l = 0; l < OBB_MAXL; ++l) {
    const bool on = l < nlevels;
    if (on) {
      EY_CHECK(box[l] && cls[l] && angle[l] && H[l] > 0 && W[l] > 0 && box_cstride[l] >= 64 && cls_cstride[l] >= nc && angle_cstride[l] >= 1, "obb_decode: level %d is empty", l);
      EY_CHECK(a_off[l] >= 0 && (long)a_off[l] + (long)H[l] * W[l] <= A_total, "obb_decode: level %d anchors [%d, +%ld) exceed A=%d", l, a_off[l], (long)H[l] * W[l], A_total);
      const long npix = (long)B * H[l] * W[l];
      if (npix * box_cstride[l] >= (1L << 31) || npix * cls_cstride[l] >= (1L << 31) || npix * angle_cstride[l] >= (1L << 31)) return ey_set_error(EY_EUNSUPPORTED, "obb_decode: level %d too large", l);
      if (!ey_aligned(box[l], 16) || ((size_t)box_cstride[l] * es) % 16) vec = 0;
    }
    lv.H[l] = on ? H[l] : 0; lv.W[l] = on ? W[l] : 0;
    lv.boxCs[l] = on ? box_cstride[l] : 0; lv.clsCs[l] = on ? cls_cstride[l] : 0; lv.angCs[l] = on ? angle_cstride[l] : 0;
    lv.a_off[l] = on ? a_off[l] : 0;
    lv.stride[l] = on ? stride[l] : 0.f;
    lv.box[l] = on ? box[l] : nullptr; lv.cls[l] = on ? cls[l] : nullptr; lv.ang[l] = on ? angle[l] : nullptr;
    lv.blk0[l] = (int)blocks;
    if (on) blocks += ey_cdiv((long)B * H[l] * W[l], OBB_DEC);
  }
  lv.blk0[OBB_MAXL] = (int)blocks;
  if (blocks >= (1L << 31)) return ey_set_error(EY_EUNSUPPORTED, "obb_decode: %ld workgroups", blocks);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == EY_F16) hipLaunchKernelGGL((obb_decode_kernel<f16>), dim3((unsigned)blocks), dim3(OBB_DEC), 0, st, B, lv, nc, pred, A_total, vec);
  else hipLaunchKernelGGL((obb_decode_kernel<float>), dim3((unsigned)blocks), dim3(OBB_DEC), 0, st, B, lv, nc, pred, A_total, vec);
  EY_LAUNCH_CHECK("ey_obb_decode_levels");
  return EY_OK;
}

// ---------------------------------------------------------------------------------------------------------------- rotated NMS
// workspace, every part 256-byte aligned: counters [B] | keys [B][A] u64 | class ids [B][A] | records [B][maxn][8] | sorted class ids [B][maxn] |
// column minima [B][maxn], maxn = min(A, max_nms).  Record = x + c max_wh, y + c max_wh, a, b, c, d, anchor, score bits.
struct ObbWs {
  int* cnt;
  unsigned long long* keys;
  int* ccls;
  float* rec;
  int* scls;
  unsigned* colmin;
  int maxn;
};
static inline size_t obb_al(size_t n) { return (n + 255) & ~(size_t)255; }
static size_t obb_ws_layout(int B, int A, int max_nms, char* base, ObbWs* ws) {
  const size_t maxn = (size_t)(A < max_nms ? A : max_nms);
  size_t off = 0;
  const size_t o_cnt = off; off += obb_al((size_t)B * 4);
  const size_t o_keys = off; off += obb_al((size_t)B * A * 8);
  const size_t o_ccls = off; off += obb_al((size_t)B * A * 4);
  const size_t o_rec = off; off += obb_al((size_t)B * maxn * 32);
  const size_t o_scls = off; off += obb_al((size_t)B * maxn * 4);
  const size_t o_min = off; off += obb_al((size_t)B * maxn * 4);
  if (ws) {
    ws->cnt = (int*)(base + o_cnt);
    ws->keys = (unsigned long long*)(base + o_keys);
    ws->ccls = (int*)(base + o_ccls);
    ws->rec = (float*)(base + o_rec);
    ws->scls = (int*)(base + o_scls);
    ws->colmin = (unsigned*)(base + o_min);
    ws->maxn = (int)maxn;
  }
  return off;
}
extern "C" size_t ey_nms_rotated_workspace_bytes(int B, int A, int max_nms) {
  if (B <= 0 || A <= 0 || max_nms <= 0) return 0;
  return obb_ws_layout(B, A, max_nms, nullptr, nullptr);
}

__global__ __launch_bounds__(256) void obb_init_kernel(int B, ObbWs ws) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < B) ws.cnt[i] = 0;
  if (i < (long)B * ws.maxn) ws.colmin[i] = OBB_INF;
}

__global__ __launch_bounds__(256) void obb_score_kernel(int nc, int A, const float* __restrict__ pred, float conf, const uint8_t* __restrict__ mask, ObbWs ws) {
  const int b = blockIdx.y, a = blockIdx.x * 256 + threadIdx.x;
  if (a >= A) return;
  const float* sp = pred + (long)b * (4 + nc + 1) * A + 4L * A + a;
  float best = sp[0];
  int bi = 0;
  for (int c = 1; c < nc; ++c) {
    const float s = sp[(long)c * A];
    if (s > best) { best = s; bi = c; }  // first maximal index (ops.py:274)
  }
  if (best > conf && (!mask || mask[bi])) {
    const int slot = atomicAdd(&ws.cnt[b], 1);
    ws.keys[(long)b * A + slot] = ((unsigned long long)__float_as_uint(best) << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)a);
    ws.ccls[(long)b * A + slot] = bi;
  }
}

// number of the n keys that are larger than `key` (the whole workgroup of 256 calls it; keys are unique, so that is the key's position)
__device__ __forceinline__ int obb_rank_of(const unsigned long long* __restrict__ keys, int n, unsigned long long key, unsigned long long* tile, int tid) {
  int rank = 0;
  for (int t0 = 0; t0 < n; t0 += 256) {
    __syncthreads();
    tile[tid] = t0 + tid < n ? keys[t0 + tid] : 0ull;  // (0 is larger than no key)
    __syncthreads();
#pragma unroll 8
    for (int k = 0; k < 256; ++k) rank += tile[k] > key ? 1 : 0;
  }
  return rank;
}

// the record of the candidate (anchor a, class cls, score bits) at position `rank` of image b
__device__ __forceinline__ void obb_write_record(int b, int nc, int A, const float* __restrict__ pred, float cls_off, const ObbWs& ws, int rank, int a, int cls, unsigned score_bits) {
  const float* pp = pred + (long)b * (4 + nc + 1) * A + a;
  const float c = (float)cls * cls_off;  // x[:, 5:6] * (0 if agnostic else max_wh), added in fp32 (ops.py:289-292)
  const ObbGauss g = obb_gauss(pp[0] + c, pp[(long)A] + c, pp[2L * A], pp[3L * A], pp[(long)(4 + nc) * A]);
  float* r = ws.rec + ((long)b * ws.maxn + rank) * 8;
  *reinterpret_cast<f32x4*>(r) = f32x4{g.x, g.y, g.a, g.b};
  *reinterpret_cast<f32x4*>(r + 4) = f32x4{g.c, g.d, __int_as_float(a), __uint_as_float(score_bits)};
  ws.scls[(long)b * ws.maxn + rank] = cls;
}

__global__ __launch_bounds__(256) void obb_rank_kernel(int nc, int A, const float* __restrict__ pred, int max_nms, float cls_off, ObbWs ws) {
  __shared__ unsigned long long tile[256];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int n = ws.cnt[b];
  if ((int)blockIdx.x * 256 >= n) return;  // (workgroup-uniform)
  const unsigned long long* keys = ws.keys + (long)b * A;
  const int j = blockIdx.x * 256 + tid;
  const unsigned long long key = j < n ? keys[j] : ~0ull;
  const int rank = obb_rank_of(keys, n, key, tile, tid);
  if (j >= n || rank >= max_nms) return;
  const int a = (int)(0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull));
  obb_write_record(b, nc, A, pred, cls_off, ws, rank, a, ws.ccls[(long)b * A + j], (unsigned)(key >> 32));
}

__global__ __launch_bounds__(OBB_TILE) void obb_pair_kernel(int max_nms, ObbWs ws) {
  __shared__ float sx[OBB_ROWS], sy[OBB_ROWS], sa[OBB_ROWS], sb[OBB_ROWS], sc[OBB_ROWS], sd[OBB_ROWS];
  const int b = blockIdx.z, tid = threadIdx.x;
  const int n = min(ws.cnt[b], max_nms);
  const int col0 = blockIdx.x * OBB_TILE, row0 = blockIdx.y * OBB_ROWS;
  // columns col0 .. min(col0 + TILE, n) - 1 meet rows row0 .. only where a row index is below a column index
  if (col0 >= n || row0 >= min(col0 + OBB_TILE, n) - 1) return;  // (workgroup-uniform)
  const float* rec = ws.rec + (long)b * ws.maxn * 8;
  const int nr = min(OBB_ROWS, n - row0);
  if (tid < nr) {  // (OBB_ROWS == OBB_TILE: one row per thread)
    const f32x4 u = *reinterpret_cast<const f32x4*>(rec + (long)(row0 + tid) * 8);
    const f32x4 v = *reinterpret_cast<const f32x4*>(rec + (long)(row0 + tid) * 8 + 4);
    sx[tid] = u[0]; sy[tid] = u[1]; sa[tid] = u[2]; sb[tid] = u[3]; sc[tid] = v[0]; sd[tid] = v[1];
  }
  __syncthreads();
  const int j = col0 + tid;
  const int iend = min(nr, j - row0);  // rows i < j of this chunk
  if (j >= n || iend <= 0) return;
  const f32x4 u = *reinterpret_cast<const f32x4*>(rec + (long)j * 8);
  const f32x4 v = *reinterpret_cast<const f32x4*>(rec + (long)j * 8 + 4);
  const ObbGauss q = {u[0], u[1], u[2], u[3], v[0], v[1]};
  float m = __uint_as_float(OBB_INF);
  bool nan = false;
  for (int i = 0; i < iend; ++i) {
    const ObbGauss p = {sx[i], sy[i], sa[i], sb[i], sc[i], sd[i]};
    const float bd = obb_pair_bd(p, q);
    nan |= bd != bd;
    m = fminf(m, bd);
  }
  atomicMin(&ws.colmin[(long)b * ws.maxn + j], nan ? 0u : __float_as_uint(m));  // (positive floats order as their bits)
}

__global__ __launch_bounds__(1024) void obb_resolve_kernel(int nc, int A, const float* __restrict__ pred, float iou_thres, int max_det, int max_nms, ObbWs ws,
                                                           float* __restrict__ out_rows, int* __restrict__ out_count, int* __restrict__ out_index) {
  __shared__ int wsum[16];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = min(ws.cnt[b], max_nms);
  const float* rec = ws.rec + (long)b * ws.maxn * 8;
  float* orow = out_rows + (long)b * max_det * 7;
  int kept = 0;
  for (int base = 0; base < n && kept < max_det; base += 1024) {  // (kept is workgroup-uniform)
    const int j = base + tid;
    bool keep = false;
    if (j < n) {
      const unsigned u = ws.colmin[(long)b * ws.maxn + j];
      // column maximum over the triu-zeroed matrix: max(0, max_{i<j} iou); a NaN in the column keeps nothing (NaN < thr is false)
      if (u == OBB_INF) keep = 0.f < iou_thres;
      else if (u != 0u) keep = fmaxf(obb_bd_iou(__uint_as_float(u)), 0.f) < iou_thres;
    }
    const unsigned long long bal = __ballot(keep);
    if (lane == 0) wsum[wave] = __popcll(bal);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < 16; ++w) {
      before += w < wave ? wsum[w] : 0;
      total += wsum[w];
    }
    __syncthreads();
    const int pos = kept + before + __popcll(bal & ((1ull << lane) - 1ull));
    if (keep && pos < max_det) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(rec + (long)j * 8 + 4);
      const int a = __float_as_int(v[2]);
      const float* pp = pred + (long)b * (4 + nc + 1) * A + a;
      float* o = orow + (long)pos * 7;
      o[0] = pp[0]; o[1] = pp[(long)A]; o[2] = pp[2L * A]; o[3] = pp[3L * A];
      o[4] = v[3];
      o[5] = (float)ws.scls[(long)b * ws.maxn + j];
      o[6] = pp[(long)(4 + nc) * A];
      if (out_index) out_index[(long)b * max_det + pos] = a;
    }
    kept += total;
  }
  const int count = min(kept, max_det);
  if (tid == 0) out_count[b] = count;
  for (int p = count + tid; p < max_det; p += 1024) {
#pragma unroll
    for (int e = 0; e < 7; ++e) orow[(long)p * 7 + e] = 0.f;
    if (out_index) out_index[(long)b * max_det + p] = -1;
  }
}

extern "C" int ey_nms_rotated(int B, int nc, int A, const float* pred, float conf_thres, float iou_thres, int max_det, int max_nms, float max_wh, int agnostic,
                              const uint8_t* class_mask, float* out_rows, int32_t* out_count, int32_t* out_index, void* workspace, size_t workspace_bytes,
                              ey_stream_t stream) {
  EY_CHECK(B > 0 && nc > 0 && A > 0 && max_det > 0 && max_nms > 0, "nms_rotated: B=%d nc=%d A=%d max_det=%d max_nms=%d", B, nc, A, max_det, max_nms);
  EY_CHECK(pred && out_rows && out_count && workspace, "nms_rotated: null pointer");
  EY_CHECK(conf_thres >= 0.f, "nms_rotated: conf_thres=%g (the sort key orders non-negative scores by their bits)", (double)conf_thres);
  EY_CHECK(ey_aligned(workspace, 256), "nms_rotated: the workspace must be 256-byte aligned");
  if (B > 65535 || (long)B * (4 + nc + 1) * A >= (1L << 40) || (long)B * max_det * 7 >= (1L << 40)) return ey_set_error(EY_EUNSUPPORTED, "nms_rotated: tensor too large");
  ObbWs ws;
  const size_t need = obb_ws_layout(B, A, max_nms, (char*)workspace, &ws);
  EY_CHECK(workspace_bytes >= need, "nms_rotated: workspace of %zu bytes, %zu needed", workspace_bytes, need);
  const int tiles = ey_cdiv(ws.maxn, OBB_TILE), chunks = ey_cdiv(ws.maxn, OBB_ROWS);
  if (chunks > 65535) return ey_set_error(EY_EUNSUPPORTED, "nms_rotated: %d candidates per image", ws.maxn);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(obb_init_kernel, dim3(ey_cdiv((long)B * ws.maxn, 256)), dim3(256), 0, st, B, ws);
  hipLaunchKernelGGL(obb_score_kernel, dim3(ey_cdiv(A, 256), B), dim3(256), 0, st, nc, A, pred, conf_thres, class_mask, ws);
  hipLaunchKernelGGL(obb_rank_kernel, dim3(ey_cdiv(A, 256), B), dim3(256), 0, st, nc, A, pred, max_nms, agnostic ? 0.f : max_wh, ws);
  hipLaunchKernelGGL(obb_pair_kernel, dim3(tiles, chunks, B), dim3(OBB_TILE), 0, st, max_nms, ws);
  hipLaunchKernelGGL(obb_resolve_kernel, dim3(B), dim3(1024), 0, st, nc, A, pred, iou_thres, max_det, max_nms, ws, out_rows, out_count, out_index);
  EY_LAUNCH_CHECK("ey_nms_rotated");
  return EY_OK;
}

// ---------------------------------------------------------------------------------------------------------------- rotated NMS, multi label
// The validation regime (ops.py:270-297 with multi_label): every (anchor a, class c) with score > conf is a candidate, up to NK = A nc per
// image, cut to the max_nms best.  Six launches, no host synchronisation:
//   obb_init        (the kernel above) candidate counters = 0, column minima = +inf
//   obb_ml_score    thread = one (anchor, class) score, read coalesced; candidates are compacted with one atomic per wave:
//                   key = score_bits << 32 | ~(a nc + c), unique per image, so the slot order does not matter
//   obb_ml_select   one workgroup per image: with more than max_nms candidates, the max_nms-th largest key by an 8-bit radix select over
//                   the 64 key bits (LDS histogram of integer counts, 8 passes over the image's keys, no ranking of all candidates); then
//                   the keys >= that key, exactly min(n, max_nms) of them, are compacted into the survivor list
//   obb_ml_rank     obb_rank_of over the survivors (all pairs of at most max_nms keys) -> the Gaussian record at the key's position
//   obb_pair, obb_resolve   the kernels above, unchanged: the records, the class list and the counter have the single-label layout
// workspace, every part 256-byte aligned: counters [B] | candidate counters [B] | keys [B][NK] u64 | survivor keys [B][maxn] u64 |
// records [B][maxn][8] | sorted class ids [B][maxn] | column minima [B][maxn], maxn = min(NK, max_nms).
struct ObbMl {
  int* ncand;
  unsigned long long* keys;
  unsigned long long* skeys;
  long NK;
};
static size_t obb_ml_layout(int B, long NK, int max_nms, char* base, ObbWs* ws, ObbMl* ml) {
  const size_t maxn = (size_t)(NK < max_nms ? NK : max_nms);
  size_t off = 0;
  const size_t o_cnt = off; off += obb_al((size_t)B * 4);
  const size_t o_ncand = off; off += obb_al((size_t)B * 4);
  const size_t o_keys = off; off += obb_al((size_t)B * NK * 8);
  const size_t o_skeys = off; off += obb_al((size_t)B * maxn * 8);
  const size_t o_rec = off; off += obb_al((size_t)B * maxn * 32);
  const size_t o_scls = off; off += obb_al((size_t)B * maxn * 4);
  const size_t o_min = off; off += obb_al((size_t)B * maxn * 4);
  if (ws) {
    ws->cnt = (int*)(base + o_cnt);
    ws->keys = (unsigned long long*)(base + o_skeys);
    ws->ccls = nullptr;
    ws->rec = (float*)(base + o_rec);
    ws->scls = (int*)(base + o_scls);
    ws->colmin = (unsigned*)(base + o_min);
    ws->maxn = (int)maxn;
    ml->ncand = (int*)(base + o_ncand);
    ml->keys = (unsigned long long*)(base + o_keys);
    ml->skeys = ws->keys;
    ml->NK = NK;
  }
  return off;
}
extern "C" size_t ey_nms_rotated_ml_workspace_bytes(int B, int nc, int A, int max_nms) {
  if (B <= 0 || nc <= 0 || A <= 0 || max_nms <= 0 || (long)A * nc >= (1L << 31)) return 0;
  return obb_ml_layout(B, (long)A * nc, max_nms, nullptr, nullptr, nullptr);
}

// slots for the lanes of a wave that hold a candidate: one atomic on `counter` per wave, the lanes in lane order behind it
__device__ __forceinline__ int obb_wave_slot(bool on, int* counter, int lane) {
  const unsigned long long bal = __ballot(on);
  int base = 0;
  if (lane == 0 && bal) base = atomicAdd(counter, __popcll(bal));
  base = __shfl(base, 0);
  return base + __popcll(bal & ((1ull << lane) - 1ull));
}

__global__ __launch_bounds__(256) void obb_ml_score_kernel(int nc, int A, const float* __restrict__ pred, float conf, const uint8_t* __restrict__ mask, ObbMl ml) {
  const int b = blockIdx.z, c = blockIdx.y, a = blockIdx.x * 256 + threadIdx.x;
  float s = 0.f;
  bool on = false;
  if (a < A && (!mask || mask[c])) {
    s = pred[(long)b * (4 + nc + 1) * A + (long)(4 + c) * A + a];
    on = s > conf;  // (strict; a NaN score is no candidate)
  }
  const int slot = obb_wave_slot(on, &ml.ncand[b], threadIdx.x & 63);
  if (on) ml.keys[(long)b * ml.NK + slot] = ((unsigned long long)__float_as_uint(s) << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)(a * nc + c));
}

__global__ __launch_bounds__(1024) void obb_ml_select_kernel(int max_nms, ObbWs ws, ObbMl ml) {
  __shared__ int hist[256];
  __shared__ int s_digit, s_k, s_cnt;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const int n = ml.ncand[b];
  const unsigned long long* keys = ml.keys + (long)b * ml.NK;
  unsigned long long thr = 0ull;  // the smallest surviving key
  if (n > max_nms) {  // (workgroup-uniform)
    // invariant: at least k keys agree with `thr` on the bits above `shift`, and the k-th largest of them is the max_nms-th largest of all
    int k = max_nms;
    for (int shift = 56; shift >= 0; shift -= 8) {
      if (tid < 256) hist[tid] = 0;
      __syncthreads();
      for (int i0 = 0; i0 < n; i0 += 1024) {  // (every lane of a wave runs the same number of rounds)
        const int i = i0 + tid;
        const unsigned long long key = i < n ? keys[i] : 0ull;
        bool on = i < n && (shift == 56 || (key >> (shift + 8)) == (thr >> (shift + 8)));
        const int digit = (int)((key >> shift) & 255ull);
        // scores share their leading bits: up to four digit values are counted by one atomic per wave each, the rest lane by lane
        for (int it = 0; it < 4; ++it) {
          const unsigned long long bal = __ballot(on);
          if (!bal) break;  // (wave-uniform)
          const int leader = __ffsll((long long)bal) - 1;
          const int d = __shfl(digit, leader);
          const unsigned long long same = __ballot(on && digit == d);
          if (lane == leader) atomicAdd(&hist[d], __popcll(same));
          if (digit == d) on = false;
        }
        if (on) atomicAdd(&hist[digit], 1);
      }
      __syncthreads();
      if (tid == 0) {
        int above = 0, d = 255;
        for (; d > 0; --d) {
          if (above + hist[d] >= k) break;
          above += hist[d];
        }
        s_digit = d;
        s_k = k - above;
      }
      __syncthreads();
      thr |= (unsigned long long)s_digit << shift;
      k = s_k;
    }
  }
  if (tid == 0) s_cnt = 0;
  __syncthreads();
  unsigned long long* skeys = ml.skeys + (long)b * ws.maxn;
  for (int i0 = 0; i0 < n; i0 += 1024) {
    const int i = i0 + tid;
    const unsigned long long key = i < n ? keys[i] : 0ull;
    const bool on = i < n && key >= thr;
    const int slot = obb_wave_slot(on, &s_cnt, lane);
    if (on && slot < ws.maxn) skeys[slot] = key;  // (keys are unique: exactly min(n, max_nms) <= maxn of them pass)
  }
  if (tid == 0) ws.cnt[b] = min(n, max_nms);
}

__global__ __launch_bounds__(256) void obb_ml_rank_kernel(int nc, int A, const float* __restrict__ pred, float cls_off, ObbWs ws) {
  __shared__ unsigned long long tile[256];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int n = ws.cnt[b];
  if ((int)blockIdx.x * 256 >= n) return;  // (workgroup-uniform)
  const unsigned long long* keys = ws.keys + (long)b * ws.maxn;
  const int j = blockIdx.x * 256 + tid;
  const unsigned long long key = j < n ? keys[j] : ~0ull;
  const int rank = obb_rank_of(keys, n, key, tile, tid);
  if (j >= n) return;
  const int flat = (int)(0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull));
  const int a = flat / nc;
  obb_write_record(b, nc, A, pred, cls_off, ws, rank, a, flat - a * nc, (unsigned)(key >> 32));
}

extern "C" int ey_nms_rotated_ml(int B, int nc, int A, const float* pred, float conf_thres, float iou_thres, int max_det, int max_nms, float max_wh, int agnostic,
                                 const uint8_t* class_mask, float* out_rows, int32_t* out_count, int32_t* out_index, void* workspace, size_t workspace_bytes,
                                 ey_stream_t stream) {
  EY_CHECK(B > 0 && nc > 0 && A > 0 && max_det > 0 && max_nms > 0, "nms_rotated_ml: B=%d nc=%d A=%d max_det=%d max_nms=%d", B, nc, A, max_det, max_nms);
  EY_CHECK(pred && out_rows && out_count && workspace, "nms_rotated_ml: null pointer");
  EY_CHECK(conf_thres >= 0.f, "nms_rotated_ml: conf_thres=%g (the sort key orders non-negative scores by their bits)", (double)conf_thres);
  EY_CHECK(ey_aligned(workspace, 256), "nms_rotated_ml: the workspace must be 256-byte aligned");
  if (B > 65535 || nc > 65535 || (long)A * nc >= (1L << 31) || (long)B * (4 + nc + 1) * A >= (1L << 40) || (long)B * max_det * 7 >= (1L << 40))
    return ey_set_error(EY_EUNSUPPORTED, "nms_rotated_ml: tensor too large");
  ObbWs ws;
  ObbMl ml;
  const size_t need = obb_ml_layout(B, (long)A * nc, max_nms, (char*)workspace, &ws, &ml);
  EY_CHECK(workspace_bytes >= need, "nms_rotated_ml: workspace of %zu bytes, %zu needed", workspace_bytes, need);
  const int tiles = ey_cdiv(ws.maxn, OBB_TILE), chunks = ey_cdiv(ws.maxn, OBB_ROWS);
  if (chunks > 65535) return ey_set_error(EY_EUNSUPPORTED, "nms_rotated_ml: %d candidates per image", ws.maxn);
  hipStream_t st = (hipStream_t)stream;
  ObbWs wi = ws;
  wi.cnt = ml.ncand;  // obb_init zeroes the counters it is given: the candidate counters (obb_ml_select writes ws.cnt itself)
  hipLaunchKernelGGL(obb_init_kernel, dim3(ey_cdiv((long)B * ws.maxn, 256)), dim3(256), 0, st, B, wi);
  hipLaunchKernelGGL(obb_ml_score_kernel, dim3(ey_cdiv(A, 256), nc, B), dim3(256), 0, st, nc, A, pred, conf_thres, class_mask, ml);
  hipLaunchKernelGGL(obb_ml_select_kernel, dim3(B), dim3(1024), 0, st, max_nms, ws, ml);
  hipLaunchKernelGGL(obb_ml_rank_kernel, dim3(ey_cdiv(ws.maxn, 256), B), dim3(256), 0, st, nc, A, pred, agnostic ? 0.f : max_wh, ws);
  hipLaunchKernelGGL(obb_pair_kernel, dim3(tiles, chunks, B), dim3(OBB_TILE), 0, st, max_nms, ws);
  hipLaunchKernelGGL(obb_resolve_kernel, dim3(B), dim3(1024), 0, st, nc, A, pred, iou_thres, max_det, max_nms, ws, out_rows, out_count, out_index);
  EY_LAUNCH_CHECK("ey_nms_rotated_ml");
  return EY_OK;
}
