// Mask IoU for segment validation (reference ultralytics/utils/metrics.py:137-153 mask_iou, fused with the ground-truth expansion of
// models/yolo/segment/val.py:204-213 SegmentationValidator._process_batch), every image of a batch in one call.
//
// Both operands are 0/1, so the reference's float matmul is a population count.  Three launches:
//   mi_pack_pred  predicted masks (bytes) -> 64-pixel words: a wave reads 256 pixels, a dword per lane, and ballots each of the four byte
//                 positions into a word; the words are stored word-major per image (P[w][n]) through an LDS transpose, so that the pair
//                 kernel's lanes (= predictions) read consecutive words;
//   mi_pack_gt    ground truth -> words G[m][w]; the stack form reads bytes, the index form compares the ONE map of the image against m + 1
//                 for 8 instances per loaded pixel (the reference's gt_masks.repeat(nl, 1, 1) is never written anywhere);
//   mi_pair       inter[m][n] = sum_w popc(G[m][w] & P[w][n]); a workgroup owns 64 predictions x 8 ground-truth rows, its 4 waves split
//                 the words and meet in LDS.  The gt word is wave-uniform.  Areas are the popcounts of the same words.
// Pixels are assigned to bits identically on both sides and the bits past the last pixel are 0, so the counts are exact integers;
// integer sums take any order, there are no float operations before the final expression and no atomics at all.  The final value is the
// reference's fp32 expression op by op (this file is built with -ffp-contract=off):
//   iou = fl(inter / fl(fl(fl(a_gt + a_pred) - inter) + 1e-7f))
#include "common.h"

#define MI_MAXB 128  // images per call (the offset tables travel as kernel arguments)
#define MI_PW 32     // words per mi_pack_pred tile
#define MI_MC 8      // ground-truth instances per mi_pack_gt wave / rows per mi_pair workgroup

typedef unsigned long long mi_word;

struct mi_tab {
  int B;
  int pred_off[MI_MAXB + 1];
  int gt_off[MI_MAXB + 1];
  long out_off[MI_MAXB];
};

// item -> (image, item within the image) for per-image item counts cdiv(cnt_b, per) * inner; false past the last item.  An image that is
// empty on the other side has no matrix and no items: its masks are not packed (their workspace rows stay unwritten and unread).
__device__ __forceinline__ bool mi_locate(const int* off, const int* other, int B, int per, long inner, long item, int& b, long& t) {
  for (int i = 0; i < B; ++i) {
    const long cnt = other[i + 1] > other[i] ? (long)((off[i + 1] - off[i] + per - 1) / per) * inner : 0;
    if (item < cnt) { b = i; t = item; return true; }
    item -= cnt;
  }
  return false;
}

// Four consecutive mask bytes of a lane: pixels base .. base + 3 of a row of HW bytes (0 beyond the row).  One dword load where the row
// is 4-byte aligned (`vec`) and the dword lies inside it.
__device__ __forceinline__ unsigned mi_load4(const uint8_t* __restrict__ src, long base, int HW, bool vec) {
  if (vec && base + 4 <= HW) return *reinterpret_cast<const unsigned*>(src + base);
  unsigned v = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (base + e < HW) v |= (unsigned)src[base + e] << (8 * e);
  return v;
}

// Pixel -> bit: a wave reads 256 consecutive pixels at once, lane l the pixels 4 l .. 4 l + 3, and ballots byte e of every lane into word
// 4 blk + e: bit l of word 4 blk + e is pixel 256 blk + 4 l + e.  The same rule on both sides; nw = 4 * ceil(HW / 256) words per mask.
__global__ __launch_bounds__(256) void mi_pack_pred(mi_tab tab, int HW, int nw, const uint8_t* __restrict__ pred, mi_word* __restrict__ P) {
  __shared__ mi_word tile[MI_PW][64];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int nwt = (nw + MI_PW - 1) / MI_PW;
  int b;
  long t;
  if (!mi_locate(tab.pred_off, tab.gt_off, tab.B, 64, nwt, blockIdx.x, b, t)) return;  // (workgroup-uniform)
  const int Nb = tab.pred_off[b + 1] - tab.pred_off[b];
  const int n0 = (int)(t / nwt) * 64, w0 = (int)(t % nwt) * MI_PW;
  for (int i = 0; i < 16; ++i) {
    const int nl = wave * 16 + i;
    const bool valid = n0 + nl < Nb;  // (wave-uniform)
    const uint8_t* src = pred + (long)(tab.pred_off[b] + (valid ? n0 + nl : 0)) * HW;
    const bool vec = ((uintptr_t)src & 3) == 0;
    unsigned v[MI_PW / 4];
#pragma unroll
    for (int j = 0; j < MI_PW / 4; ++j) v[j] = valid ? mi_load4(src, (long)(w0 / 4 + j) * 256 + 4 * lane, HW, vec) : 0u;  // (blocks past the mask: 0)
#pragma unroll
    for (int j = 0; j < MI_PW / 4; ++j) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const mi_word bal = __ballot((v[j] >> (8 * e)) & 0xffu);
        if (lane == 0) tile[4 * j + e][nl] = bal;
      }
    }
  }
  __syncthreads();
  mi_word* out = P + (long)tab.pred_off[b] * nw;
  for (int idx = threadIdx.x; idx < MI_PW * 64; idx += 256) {
    const int j = idx >> 6, nl = idx & 63;
    if (w0 + j < nw && n0 + nl < Nb) out[(long)(w0 + j) * Nb + n0 + nl] = tile[j][nl];
  }
}

// a wave owns 64 words (16 blocks of 256 pixels) of up to MI_MC instances of one image; lane j keeps word j
__global__ __launch_bounds__(256) void mi_pack_gt(mi_tab tab, int index_mode, int HW, int nw, const void* __restrict__ gt, mi_word* __restrict__ G) {
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int nwg = (nw + 63) / 64;
  int b;
  long t;
  if (!mi_locate(tab.gt_off, tab.pred_off, tab.B, MI_MC, nwg, (long)blockIdx.x * 4 + wave, b, t)) return;  // (wave-uniform; no barrier below)
  const int Mb = tab.gt_off[b + 1] - tab.gt_off[b];
  const int m0 = (int)(t / nwg) * MI_MC, w0 = (int)(t % nwg) * 64;
  const int* map = (const int*)gt + (long)b * HW;
  const uint8_t* stack = (const uint8_t*)gt + (long)(tab.gt_off[b] + m0) * HW;
  mi_word mine[MI_MC];
#pragma unroll
  for (int k = 0; k < MI_MC; ++k) mine[k] = 0;
  const int nj = min(16, (nw - w0) / 4);  // (nw and w0 are multiples of 4)
  for (int j = 0; j < nj; ++j) {
    const long base = (long)(w0 / 4 + j) * 256 + 4 * lane;
    if (index_mode) {
      int v[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = base + e < HW ? map[base + e] : 0;  // (0 belongs to no instance)
#pragma unroll
      for (int k = 0; k < MI_MC; ++k) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const mi_word bal = __ballot(v[e] == m0 + k + 1);
          if (lane == 4 * j + e) mine[k] = bal;
        }
      }
    } else {
#pragma unroll
      for (int k = 0; k < MI_MC; ++k) {
        const uint8_t* src = stack + (long)k * HW;
        const unsigned v = m0 + k < Mb ? mi_load4(src, base, HW, ((uintptr_t)src & 3) == 0) : 0u;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const mi_word bal = __ballot((v >> (8 * e)) & 0xffu);
          if (lane == 4 * j + e) mine[k] = bal;
        }
      }
    }
  }
  if (lane < 4 * nj) {
#pragma unroll
    for (int k = 0; k < MI_MC; ++k)
      if (m0 + k < Mb) G[(long)(tab.gt_off[b] + m0 + k) * nw + w0 + lane] = mine[k];
  }
}

__global__ __launch_bounds__(256) void mi_pair(mi_tab tab, int nw, const mi_word* __restrict__ P, const mi_word* __restrict__ G, float* __restrict__ iou,
                                               int* __restrict__ inter) {
  __shared__ int red[3][MI_MC + 1][64];  // waves 1..3: inter of the MI_MC rows, then the prediction's area
  __shared__ int red_g[3][MI_MC];        // ... and the rows' areas
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  int b = 0;
  long t = 0;
  {  // items of image b: cdiv(N_b, 64) * cdiv(M_b, MI_MC); an image without predictions or without ground truth has none
    long item = blockIdx.x;
    for (int i = 0; i < tab.B; ++i) {
      const long cnt = (long)((tab.pred_off[i + 1] - tab.pred_off[i] + 63) / 64) * ((tab.gt_off[i + 1] - tab.gt_off[i] + MI_MC - 1) / MI_MC);
      if (item < cnt) { b = i; t = item; item = -1; break; }
      item -= cnt;
    }
    if (item >= 0) return;  // (workgroup-uniform)
  }
  const int Nb = tab.pred_off[b + 1] - tab.pred_off[b], Mb = tab.gt_off[b + 1] - tab.gt_off[b];
  const int nmc = (Mb + MI_MC - 1) / MI_MC;
  const int n = (int)(t / nmc) * 64 + lane, m0 = (int)(t % nmc) * MI_MC;
  const bool live = n < Nb;
  const mi_word* p = P + (long)tab.pred_off[b] * nw + (live ? n : 0);
  const mi_word* g[MI_MC];
#pragma unroll
  for (int k = 0; k < MI_MC; ++k) g[k] = G + (long)(tab.gt_off[b] + min(m0 + k, Mb - 1)) * nw;  // (tail rows: a valid row, never stored)
  int acc[MI_MC], ap = 0, ag[MI_MC];
#pragma unroll
  for (int k = 0; k < MI_MC; ++k) acc[k] = ag[k] = 0;
  const int per = (nw + 3) / 4;
  const int wlo = wave * per, whi = min(nw, wlo + per);
#pragma unroll 2
  for (int w = wlo; w < whi; ++w) {
    const mi_word pw = live ? p[(long)w * Nb] : 0ull;
    ap += __popcll(pw);
#pragma unroll
    for (int k = 0; k < MI_MC; ++k) {
      const mi_word gw = g[k][w];  // wave-uniform address
      acc[k] += __popcll(gw & pw);
      ag[k] += __popcll(gw);
    }
  }
  if (wave) {
#pragma unroll
    for (int k = 0; k < MI_MC; ++k) red[wave - 1][k][lane] = acc[k];
    red[wave - 1][MI_MC][lane] = ap;
    if (lane == 0) {
#pragma unroll
      for (int k = 0; k < MI_MC; ++k) red_g[wave - 1][k] = ag[k];
    }
  }
  __syncthreads();
  if (wave || !live) return;
  for (int q = 0; q < 3; ++q) ap += red[q][MI_MC][lane];
  const float fap = (float)ap;
#pragma unroll
  for (int k = 0; k < MI_MC; ++k) {
    if (m0 + k >= Mb) break;
    int it = acc[k], a = ag[k];
    for (int q = 0; q < 3; ++q) { it += red[q][k][lane]; a += red_g[q][k]; }
    const float fi = (float)it;
    const float uni = __fadd_rn(__fsub_rn(__fadd_rn((float)a, fap), fi), 1e-7f);
    const long o = tab.out_off[b] + (long)(m0 + k) * Nb + n;
    iou[o] = __fdiv_rn(fi, uni);
    if (inter) inter[o] = it;
  }
}

static inline size_t mi_words(int H, int W) { return ((size_t)H * W + 255) / 256 * 4; }

extern "C" size_t ey_mask_iou_workspace_bytes(int H, int W, long n_pred, long n_gt) {
  if (H <= 0 || W <= 0 || n_pred < 0 || n_gt < 0) return 0;
  return ((size_t)(n_pred + n_gt) * mi_words(H, W) * sizeof(mi_word) + 15) / 16 * 16;
}

extern "C" int ey_mask_iou(int gt_mode, int B, int H, int W, const uint8_t* pred, const int* pred_off, const void* gt, const int* gt_off,
                           const long* out_off, float* iou, int* inter, void* workspace, size_t workspace_bytes, ey_stream_t stream) {
  EY_CHECK(gt_mode == EY_MASK_GT_STACK || gt_mode == EY_MASK_GT_INDEX, "mask_iou: gt_mode=%d (EY_MASK_GT_STACK or EY_MASK_GT_INDEX)", gt_mode);
  EY_CHECK(B >= 0 && H > 0 && W > 0, "mask_iou: B=%d H=%d W=%d", B, H, W);
  if (B > MI_MAXB) return ey_set_error(EY_EUNSUPPORTED, "mask_iou: B=%d (up to %d images per call are built)", B, MI_MAXB);
  if ((long)H * W > (1L << 24)) return ey_set_error(EY_EUNSUPPORTED, "mask_iou: %d x %d pixels (up to 2^24: the areas must be exact in fp32)", H, W);
  if (B == 0) return EY_OK;
  EY_CHECK(pred_off && gt_off && out_off, "mask_iou: null offset table");
  EY_CHECK(pred_off[0] == 0 && gt_off[0] == 0, "mask_iou: pred_off[0]=%d gt_off[0]=%d must be 0", pred_off[0], gt_off[0]);
  mi_tab tab = {};
  tab.B = B;
  const int HW = H * W, nw = (int)mi_words(H, W);
  long pack_p = 0, pack_g = 0, pairs = 0;
  for (int b = 0; b < B; ++b) {
    const long nb = (long)pred_off[b + 1] - pred_off[b], mb = (long)gt_off[b + 1] - gt_off[b];
    EY_CHECK(nb >= 0 && mb >= 0, "mask_iou: offsets of image %d decrease", b);
    EY_CHECK(!(nb && mb) || out_off[b] >= 0, "mask_iou: out_off[%d]=%ld", b, out_off[b]);
    tab.pred_off[b + 1] = pred_off[b + 1];
    tab.gt_off[b + 1] = gt_off[b + 1];
    tab.out_off[b] = out_off[b];
    if (!(nb && mb)) continue;  // no matrix: nothing of this image is packed (mi_locate skips it the same way)
    pack_p += ey_cdiv(nb, 64) * (long)ey_cdiv(nw, MI_PW);
    pack_g += ey_cdiv(mb, MI_MC) * (long)ey_cdiv(nw, 64);
    pairs += ey_cdiv(nb, 64) * (long)ey_cdiv(mb, MI_MC);
  }
  const long n_pred = pred_off[B], n_gt = gt_off[B];
  if ((n_pred + n_gt) * (long)nw >= (1L << 40) || pack_p >= (1L << 31) || pack_g >= (1L << 31) || pairs >= (1L << 31))
    return ey_set_error(EY_EUNSUPPORTED, "mask_iou: too much work for one call (%ld + %ld masks of %d words)", n_pred, n_gt, nw);
  if (pairs == 0) return EY_OK;
  EY_CHECK(pred && gt && iou && workspace, "mask_iou: null pointer");
  EY_CHECK(ey_aligned(workspace, 16), "mask_iou: workspace must be 16-byte aligned");
  EY_CHECK(ey_aligned(iou, 4) && ey_aligned(inter, 4) && (gt_mode != EY_MASK_GT_INDEX || ey_aligned(gt, 4)), "mask_iou: misaligned iou / inter / index map");
  const size_t need = ey_mask_iou_workspace_bytes(H, W, n_pred, n_gt);
  EY_CHECK(workspace_bytes >= need, "mask_iou: workspace of %zu bytes, needs %zu (ey_mask_iou_workspace_bytes)", workspace_bytes, need);
  mi_word* P = (mi_word*)workspace;
  mi_word* G = P + (size_t)n_pred * nw;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(mi_pack_pred, dim3((unsigned)pack_p), dim3(256), 0, st, tab, HW, nw, pred, P);
  EY_LAUNCH_CHECK("ey_mask_iou (pack pred)");
  hipLaunchKernelGGL(mi_pack_gt, dim3((unsigned)ey_cdiv(pack_g, 4)), dim3(256), 0, st, tab, gt_mode == EY_MASK_GT_INDEX, HW, nw, gt, G);
  EY_LAUNCH_CHECK("ey_mask_iou (pack gt)");
  hipLaunchKernelGGL(mi_pair, dim3((unsigned)pairs), dim3(256), 0, st, tab, nw, (const mi_word*)P, (const mi_word*)G, iou, inter);
  EY_LAUNCH_CHECK("ey_mask_iou (pair)");
  return EY_OK;
}
