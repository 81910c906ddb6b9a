// FastSAM prompt selection (reference ultralytics/models/fastsam/predict.py:61-103 FastSAMPredictor.prompt, with the resize of
// utils/ops.py:716-737 scale_masks folded in) and scale_masks itself.
//
// The reference resizes every kept mask bilinearly to the original image and then slices and sums that tensor once per prompt.  The
// resize is linear and separable: with wy(y, i), wx(x, j) the per-axis interpolation weights of F.interpolate(mode="bilinear",
// align_corners=False) on the cropped mask,
//   resized[y][x]                    = sum_ij M[i][j] wy(y, i) wx(x, j)
//   sum_{y1<=y<y2, x1<=x<x2} resized = sum_ij M[i][j] Wy[i] Wx[j],     Wy[i] = sum_{y1<=y<y2} wy(y, i),  Wx[j] = sum_{x1<=x<x2} wx(x, j)
// so one pass over the network-resolution bytes scores every box, and the full area is the box [0,W0) x [0,H0).  Three launches:
//   mp_weights  W[image][axis][index][slot] for slot = box 0 .. P-1, then the whole image (slot P); slots up to NB-1 and indices outside the
//               crop are 0.  A thread owns one (index, slot) and GATHERS: it walks the few target coordinates whose two source indices can
//               be this one, ascending, and adds their weights in that order (no atomics).
//   mp_score    a workgroup owns one mask.  Both weight tables of its image sit in LDS; the mask is read as 16-byte words counted from its first byte (every
//               byte once), all-zero words are skipped; a set byte at (i, j) adds Wx[j] to the row sums of its word, a row's sums times
//               Wy[i] go to the thread's accumulators; the point prompts are tested on the same byte (only in words that
//               touch a source row of some point).  Threads meet through a wave
//               shuffle tree and LDS in a fixed order.  Writes inter[p][n], full[n], hit[q][n].
//   mp_select   a workgroup owns one image: iou, the per-box argmax (ties to the lower index) and keep.
// Per-axis source index and weights (mp_source, mask_source.h) are torch's CPU operator's (aten/src/ATen/native/UpSample.h
// compute_source_index_and_lambda with float opmath; the source coordinate is ONE fused multiply-add, which is what the operator's compiled
// code evaluates -- the two-rounding form differs from it in individual weights):
//   in == out:  i0 = i1 = y, l0 = 1, l1 = 0
//   otherwise:  r = max(fmaf((float)in / out, y + 0.5f, -0.5f), 0);  i0 = min((int)r, in - 1);  l1 = min(max(r - i0, 0), 1);
//               i1 = i0 + (i0 < in - 1);  l0 = 1 - l1
// This file is built with -ffp-contract=off: every fused operation below is written out.
#include "common.h"
#include "mask_source.h"

#define MP_MAXB 64   // images per call (the tables travel as a kernel argument)
#define MP_MAXP 32   // box prompts
#define MP_MAXQ 32   // point prompts (the hits of a mask are one 32-bit word)
#define MP_MAXC 32767  // coordinates: the reference's int32 box area cannot overflow below this

struct mp_tab {
  int B, P, Q, all_neg;
  int off[MP_MAXB + 1];
  int geo[MP_MAXB][6];  // top, bottom, left, right (crop of the mask), H0, W0 (target)
  int box[MP_MAXP][4];  // x1, y1, x2, y2
  int pt[MP_MAXQ][3];   // x, y, label
};

struct __attribute__((packed, aligned(1))) mp_u4 {
  unsigned x, y, z, w;
};

// W[b][axis][index * NB + slot]; axis 0 = rows (mh entries), axis 1 = columns (mw entries)
__global__ __launch_bounds__(256) void mp_weights(mp_tab tab, int mh, int mw, int NB, float* __restrict__ W) {
  const int b = blockIdx.z, axis = blockIdx.y;
  const int len = axis ? mw : mh;
  const int item = blockIdx.x * 256 + threadIdx.x;
  if (item >= len * NB) return;
  const int idx = item / NB, p = item - idx * NB;
  const int* g = tab.geo[b];
  const int c0 = axis ? g[2] : g[0], c1 = axis ? g[3] : g[1], out = axis ? g[5] : g[4];
  const int in = c1 - c0, ci = idx - c0;
  int lo = 0, hi = 0;  // target range of the slot (empty: padding slot)
  if (p < tab.P) {
    lo = axis ? tab.box[p][0] : tab.box[p][1];
    hi = min(axis ? tab.box[p][2] : tab.box[p][3], out);
  } else if (p == tab.P) {
    hi = out;
  }
  float w = 0.f;
  if (ci >= 0 && ci < in && lo < hi) {
    int ya, yb;
    if (in == out) {
      ya = ci;
      yb = ci + 1;
    } else {  // targets whose source coordinate lies in [ci - 1, ci + 1), one more on either side
      const double inv = (double)out / (double)in;
      ya = (int)floor((ci - 0.5) * inv - 0.5) - 1;
      yb = (int)ceil((ci + 1.5) * inv - 0.5) + 2;
    }
    ya = max(ya, lo);
    yb = min(yb, hi);
    for (int y = ya; y < yb; ++y) {
      const mp_src s = mp_source(y, in, out);
      if (s.i0 == ci) w = __fadd_rn(w, s.l0);
      if (s.i1 == ci) w = __fadd_rn(w, s.l1);
    }
  }
  W[((long)b * (mh + mw) + (axis ? mh : 0)) * NB + item] = w;
}

// One 16-byte word of a mask: `pos` = index of its first byte.  Adds the set bytes' column weights to row sums and every row's sum times its
// row weight to acc; tests the points where `rowflag` says the word touches a row some point reads.
template <int NB>
__device__ __forceinline__ void mp_word(const uint4 v4, int pos, int mw, int HW, const float* Wy, const float* Wx, const uint8_t* rowflag, int Q,
                                        const int (*prow)[2], const int (*pcol)[2], float (&acc)[NB], unsigned& hits) {
  const unsigned v[4] = {v4.x, v4.y, v4.z, v4.w};
  int i = pos / mw, j = pos - i * mw;
  bool pts = false;
  if (Q) {
    const int last = (min(pos + 15, HW - 1)) / mw;
    for (int r = i; r <= last; ++r) pts |= rowflag[r] != 0;
  }
  float rs[NB];
#pragma unroll
  for (int p = 0; p < NB; ++p) rs[p] = 0.f;
  bool any = false;
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    unsigned u = v[d];
    for (int e = 0; e < 4; ++e, ++pos, u >>= 8) {
      if (pos >= HW) continue;
      if (u & 0xffu) {
        const float* wx = Wx + j * NB;
#pragma unroll
        for (int p = 0; p < NB; ++p) rs[p] = __fadd_rn(rs[p], wx[p]);
        any = true;
        if (pts) {
          for (int q = 0; q < Q; ++q)
            if ((i == prow[q][0] || i == prow[q][1]) && (j == pcol[q][0] || j == pcol[q][1])) hits |= 1u << q;
        }
      }
      if (++j == mw) {  // the row ends inside the word
        if (any) {
          const float* wy = Wy + i * NB;
#pragma unroll
          for (int p = 0; p < NB; ++p) {
            acc[p] = __fadd_rn(acc[p], __fmul_rn(wy[p], rs[p]));
            rs[p] = 0.f;
          }
          any = false;
        }
        j = 0;
        ++i;
      }
    }
  }
  if (any) {
    const float* wy = Wy + i * NB;
#pragma unroll
    for (int p = 0; p < NB; ++p) acc[p] = __fadd_rn(acc[p], __fmul_rn(wy[p], rs[p]));
  }
}

// Word w of a mask (bytes 16 w .. 16 w + 15 from its first byte), zeros past its end.
__device__ __forceinline__ uint4 mp_load(const uint8_t* src, int w, int HW) {
  if (w * 16 + 16 <= HW) {
    const mp_u4 t = *reinterpret_cast<const mp_u4*>(src + w * 16);  // any byte alignment: one global_load_dwordx4
    return make_uint4(t.x, t.y, t.z, t.w);
  }
  unsigned long long lo = 0, hi = 0;  // the last, partial word: byte by byte, nothing is read past the mask
  for (int e = 0; e < 8; ++e) {
    if (w * 16 + e < HW) lo |= (unsigned long long)src[w * 16 + e] << (8 * e);
    if (w * 16 + 8 + e < HW) hi |= (unsigned long long)src[w * 16 + 8 + e] << (8 * e);
  }
  return make_uint4((unsigned)lo, (unsigned)(lo >> 32), (unsigned)hi, (unsigned)(hi >> 32));
}

#define MP_FLIGHT 4  // words a thread loads before it looks at the first (they are processed in ascending order all the same)

template <int NB>
__global__ __launch_bounds__(256) void mp_score(mp_tab tab, int mh, int mw, const uint8_t* __restrict__ masks, const float* __restrict__ W, long ld,
                                                float* __restrict__ full, float* __restrict__ inter, uint8_t* __restrict__ hit) {
  extern __shared__ __attribute__((aligned(16))) float lds[];  // Wy[mh][NB], Wx[mw][NB], then rowflag[mh] bytes
  __shared__ float red[3][NB];
  __shared__ unsigned red_hit[4];
  __shared__ int prow[MP_MAXQ][2], pcol[MP_MAXQ][2];  // source rows / columns of a point whose weight is not 0 (-1: none)
  const int n = blockIdx.x;  // mask row of the whole batch
  int b = 0;
  while (b + 1 < tab.B && n >= tab.off[b + 1]) ++b;  // (workgroup-uniform)
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const float* Wb = W + (long)b * (mh + mw) * NB;
  uint8_t* rowflag = reinterpret_cast<uint8_t*>(lds + (mh + mw) * NB);
  for (int k = threadIdx.x; k < (mh + mw) * NB; k += 256) lds[k] = Wb[k];
  for (int k = threadIdx.x; k < mh; k += 256) rowflag[k] = 0;
  const int Q = tab.Q;
  if (threadIdx.x < Q) {
    const int* g = tab.geo[b];
    const int q = threadIdx.x;
    const mp_src sy = mp_source(tab.pt[q][1], g[1] - g[0], g[4]), sx = mp_source(tab.pt[q][0], g[3] - g[2], g[5]);
    prow[q][0] = sy.l0 != 0.f ? g[0] + sy.i0 : -1;
    prow[q][1] = sy.l1 != 0.f ? g[0] + sy.i1 : -1;
    pcol[q][0] = sx.l0 != 0.f ? g[2] + sx.i0 : -1;
    pcol[q][1] = sx.l1 != 0.f ? g[2] + sx.i1 : -1;
  }
  __syncthreads();
  if (threadIdx.x < Q) {  // (several points may flag one row: they all write 1)
    if (prow[threadIdx.x][0] >= 0) rowflag[prow[threadIdx.x][0]] = 1;
    if (prow[threadIdx.x][1] >= 0) rowflag[prow[threadIdx.x][1]] = 1;
  }
  __syncthreads();
  const float* Wy = lds;
  const float* Wx = lds + mh * NB;
  const int HW = mh * mw;
  const uint8_t* src = masks + (long)n * HW;
  const int nwords = (HW + 15) >> 4;  // 16-byte words counted from the mask's first byte: the summation order does not depend on where the mask lies
  float acc[NB];
#pragma unroll
  for (int p = 0; p < NB; ++p) acc[p] = 0.f;
  unsigned hits = 0;
  for (int w0 = threadIdx.x; w0 < nwords; w0 += 256 * MP_FLIGHT) {
    const uint4 va = mp_load(src, w0, HW), vb = mp_load(src, w0 + 256, HW), vc = mp_load(src, w0 + 512, HW), vd = mp_load(src, w0 + 768, HW);
#pragma unroll 1
    for (int f = 0; f < MP_FLIGHT; ++f) {  // (one copy of the word's code: the word is selected, not indexed)
      const uint4 v = f == 0 ? va : f == 1 ? vb : f == 2 ? vc : vd;
      if (v.x | v.y | v.z | v.w) mp_word<NB>(v, (w0 + 256 * f) * 16, mw, HW, Wy, Wx, rowflag, Q, prow, pcol, acc, hits);
    }
  }
  // lanes: xor tree (6 levels), waves: 1, 2, 3 added to wave 0 in that order
#pragma unroll
  for (int p = 0; p < NB; ++p) {
#pragma unroll
    for (int d = 32; d; d >>= 1) acc[p] = __fadd_rn(acc[p], __shfl_xor(acc[p], d, 64));
  }
#pragma unroll
  for (int d = 32; d; d >>= 1) hits |= (unsigned)__shfl_xor((int)hits, d, 64);
  if (wave && lane == 0) {
#pragma unroll
    for (int p = 0; p < NB; ++p) red[wave - 1][p] = acc[p];
  }
  if (lane == 0) red_hit[wave] = hits;
  __syncthreads();
  if (threadIdx.x == 0) {
    const int P = tab.P;
#pragma unroll
    for (int p = 0; p < NB; ++p) {
      float a = acc[p];
      for (int k = 0; k < 3; ++k) a = __fadd_rn(a, red[k][p]);
      if (p < P) inter[(long)p * ld + n] = a;
      else if (p == P) full[n] = a;
    }
  }
  if (threadIdx.x < Q) hit[(long)threadIdx.x * ld + n] = ((red_hit[0] | red_hit[1] | red_hit[2] | red_hit[3]) >> threadIdx.x) & 1u;
}

// (value, index) with the larger value first, equal values by the lower index
__device__ __forceinline__ bool mp_better(float v, int i, float w, int k) { return v > w || (v == w && i < k); }

__global__ __launch_bounds__(256) void mp_select(mp_tab tab, long ld, const float* __restrict__ full, const float* __restrict__ inter, const uint8_t* __restrict__ hit,
                                                 float* __restrict__ iou, int* __restrict__ best, uint8_t* __restrict__ keep) {
  __shared__ float sv[256];
  __shared__ int si[256];
  __shared__ int sbest[MP_MAXP];
  const int b = blockIdx.x, P = tab.P, Q = tab.Q;
  const int n0 = tab.off[b], Nb = tab.off[b + 1] - n0;
  if (Nb == 0) {  // (workgroup-uniform)
    if (threadIdx.x < P) best[b * P + threadIdx.x] = -1;
    return;
  }
  for (int p = 0; p < P; ++p) {
    const float area = (float)((long)(tab.box[p][3] - tab.box[p][1]) * (long)(tab.box[p][2] - tab.box[p][0]));
    float bv = -1.f;
    int bi = 0x7fffffff;
    for (int k = threadIdx.x; k < Nb; k += 256) {  // ascending: a later equal value does not replace an earlier one
      const float it = inter[(long)p * ld + n0 + k];
      const float v = __fdiv_rn(it, __fsub_rn(__fadd_rn(area, full[n0 + k]), it));  // predict.py:83-84, op by op
      iou[(long)p * ld + n0 + k] = v;
      if (mp_better(v, k, bv, bi)) { bv = v; bi = k; }
    }
    sv[threadIdx.x] = bv;
    si[threadIdx.x] = bi;
    __syncthreads();
    for (int d = 128; d; d >>= 1) {
      if (threadIdx.x < d && mp_better(sv[threadIdx.x + d], si[threadIdx.x + d], sv[threadIdx.x], si[threadIdx.x])) {
        sv[threadIdx.x] = sv[threadIdx.x + d];
        si[threadIdx.x] = si[threadIdx.x + d];
      }
      __syncthreads();
    }
    if (threadIdx.x == 0) {
      sbest[p] = si[0];
      best[b * P + p] = si[0];
    }
    __syncthreads();
  }
  for (int k = threadIdx.x; k < Nb; k += 256) {
    bool kp = false;
    for (int p = 0; p < P; ++p) kp |= sbest[p] == k;
    if (Q) {  // predict.py:94-101: the points in order, each writes bool(label) into the masks it hits
      bool pk = tab.all_neg != 0;
      for (int q = 0; q < Q; ++q)
        if (hit[(long)q * ld + n0 + k]) pk = tab.pt[q][2] != 0;
      kp |= pk;
    }
    keep[n0 + k] = kp ? 1 : 0;
  }
}

static inline int mp_slots(int P) { return P + 1 <= 2 ? 2 : P + 1 <= 5 ? 5 : P + 1 <= 17 ? 17 : 33; }
#define MP_LDS_MAX (160 * 1024 - 4096)  // dynamic LDS of mp_score next to its static arrays

extern "C" size_t ey_mask_prompt_workspace_bytes(int B, int mh, int mw, int P) {
  if (B < 0 || mh <= 0 || mw <= 0 || P < 0 || P > MP_MAXP) return 0;
  return ((size_t)B * (size_t)(mh + mw) * mp_slots(P) * sizeof(float) + 15) / 16 * 16;
}

template <int NB>
static int mp_launch_score(const mp_tab& tab, int mh, int mw, long N, const uint8_t* masks, const float* W, long ld, float* full, float* inter, uint8_t* hit,
                           hipStream_t st) {
  const size_t lds = (size_t)(mh + mw) * NB * sizeof(float) + (size_t)(mh + 3) / 4 * 4;
  if (!ey_lds_reserve<mp_score<NB>>(lds)) return ey_set_error(EY_EUNSUPPORTED, "mask_prompt: %zu bytes of LDS were refused", lds);
  hipLaunchKernelGGL(mp_score<NB>, dim3((unsigned)N), dim3(256), lds, st, tab, mh, mw, masks, W, ld, full, inter, hit);
  EY_LAUNCH_CHECK("ey_mask_prompt (score)");
  return EY_OK;
}

extern "C" int ey_mask_prompt(int B, int mh, int mw, const uint8_t* masks, const int* mask_off, const int* geo, int P, const int* boxes, int Q, const int* points,
                              const int* labels, long ld, float* full, float* inter, float* iou, int* best, uint8_t* hit, uint8_t* keep, void* workspace,
                              size_t workspace_bytes, ey_stream_t stream) {
  EY_CHECK(B >= 0 && mh > 0 && mw > 0 && P >= 0 && Q >= 0, "mask_prompt: B=%d mh=%d mw=%d P=%d Q=%d", B, mh, mw, P, Q);
  EY_CHECK(P + Q > 0, "mask_prompt: no prompt (P = Q = 0)");
  EY_CHECK(mask_off && geo && (P == 0 || boxes) && (Q == 0 || (points && labels)), "mask_prompt: null table");
  if (B > MP_MAXB) return ey_set_error(EY_EUNSUPPORTED, "mask_prompt: B=%d (up to %d images per call are built)", B, MP_MAXB);
  if (P > MP_MAXP || Q > MP_MAXQ) return ey_set_error(EY_EUNSUPPORTED, "mask_prompt: P=%d Q=%d (up to %d boxes and %d points are built)", P, Q, MP_MAXP, MP_MAXQ);
  if ((long)mh * mw > (1L << 24)) return ey_set_error(EY_EUNSUPPORTED, "mask_prompt: %d x %d mask pixels (up to 2^24 are built)", mh, mw);
  const int NB = mp_slots(P);
  if ((size_t)(mh + mw) * NB * sizeof(float) + (size_t)mh + 4 > MP_LDS_MAX)
    return ey_set_error(EY_EUNSUPPORTED, "mask_prompt: the weights of %d boxes over %d + %d mask rows and columns exceed the LDS (%d bytes)", P, mh, mw, MP_LDS_MAX);
  EY_CHECK(mask_off[0] == 0, "mask_prompt: mask_off[0]=%d must be 0", mask_off[0]);
  mp_tab tab = {};
  tab.B = B;
  tab.P = P;
  tab.Q = Q;
  for (int b = 0; b < B; ++b) {
    EY_CHECK(mask_off[b + 1] >= mask_off[b], "mask_prompt: offsets of image %d decrease", b);
    tab.off[b + 1] = mask_off[b + 1];
    const int* g = geo + 6 * b;
    EY_CHECK(0 <= g[0] && g[0] < g[1] && g[1] <= mh && 0 <= g[2] && g[2] < g[3] && g[3] <= mw && g[4] >= 1 && g[5] >= 1,
             "mask_prompt: image %d: crop rows %d..%d, columns %d..%d of a %d x %d mask, target %d x %d", b, g[0], g[1], g[2], g[3], mh, mw, g[4], g[5]);
    if (g[4] > MP_MAXC || g[5] > MP_MAXC) return ey_set_error(EY_EUNSUPPORTED, "mask_prompt: image %d: target %d x %d (up to %d)", b, g[4], g[5], MP_MAXC);
    for (int k = 0; k < 6; ++k) tab.geo[b][k] = g[k];
  }
  for (int p = 0; p < P; ++p) {
    const int* r = boxes + 4 * p;
    EY_CHECK(r[0] >= 0 && r[1] >= 0 && r[2] > r[0] && r[3] > r[1], "mask_prompt: box %d = (%d, %d, %d, %d): needs 0 <= x1 < x2, 0 <= y1 < y2", p, r[0], r[1], r[2], r[3]);
    if (r[2] > MP_MAXC || r[3] > MP_MAXC) return ey_set_error(EY_EUNSUPPORTED, "mask_prompt: box %d reaches (%d, %d) (up to %d)", p, r[2], r[3], MP_MAXC);
    for (int k = 0; k < 4; ++k) tab.box[p][k] = r[k];
  }
  int lab_sum = 0;
  for (int q = 0; q < Q; ++q) {
    const int x = points[2 * q], y = points[2 * q + 1];
    for (int b = 0; b < B; ++b)
      EY_CHECK(x >= 0 && y >= 0 && x < geo[6 * b + 5] && y < geo[6 * b + 4], "mask_prompt: point %d = (%d, %d) is outside image %d (%d x %d)", q, x, y, b, geo[6 * b + 4],
               geo[6 * b + 5]);
    tab.pt[q][0] = x;
    tab.pt[q][1] = y;
    tab.pt[q][2] = labels[q];
    lab_sum += labels[q];
  }
  tab.all_neg = Q > 0 && lab_sum == 0;  // predict.py:95: `labels.sum() == 0`
  const long N = B ? mask_off[B] : 0;
  if (N >= (1L << 31) / 2) return ey_set_error(EY_EUNSUPPORTED, "mask_prompt: %ld masks in one call", N);
  if (B == 0) return EY_OK;
  EY_CHECK(ld >= N, "mask_prompt: row stride %ld of the outputs is below the %ld masks", ld, N);
  EY_CHECK(full && keep && (P == 0 || (inter && iou && best)) && (Q == 0 || hit) && workspace && (N == 0 || masks), "mask_prompt: null pointer");
  EY_CHECK(ey_aligned(workspace, 16) && ey_aligned(full, 4) && ey_aligned(inter, 4) && ey_aligned(iou, 4) && ey_aligned(best, 4), "mask_prompt: misaligned buffer");
  const size_t need = ey_mask_prompt_workspace_bytes(B, mh, mw, P);
  EY_CHECK(workspace_bytes >= need, "mask_prompt: workspace of %zu bytes, needs %zu (ey_mask_prompt_workspace_bytes)", workspace_bytes, need);
  hipStream_t st = (hipStream_t)stream;
  float* W = (float*)workspace;
  if (N) {
    hipLaunchKernelGGL(mp_weights, dim3((unsigned)ey_cdiv((long)(mh > mw ? mh : mw) * NB, 256), 2, (unsigned)B), dim3(256), 0, st, tab, mh, mw, NB, W);
    EY_LAUNCH_CHECK("ey_mask_prompt (weights)");
    int rc;
    switch (NB) {
      case 2: rc = mp_launch_score<2>(tab, mh, mw, N, masks, W, ld, full, inter, hit, st); break;
      case 5: rc = mp_launch_score<5>(tab, mh, mw, N, masks, W, ld, full, inter, hit, st); break;
      case 17: rc = mp_launch_score<17>(tab, mh, mw, N, masks, W, ld, full, inter, hit, st); break;
      default: rc = mp_launch_score<33>(tab, mh, mw, N, masks, W, ld, full, inter, hit, st); break;
    }
    if (rc != EY_OK) return rc;
  }
  hipLaunchKernelGGL(mp_select, dim3((unsigned)B), dim3(256), 0, st, tab, ld, (const float*)full, (const float*)inter, (const uint8_t*)hit, iou, best, keep);
  EY_LAUNCH_CHECK("ey_mask_prompt (select)");
  return EY_OK;
}

// ---- scale_masks (utils/ops.py:716-737): crop, then F.interpolate(mode="bilinear", align_corners=False) to (H0, W0)
template <typename Tin, typename Tout>
__global__ __launch_bounds__(256) void scale_masks_kernel(long planes, int H, int W, int top, int bottom, int left, int right, int H0, int W0, const Tin* __restrict__ x,
                                                          Tout* __restrict__ y) {
  const long total = planes * H0 * W0;
  for (long t = (long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long)gridDim.x * 256) {
    const int ox = (int)(t % W0), oy = (int)((t / W0) % H0);
    const long pl = t / ((long)W0 * H0);
    const mp_src sy = mp_source(oy, bottom - top, H0), sx = mp_source(ox, right - left, W0);
    const Tin* r0 = x + (pl * H + top + sy.i0) * W + left;
    const Tin* r1 = x + (pl * H + top + sy.i1) * W + left;
    const float a = (float)r0[sx.i0], b = (float)r0[sx.i1], c = (float)r1[sx.i0], d = (float)r1[sx.i1];
    const float u = __fadd_rn(__fmul_rn(sx.l0, a), __fmul_rn(sx.l1, b)), v = __fadd_rn(__fmul_rn(sx.l0, c), __fmul_rn(sx.l1, d));
    y[t] = (Tout)__fadd_rn(__fmul_rn(sy.l0, u), __fmul_rn(sy.l1, v));
  }
}

extern "C" int ey_scale_masks(int in_dtype, long planes, int H, int W, int top, int bottom, int left, int right, int H0, int W0, const void* x, void* y,
                              ey_stream_t stream) {
  EY_CHECK(in_dtype == EY_F16 || in_dtype == EY_F32 || in_dtype == EY_MASK_U8, "scale_masks: in_dtype=%d (EY_F16, EY_F32 or EY_MASK_U8)", in_dtype);
  EY_CHECK(planes >= 0 && H > 0 && W > 0 && H0 > 0 && W0 > 0, "scale_masks: planes=%ld H=%d W=%d H0=%d W0=%d", planes, H, W, H0, W0);
  EY_CHECK(0 <= top && top < bottom && bottom <= H && 0 <= left && left < right && right <= W, "scale_masks: crop rows %d..%d, columns %d..%d of %d x %d", top, bottom,
           left, right, H, W);
  if (planes == 0) return EY_OK;
  EY_CHECK(x && y, "scale_masks: null pointer");
  const long total = planes * H0 * W0;
  const unsigned grid = (unsigned)((total + 255) / 256 < 256L * 32 ? (total + 255) / 256 : 256L * 32);
  hipStream_t st = (hipStream_t)stream;
  if (in_dtype == EY_MASK_U8)
    hipLaunchKernelGGL((scale_masks_kernel<uint8_t, float>), dim3(grid), dim3(256), 0, st, planes, H, W, top, bottom, left, right, H0, W0, (const uint8_t*)x, (float*)y);
  else if (in_dtype == EY_F16)
    hipLaunchKernelGGL((scale_masks_kernel<f16, f16>), dim3(grid), dim3(256), 0, st, planes, H, W, top, bottom, left, right, H0, W0, (const f16*)x, (f16*)y);
  else
    hipLaunchKernelGGL((scale_masks_kernel<float, float>), dim3(grid), dim3(256), 0, st, planes, H, W, top, bottom, left, right, H0, W0, (const float*)x, (float*)y);
  EY_LAUNCH_CHECK("ey_scale_masks");
  return EY_OK;
}
