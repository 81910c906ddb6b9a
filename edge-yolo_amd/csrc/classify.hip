// Image classification (reference ultralytics/nn/modules/head.py:454-476 Classify, data/augment.py:2346 classify_transforms).
//
// ey_classify_pool: Classify.conv (1x1, BN folded, activation) + AdaptiveAvgPool2d(1) + flatten as one launch: the (B, Cout, H, W) map never
//   exists.  A workgroup owns one image and CP_NT output channels; tiles of the image's pixel rows are staged in LDS, every wave multiplies
//   them with its 32 weight rows (f16: MFMA 16x16x32 with fp32 accumulation; fp32: a k-ordered fmaf chain, one channel per thread), adds the
//   bias, activates, and adds the pixels of the tile into per-channel fp32 sums.  out = sum / (float)(H W): one IEEE division.
// ey_classify_linear_softmax: Classify.linear + softmax(1) + the top-min(nc, 5) classes as one launch.  A workgroup owns IB images: the
//   pooled rows sit in LDS, a wave computes four class rows at a time for all of them (lanes along K, 16-byte weight loads, fp32 fmaf, butterfly
//   sum), then the block does the max-subtracted softmax and five rounds of arg-max.  Equal probabilities rank the lower class first.
// ey_classify_transform: torchvision Resize(S) + CenterCrop(S) + ToTensor on uint8 BGR images in one launch: a thread owns one output pixel
//   of the crop and evaluates Pillow's antialiased BILINEAR filter for it directly from the source (filter weights in double, pixel sums in
//   fp32, no uint8 intermediate).
//
// Compiled without FMA contraction; the fmaf calls are explicit.
#include "common.h"

#define CP_THREADS 256
#define CP_NT 128       // output channels per workgroup of the MFMA kernel (32 per wave)
#define CP_LDS (64 * 1024)
#define CP_MAXC1 4096   // f16: up to 2016 the 16 pixel rows of (C1 + 16) f16 stay inside 64 KiB, wider tiles (2048 of the ResNets) take up to 129 KiB
                        // of the CU's 160 KiB as dynamic LDS; fp32: tp = (64 KiB / (4 C1)) & ~3 pixel rows, exactly 4 at C1 = 4096
#define CL_THREADS 1024
#define CL_ROWS 4      // class rows a wave has in flight
#define CL_MAXNC 8192
#define CL_MAXK 4096
#define CL_TOPK 5

// ---------------------------------------------------------------------------------------------------------------- conv + pool, f16 MFMA
// LDS tile [tp pixels][kp + 16] f16, kp = C1 rounded up to 32 (zero filled): rows of 2 (mod 4) 16-byte units, the pitch at which the 16-byte
// fragment reads of a wave (lane (r, g): row r at +16 g bytes) are conflict-free (ey_conv_kpad's rule).  A and B fragments of the
// 16x16x32 MFMA take the same 8 consecutive k per lane, so the weight rows are read with 16-byte loads straight from global memory.
__global__ __launch_bounds__(CP_THREADS) void classify_pool_mfma_kernel(const f16* __restrict__ x, int HW, int C1, int cs, const f16* __restrict__ w,
                                                                        const float* __restrict__ bias, int Cout, int act, float* __restrict__ out, int tp, int kp, int vec) {
  extern __shared__ f16 cp_a[];
  const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int pitch = kp + 16;
  const int nw0 = blockIdx.x * CP_NT + wave * 32;
  const f16* xb = x + (long)b * HW * cs;
  bool non[2];
  float bv[2], csum[2];
  const f16* wr[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    non[j] = nw0 + 16 * j < Cout;  // (wave-uniform: Cout is a multiple of 16)
    bv[j] = non[j] ? bias[nw0 + 16 * j + r] : 0.f;
    wr[j] = w + (long)(non[j] ? nw0 + 16 * j + r : 0) * C1 + 8 * g;
    csum[j] = 0.f;
  }
  const int nch = kp >> 3;
  for (int p0 = 0; p0 < HW; p0 += tp) {
    const int np = min(tp, HW - p0);
    __syncthreads();  // the last tile's fragments are read
    for (int i = tid; i < tp * nch; i += CP_THREADS) {
      const int p = i / nch, c0 = (i - p * nch) * 8;
      Vec8<f16> v;
      v.zero();
      if (p < np && c0 < C1) {  // C1 is a multiple of 8: a chunk lies inside the window or outside it
        const f16* s = xb + (long)(p0 + p) * cs + c0;
        if (vec) v.load(s);
        else {
#pragma unroll
          for (int j = 0; j < 8; ++j) v.v[j] = s[j];
        }
      }
      *reinterpret_cast<f16x8*>(cp_a + p * pitch + c0) = v.v;
    }
    __syncthreads();
    const int mts = (np + 15) >> 4;
    f32x4 acc[4][2];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) acc[mt][0] = acc[mt][1] = (f32x4)0.f;
    for (int k = 0; k < kp; k += 32) {
      const bool kon = k + 8 * g < C1;
      f16x8 bf[2];
#pragma unroll
      for (int j = 0; j < 2; ++j) bf[j] = (non[j] && kon) ? *reinterpret_cast<const f16x8*>(wr[j] + k) : (f16x8)(f16)0;
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) {
        if (mt < mts) {  // (workgroup-uniform)
          const f16x8 a = *reinterpret_cast<const f16x8*>(cp_a + (mt * 16 + r) * pitch + k + 8 * g);
          acc[mt][0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, bf[0], acc[mt][0], 0, 0, 0);
          acc[mt][1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, bf[1], acc[mt][1], 0, 0, 0);
        }
      }
    }
    // lane (r, g) holds pixels mt*16 + 4g + i of channel r: bias, activation, then the tile's share of the channel sum
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
      if (mt < mts) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          float v[4];
#pragma unroll
          for (int i = 0; i < 4; ++i) v[i] = acc[mt][j][i] + bv[j];
          ey_act_n<4>(v, act);
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (mt * 16 + 4 * g + i < np) csum[j] += v[i];
        }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    float s = csum[j];
    s += __shfl_xor(s, 16);
    s += __shfl_xor(s, 32);
    if (g == 0 && non[j]) out[(long)b * Cout + nw0 + 16 * j + r] = s / (float)HW;
  }
}

// ---------------------------------------------------------------------------------------------------------------- conv + pool, fp32 VALU
// LDS tile [tp pixels][C1] fp32 (rows past the image zero filled); a thread owns one output channel and walks its weight row once per
// four pixels; the LDS reads are broadcasts
__global__ __launch_bounds__(CP_THREADS) void classify_pool_f32_kernel(const float* __restrict__ x, int HW, int C1, int cs, const float* __restrict__ w,
                                                                       const float* __restrict__ bias, int Cout, int act, float* __restrict__ out, int tp, int vec) {
  extern __shared__ float cp_x[];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int c = blockIdx.x * CP_THREADS + tid;
  const bool on = c < Cout;
  const float* xb = x + (long)b * HW * cs;
  const float* wr = w + (long)(on ? c : 0) * C1;
  const float bv = on ? bias[c] : 0.f;
  const int nch = C1 >> 3;
  float sum = 0.f;
  for (int p0 = 0; p0 < HW; p0 += tp) {
    const int np = min(tp, HW - p0);
    __syncthreads();
    for (int i = tid; i < tp * nch; i += CP_THREADS) {
      const int p = i / nch, c0 = (i - p * nch) * 8;
      Vec8<float> v;
      v.zero();
      if (p < np) {
        const float* s = xb + (long)(p0 + p) * cs + c0;
        if (vec) v.load(s);
        else {
#pragma unroll
          for (int j = 0; j < 8; ++j) v.set(j, s[j]);
        }
      }
      v.store(cp_x + p * C1 + c0);
    }
    __syncthreads();
    if (on) {
      for (int p = 0; p < np; p += 4) {  // (tp is a multiple of 4: rows p..p+3 exist in the tile)
        float a[4] = {0.f, 0.f, 0.f, 0.f};
        for (int k = 0; k < C1; k += 4) {
          const f32x4 wv = *reinterpret_cast<const f32x4*>(wr + k);
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const f32x4 xv = *reinterpret_cast<const f32x4*>(cp_x + (p + q) * C1 + k);
#pragma unroll
            for (int e = 0; e < 4; ++e) a[q] = __builtin_fmaf(xv[e], wv[e], a[q]);
          }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) a[q] += bv;
        ey_act_n<4>(a, act);
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (p + q < np) sum += a[q];
      }
    }
  }
  if (on) out[(long)b * Cout + c] = sum / (float)HW;
}

extern "C" int ey_classify_pool(int dtype, int B, int HW, int C1, int Cout, int act, const void* x, int x_cstride, const void* w, const float* bias, float* out,
                                ey_stream_t stream) {
  EY_CHECK(dtype == EY_F16 || dtype == EY_F32, "classify_pool: bad dtype");
  EY_CHECK(act >= EY_ACT_NONE && act <= EY_ACT_SIGMOID, "classify_pool: act=%d", act);
  EY_CHECK(B > 0 && HW > 0 && C1 > 0 && Cout > 0, "classify_pool: bad extent B=%d HW=%d C1=%d Cout=%d", B, HW, C1, Cout);
  EY_CHECK(x && w && bias && out, "classify_pool: null pointer");
  EY_CHECK(x_cstride >= C1, "classify_pool: pixel stride %d < C1=%d", x_cstride, C1);
  if (C1 % 8 || C1 > CP_MAXC1) return ey_set_error(EY_EUNSUPPORTED, "classify_pool: C1=%d (multiples of 8 up to %d are built)", C1, CP_MAXC1);
  if (dtype == EY_F16 && Cout % 16) return ey_set_error(EY_EUNSUPPORTED, "classify_pool: Cout=%d (f16: multiples of 16 are built)", Cout);
  if (B > 65535 || (long)B * HW * x_cstride >= (1L << 31) || (long)Cout * C1 >= (1L << 31))
    return ey_set_error(EY_EUNSUPPORTED, "classify_pool: view too large (B=%d HW=%d cstride=%d)", B, HW, x_cstride);
  EY_CHECK(ey_aligned(w, 16), "classify_pool: the weight must be 16-byte aligned");
  const size_t es = dtype == EY_F16 ? 2 : 4;
  const int vec = ey_aligned(x, 16) && ((size_t)x_cstride * es) % 16 == 0;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == EY_F16) {
    const int kp = (C1 + 31) & ~31;
    int tp = 64;
    while (tp > 16 && (size_t)tp * (kp + 16) * 2 > CP_LDS) tp >>= 1;
    while (tp > 16 && tp / 2 >= HW) tp >>= 1;
    const size_t lds = (size_t)tp * (kp + 16) * 2;  // C1 <= 2016: at most 64 KiB, the launch every earlier width has always had
    // wider tiles: the kernel's dynamic LDS limit is raised to the widest supported tile (16 rows of 4096 + 16 halves).  The attribute belongs to
    // the function on the CURRENT device, so it is set on every such launch (a host-side call, legal during stream capture), not once per process
    if (lds > CP_LDS && hipFuncSetAttribute((const void*)classify_pool_mfma_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 16 * (CP_MAXC1 + 16) * 2) != hipSuccess)
      return ey_set_error(EY_EUNSUPPORTED, "classify_pool: %zu bytes of LDS for C1=%d refused by the runtime", lds, C1);
    hipLaunchKernelGGL(classify_pool_mfma_kernel, dim3(ey_cdiv(Cout, CP_NT), B), dim3(CP_THREADS), lds, st, (const f16*)x, HW, C1, x_cstride, (const f16*)w, bias, Cout,
                       act, out, tp, kp, vec);
  } else {
    int tp = (int)(CP_LDS / ((size_t)C1 * 4)) & ~3;
    if (tp > 64) tp = 64;
    while (tp > 4 && tp - 4 >= HW) tp -= 4;
    const size_t lds = (size_t)tp * C1 * 4;
    hipLaunchKernelGGL(classify_pool_f32_kernel, dim3(ey_cdiv(Cout, CP_THREADS), B), dim3(CP_THREADS), lds, st, (const float*)x, HW, C1, x_cstride, (const float*)w, bias,
                       Cout, act, out, tp, vec);
  }
  EY_LAUNCH_CHECK("ey_classify_pool");
  return EY_OK;
}

// ---------------------------------------------------------------------------------------------------------------- linear + softmax + top-k
struct ClBest {
  float p;
  int i;
};
// the ranking: higher probability first, equal probabilities by the lower class index
__device__ __forceinline__ bool cl_before(float pa, int ia, float pb, int ib) { return pa > pb || (pa == pb && ia < ib); }

__device__ __forceinline__ float cl_block_max(float v, float* red) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  __syncthreads();
  if (lane == 0) red[wave] = v;
  __syncthreads();
  float m = red[0];
  for (int i = 1; i < CL_THREADS / 64; ++i) m = fmaxf(m, red[i]);
  return m;
}
__device__ __forceinline__ float cl_block_sum(float v, float* red) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  __syncthreads();
  if (lane == 0) red[wave] = v;
  __syncthreads();
  float s = red[0];
  for (int i = 1; i < CL_THREADS / 64; ++i) s += red[i];
  return s;
}

// LDS: pooled [IB][K] fp32, then logits / probabilities [IB][nc] fp32
template <typename T, int IB>
__global__ __launch_bounds__(CL_THREADS) void classify_linear_softmax_kernel(const float* __restrict__ pooled, int B, int K, const T* __restrict__ w, const float* __restrict__ bias,
                                                                             int nc, float* __restrict__ logits, float* __restrict__ probs, int* __restrict__ topi,
                                                                             float* __restrict__ topp, int kk) {
  extern __shared__ float cl_lds[];
  __shared__ float red[CL_THREADS / 64];
  __shared__ float red_p[CL_THREADS / 64];
  __shared__ int red_i[CL_THREADS / 64];
  float* xs = cl_lds;
  float* ls = cl_lds + IB * K;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b0 = blockIdx.x * IB;
  const int nb = min(IB, B - b0);
  for (int i = tid; i < IB * K; i += CL_THREADS) {
    const int ib = i / K;
    xs[i] = ib < nb ? pooled[(long)b0 * K + i] : 0.f;
  }
  __syncthreads();
  for (int c0 = wave * CL_ROWS; c0 < nc; c0 += CL_THREADS / 64 * CL_ROWS) {  // CL_ROWS independent load streams per wave: the loop is latency-bound
    const T* wr[CL_ROWS];
    float acc[CL_ROWS][IB];
#pragma unroll
    for (int q = 0; q < CL_ROWS; ++q) {
      wr[q] = w + (long)min(c0 + q, nc - 1) * K;  // (rows past nc repeat the last one; their sums are not stored)
#pragma unroll
      for (int ib = 0; ib < IB; ++ib) acc[q][ib] = 0.f;
    }
    for (int k = lane * 8; k < K; k += 64 * 8) {
      Vec8<T> wv[CL_ROWS];
#pragma unroll
      for (int q = 0; q < CL_ROWS; ++q) wv[q].load(wr[q] + k);
#pragma unroll
      for (int ib = 0; ib < IB; ++ib) {
        Vec8<float> xv;
        xv.load(xs + ib * K + k);
#pragma unroll
        for (int q = 0; q < CL_ROWS; ++q) {
#pragma unroll
          for (int e = 0; e < 8; ++e) acc[q][ib] = __builtin_fmaf(wv[q].get(e), xv.get(e), acc[q][ib]);
        }
      }
    }
#pragma unroll
    for (int q = 0; q < CL_ROWS; ++q) {
#pragma unroll
      for (int ib = 0; ib < IB; ++ib) {
        float s = acc[q][ib];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
        if (lane == 0 && c0 + q < nc) ls[ib * nc + c0 + q] = s + bias[c0 + q];
      }
    }
  }
  __syncthreads();
  for (int ib = 0; ib < nb; ++ib) {  // (workgroup-uniform)
    const long row = (long)(b0 + ib) * nc;
    float* l = ls + ib * nc;
    float m = -INFINITY;
    for (int c = tid; c < nc; c += CL_THREADS) {
      logits[row + c] = l[c];
      m = fmaxf(m, l[c]);
    }
    m = cl_block_max(m, red);
    float s = 0.f;
    for (int c = tid; c < nc; c += CL_THREADS) {
      const float e = expf(l[c] - m);
      l[c] = e;  // (a thread re-reads only what it wrote)
      s += e;
    }
    s = cl_block_sum(s, red);
    for (int c = tid; c < nc; c += CL_THREADS) {
      const float p = l[c] / s;
      l[c] = p;
      probs[row + c] = p;
    }
    __syncthreads();
    // kk rounds of arg-max over the classes ranked after the last winner
    float lp = INFINITY;
    int li = -1;
    for (int t = 0; t < kk; ++t) {
      float bp = -1.f;
      int bi = -1;
      for (int c = tid; c < nc; c += CL_THREADS) {
        const float p = l[c];
        if (cl_before(lp, li, p, c) && (bi < 0 || cl_before(p, c, bp, bi))) { bp = p; bi = c; }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const float op = __shfl_xor(bp, o);
        const int oi = __shfl_xor(bi, o);
        if (oi >= 0 && (bi < 0 || cl_before(op, oi, bp, bi))) { bp = op; bi = oi; }
      }
      __syncthreads();
      if (lane == 0) { red_p[wave] = bp; red_i[wave] = bi; }
      __syncthreads();
      bp = red_p[0];
      bi = red_i[0];
      for (int i = 1; i < CL_THREADS / 64; ++i)
        if (red_i[i] >= 0 && (bi < 0 || cl_before(red_p[i], red_i[i], bp, bi))) { bp = red_p[i]; bi = red_i[i]; }
      if (bi < 0) {  // (workgroup-uniform) no class left that compares (a row of NaN): index -1 from here on
        if (tid == 0)
          for (int u = t; u < kk; ++u) {
            topi[(long)(b0 + ib) * kk + u] = -1;
            topp[(long)(b0 + ib) * kk + u] = 0.f;
          }
        break;
      }
      if (tid == 0) {
        topi[(long)(b0 + ib) * kk + t] = bi;
        topp[(long)(b0 + ib) * kk + t] = bp;
      }
      lp = bp;
      li = bi;
    }
    __syncthreads();
  }
}

extern "C" int ey_classify_linear_softmax(int dtype, int B, int K, int nc, const float* pooled, const void* w, const float* bias, float* logits, float* probs,
                                          int32_t* topk_index, float* topk_prob, ey_stream_t stream) {
  EY_CHECK(dtype == EY_F16 || dtype == EY_F32, "classify_linear_softmax: bad dtype");
  EY_CHECK(B > 0 && K > 0 && nc > 0, "classify_linear_softmax: bad extent B=%d K=%d nc=%d", B, K, nc);
  if (nc > CL_MAXNC) return ey_set_error(EY_EUNSUPPORTED, "classify_linear_softmax: nc=%d (1 to %d classes are built)", nc, CL_MAXNC);
  if (K % 8 || K > CL_MAXK) return ey_set_error(EY_EUNSUPPORTED, "classify_linear_softmax: K=%d (multiples of 8 up to %d are built)", K, CL_MAXK);
  EY_CHECK(pooled && w && bias && logits && probs && topk_index && topk_prob, "classify_linear_softmax: null pointer");
  EY_CHECK(ey_aligned(w, 16), "classify_linear_softmax: the weight must be 16-byte aligned");
  if ((long)B * nc >= (1L << 31) || (long)B * K >= (1L << 31)) return ey_set_error(EY_EUNSUPPORTED, "classify_linear_softmax: B=%d too large", B);
  const int kk = nc < CL_TOPK ? nc : CL_TOPK;
  // four images per workgroup (a quarter of the weight traffic) once there are enough images to fill the chip that way
  const bool four = B >= 128 && (size_t)4 * (K + nc) * 4 <= CP_LDS;
  const int ib = four ? 4 : 1;
  const size_t lds = (size_t)ib * (K + nc) * 4;
  const dim3 grid(ey_cdiv(B, ib));
  hipStream_t st = (hipStream_t)stream;
#define CL_LAUNCH(T, IB) \
  hipLaunchKernelGGL((classify_linear_softmax_kernel<T, IB>), grid, dim3(CL_THREADS), lds, st, pooled, B, K, (const T*)w, bias, nc, logits, probs, topk_index, topk_prob, kk)
  if (dtype == EY_F16) {
    if (four) CL_LAUNCH(f16, 4);
    else CL_LAUNCH(f16, 1);
  } else {
    if (four) CL_LAUNCH(float, 4);
    else CL_LAUNCH(float, 1);
  }
#undef CL_LAUNCH
  EY_LAUNCH_CHECK("ey_classify_linear_softmax");
  return EY_OK;
}

// ---------------------------------------------------------------------------------------------------------------- image transform
// Pillow's resample coefficients (src/libImaging/Resample.c precompute_coeffs, bilinear support 1) of output index i, in double as Pillow
// computes them: taps [lo, hi), weight of tap t = max(0, 1 - |(t - center + 0.5) / fs|) / sum
struct CtAxis {
  int lo, hi;
  double center, inv_fs, sum;
};
__device__ __forceinline__ double ct_weight(const CtAxis& a, int t) {
  const double v = 1.0 - fabs(((double)t - a.center + 0.5) * a.inv_fs);
  return v > 0.0 ? v : 0.0;
}
__device__ __forceinline__ CtAxis ct_axis(int i, int in, int out) {
  CtAxis a;
  const double scale = (double)in / (double)out;
  const double fs = scale > 1.0 ? scale : 1.0;
  a.center = ((double)i + 0.5) * scale;
  a.inv_fs = 1.0 / fs;
  a.lo = (int)(a.center - fs + 0.5);
  a.lo = a.lo < 0 ? 0 : a.lo;
  a.hi = (int)(a.center + fs + 0.5);
  a.hi = a.hi > in ? in : a.hi;
  double s = 0.0;
  for (int t = a.lo; t < a.hi; ++t) s += ct_weight(a, t);
  a.sum = s;
  return a;
}

template <typename T>
__global__ __launch_bounds__(256) void classify_transform_kernel(const uint8_t* __restrict__ src, int h, int w, long row_bytes, long image_bytes, T* __restrict__ dst, int S,
                                                                 int nh, int nw, int top, int left, int swap_rb) {
  const int ox = blockIdx.x * 64 + threadIdx.x, oy = blockIdx.y * 4 + threadIdx.y, b = blockIdx.z;
  if (ox >= S || oy >= S) return;
  const CtAxis ay = ct_axis(oy + top, h, nh), ax = ct_axis(ox + left, w, nw);
  const uint8_t* img = src + (long)b * image_bytes;
  float acc[3] = {0.f, 0.f, 0.f};
  for (int y = ay.lo; y < ay.hi; ++y) {
    const float wy = (float)(ct_weight(ay, y) / ay.sum);
    const uint8_t* row = img + (long)y * row_bytes;
    float ra[3] = {0.f, 0.f, 0.f};
    for (int xx = ax.lo; xx < ax.hi; ++xx) {
      const float wx = (float)(ct_weight(ax, xx) / ax.sum);
      const uint8_t* px = row + (long)xx * 3;
#pragma unroll
      for (int c = 0; c < 3; ++c) ra[c] = __builtin_fmaf(wx, (float)px[c], ra[c]);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) acc[c] = __builtin_fmaf(wy, ra[c], acc[c]);
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int ch = swap_rb ? 2 - c : c;
    dst[(((long)b * 3 + ch) * S + oy) * S + ox] = from_f<T>(acc[c] / 255.f);
  }
}

// round-half-to-even of d / 2 for d >= 0 (Python's round((n - S) / 2.0))
static inline int ct_crop(int d) {
  const int k = d >> 1;
  return (d & 1) ? k + (k & 1) : k;
}

extern "C" int ey_classify_transform(int out_dtype, const uint8_t* src_hwc, int B, int src_h, int src_w, int src_row_bytes, long src_image_bytes, void* dst_chw, int S,
                                     int swap_rb, ey_stream_t stream) {
  EY_CHECK(out_dtype == EY_F16 || out_dtype == EY_F32, "classify_transform: bad dtype");
  EY_CHECK(src_hwc && dst_chw, "classify_transform: null pointer");
  EY_CHECK(B > 0 && B <= 65535 && src_h > 0 && src_w > 0 && S > 0, "classify_transform: bad extent B=%d %dx%d -> %d", B, src_h, src_w, S);
  EY_CHECK(src_row_bytes >= 3 * src_w && (B == 1 || src_image_bytes >= (long)src_row_bytes * src_h), "classify_transform: row stride %d, image stride %ld", src_row_bytes,
           src_image_bytes);
  if (S > 16384 || src_h > (1 << 20) || src_w > (1 << 20)) return ey_set_error(EY_EUNSUPPORTED, "classify_transform: %dx%d -> %d is too large", src_h, src_w, S);
  // torchvision Resize(S): the shorter side becomes S, the longer int(S * long / short) (true division, truncated)
  int nh, nw;
  if (src_w <= src_h) { nw = S; nh = (int)((double)((long)S * src_h) / (double)src_w); }
  else { nh = S; nw = (int)((double)((long)S * src_w) / (double)src_h); }
  EY_CHECK(nh >= S && nw >= S, "classify_transform: resized %dx%d is smaller than the crop %d", nh, nw, S);
  const int top = ct_crop(nh - S), left = ct_crop(nw - S);
  const dim3 grid(ey_cdiv(S, 64), ey_cdiv(S, 4), B), block(64, 4);
  hipStream_t st = (hipStream_t)stream;
  if (out_dtype == EY_F16)
    hipLaunchKernelGGL(classify_transform_kernel<f16>, grid, block, 0, st, src_hwc, src_h, src_w, (long)src_row_bytes, src_image_bytes, (f16*)dst_chw, S, nh, nw, top, left,
                       swap_rb);
  else
    hipLaunchKernelGGL(classify_transform_kernel<float>, grid, block, 0, st, src_hwc, src_h, src_w, (long)src_row_bytes, src_image_bytes, (float*)dst_chw, S, nh, nw, top,
                       left, swap_rb);
  EY_LAUNCH_CHECK("ey_classify_transform");
  return EY_OK;
}
