// YOLOv9 (GELAN) memory-bound operators: the ADown / AConv pooling front end and the CBFuse resize-and-sum (gfx950).
#include "common.h"

// ============================================================================ ADown / AConv: avg 2x2 s1 -> [write | max 3x3 s2 p1]
// A = avg_pool2d(x, 2, 1, 0), (H-1) x (W-1): fp32 ((x00 + x01) + x10) + x11, times 0.25f, rounded once to T.
// Channels [0, c_avg) of A are written to `a`; channels [c_avg, C) go through max_pool2d(., 3, 2, 1) over the ROUNDED A values and only that
// result is written (`m`); their A values live in LDS.
// block = one image x one band of MR pooled rows (= 2 MR rows of A) x CV consecutive 8-channel vectors, all on one side of the split.
//   first-half group : every A value of rows [2 j0, 2 j0 + 2 MR) is computed once and stored to `a`
//   second-half group: A rows [2 j0 - 1, 2 j0 + 2 MR - 1] (one halo row) are computed into LDS, then each pooled pixel reduces its window from
//                      LDS; window positions outside A are skipped
// Neighbouring blocks (channel groups of one band, then the next band) share input lines, so the work list goes through ey_xcd_block.
template <typename T, int CV>
__global__ __launch_bounds__(256) void adown_kernel(int H, int W, int C, int c_avg, int MR, int nbands, const T* __restrict__ x, int xCs, T* __restrict__ a,
                                                    int aCs, T* __restrict__ m, int mCs) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  Vec8<T>* S = reinterpret_cast<Vec8<T>*>(smem);
  const int Ha = H - 1, Wa = W - 1, Hm = H / 2, Wm = W / 2;
  const int groups = C / (8 * CV);
  unsigned blk = ey_xcd_block(blockIdx.x, gridDim.x);
  const int g = (int)(blk % (unsigned)groups);
  blk /= (unsigned)groups;
  const int band = (int)(blk % (unsigned)nbands), b = (int)(blk / (unsigned)nbands);
  const int c0 = g * 8 * CV, j0 = band * MR;
  const bool pooled = c0 >= c_avg;
  // rows of A this block computes
  const int r_lo = pooled ? max(2 * j0 - 1, 0) : 2 * j0;
  const int r_hi = min(pooled ? 2 * j0 + 2 * MR : 2 * j0 + 2 * MR, Ha);  // exclusive (pooled: rows up to 2 (j0 + MR - 1) + 1)
  const int r_base = 2 * j0 - 1;                                            // A row held by LDS row 0
  const int n = (r_hi - r_lo) * Wa * CV;
  const T* xb = x + (long)b * H * W * xCs + c0;
  for (int i = threadIdx.x; i < n; i += 256) {
    const int v = i % CV, px = i / CV, rr = px / Wa, col = px - rr * Wa, row = r_lo + rr;
    const T* p = xb + ((long)row * W + col) * xCs + v * 8;
    Vec8<T> x00, x01, x10, x11, o;
    x00.load(p);
    x01.load(p + xCs);
    x10.load(p + (long)W * xCs);
    x11.load(p + (long)W * xCs + xCs);
#pragma unroll
    for (int k = 0; k < 8; ++k) o.set(k, (((x00.get(k) + x01.get(k)) + x10.get(k)) + x11.get(k)) * 0.25f);
    if (pooled) S[((row - r_base) * Wa + col) * CV + v] = o;
    else o.store(a + (((long)b * Ha + row) * Wa + col) * aCs + c0 + v * 8);
  }
  if (!pooled) return;  // (uniform over the block)
  __syncthreads();
  const int rows = min(MR, Hm - j0), np = rows * Wm * CV;
  for (int i = threadIdx.x; i < np; i += 256) {
    const int v = i % CV, px = i / CV, jj = px / Wm, q = px - jj * Wm, j = j0 + jj;
    float mx[8];
    bool first = true;
    for (int dy = -1; dy <= 1; ++dy) {
      const int r = 2 * j + dy;
      if (r < 0 || r >= Ha) continue;
      for (int dx = -1; dx <= 1; ++dx) {
        const int c = 2 * q + dx;
        if (c < 0 || c >= Wa) continue;
        const Vec8<T> t = S[((r - r_base) * Wa + c) * CV + v];
#pragma unroll
        for (int k = 0; k < 8; ++k) mx[k] = first ? t.get(k) : fmaxf(mx[k], t.get(k));
        first = false;
      }
    }
    Vec8<T> o;  // (the window's centre (2j, 2q) is always inside A: 2j <= H - 2, 2q <= W - 2)
#pragma unroll
    for (int k = 0; k < 8; ++k) o.set(k, mx[k]);
    o.store(m + (((long)b * Hm + j) * Wm + q) * mCs + (c0 - c_avg) + v * 8);
  }
}

template <typename T, int CV>
static int adown_launch(int B, int H, int W, int C, int c_avg, int MR, const void* x, int xCs, void* a, int aCs, void* m, int mCs, size_t lds, hipStream_t st) {
  const int nbands = ey_cdiv(H / 2, MR);
  const long blocks = (long)B * nbands * (C / (8 * CV));
  if (blocks >= (1L << 31)) return ey_set_error(EY_EUNSUPPORTED, "adown_pool: %ld workgroups", blocks);
  hipLaunchKernelGGL((adown_kernel<T, CV>), dim3((unsigned)blocks), dim3(256), lds, st, H, W, C, c_avg, MR, nbands, (const T*)x, xCs, (T*)a, aCs, (T*)m, mCs);
  return EY_OK;
}

extern "C" int ey_adown_pool(int dtype, int B, int H, int W, int C, int c_avg, const void* x, int x_cstride, void* a, int a_cstride, void* m,
                             int m_cstride, ey_stream_t stream) {
  EY_CHECK(dtype == EY_F16 || dtype == EY_F32, "adown_pool: bad dtype");
  EY_CHECK(B > 0 && H >= 2 && W >= 2, "adown_pool: B=%d, a %dx%d map (H, W >= 2)", B, H, W);
  EY_CHECK(C > 0 && C % 8 == 0 && c_avg > 0 && c_avg <= C && c_avg % 8 == 0, "adown_pool: C=%d, c_avg=%d (multiples of 8, 0 < c_avg <= C)", C, c_avg);
  const int c_max = C - c_avg;
  EY_CHECK(x && a && (m || c_max == 0), "adown_pool: null pointer");
  const size_t es = dtype == EY_F16 ? 2 : 4;
  EY_CHECK(x_cstride >= C && a_cstride >= c_avg && (c_max == 0 || m_cstride >= c_max), "adown_pool: a pixel stride is below its channel count");
  EY_CHECK(((size_t)x_cstride * es) % 16 == 0 && ((size_t)a_cstride * es) % 16 == 0 && ey_aligned(x, 16) && ey_aligned(a, 16) &&
               (c_max == 0 || (((size_t)m_cstride * es) % 16 == 0 && ey_aligned(m, 16))),
           "adown_pool: views must be 16-byte aligned (pixel strides multiples of 16 bytes)");
  // channel group (whole 128-byte lines where possible) that stays on one side of the split, and a band of pooled rows, in order of
  // preference; the first pair whose A rows fit 40 KiB of LDS (four workgroups per CU) is taken, else the first that fits 64 KiB
  int cvmax = 128 / (8 * (int)es);
  while (cvmax > 1 && (c_avg % (8 * cvmax) || c_max % (8 * cvmax))) cvmax >>= 1;
  const size_t row_bytes = (size_t)(W - 1) * 16 * (es / 2);  // one A row of one 8-channel vector
  static const int pref[12][2] = {{8, 4}, {8, 2}, {4, 4}, {4, 2}, {8, 1}, {2, 4}, {4, 1}, {2, 2}, {1, 4}, {2, 1}, {1, 2}, {1, 1}};
  int cv = 0, mr = 0;
  for (size_t cap : {(size_t)40 * 1024, (size_t)64 * 1024}) {
    for (int i = 0; i < 12 && !cv; ++i)
      if (pref[i][0] <= cvmax && (c_max == 0 || (2 * pref[i][1] + 1) * row_bytes * pref[i][0] <= cap)) cv = pref[i][0], mr = pref[i][1];
    if (cv) break;
  }
  if (!cv) return ey_set_error(EY_EUNSUPPORTED, "adown_pool: a row of %d pixels does not fit LDS", W);
  const size_t lds = c_max ? (2 * mr + 1) * row_bytes * cv : 0;
  hipStream_t st = (hipStream_t)stream;
  int rc;
#define EY_ADOWN(TT, CVV) rc = adown_launch<TT, CVV>(B, H, W, C, c_avg, mr, x, x_cstride, a, a_cstride, m, m_cstride, lds, st)
  if (dtype == EY_F16) { if (cv == 8) EY_ADOWN(f16, 8); else if (cv == 4) EY_ADOWN(f16, 4); else if (cv == 2) EY_ADOWN(f16, 2); else EY_ADOWN(f16, 1); }
  else { if (cv == 4) EY_ADOWN(float, 4); else if (cv == 2) EY_ADOWN(float, 2); else EY_ADOWN(float, 1); }
#undef EY_ADOWN
  if (rc != EY_OK) return rc;
  EY_LAUNCH_CHECK("ey_adown_pool");
  return EY_OK;
}

// ============================================================================ CBFuse: nearest-resize n maps to H x W and sum them
// one thread = one output pixel x 8 channels; the source row / column of every map is computed once per thread with PyTorch's rule
// min((int)floorf(dst * scale), in - 1), scale = (float)in / (float)out formed on the host; fp32 sum in list order, one rounding.
struct cbfuse_args {
  const void* p[EY_CBFUSE_MAX];
  int cs[EY_CBFUSE_MAX], Hi[EY_CBFUSE_MAX], Wi[EY_CBFUSE_MAX];
  float sh[EY_CBFUSE_MAX], sw[EY_CBFUSE_MAX];
};

template <typename T>
__global__ __launch_bounds__(256) void cbfuse_kernel(long total, int H, int W, int cvn, int n, cbfuse_args s, T* __restrict__ y, int yCs) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int v = (int)(idx % cvn);
  long px = idx / cvn;
  const int q = (int)(px % W);
  px /= W;
  const int r = (int)(px % H), b = (int)(px / H);
  float acc[8];
#pragma unroll
  for (int i = 0; i < EY_CBFUSE_MAX; ++i) {
    if (i >= n) break;
    const int ri = s.Hi[i] == H ? r : min((int)floorf((float)r * s.sh[i]), s.Hi[i] - 1);
    const int qi = s.Wi[i] == W ? q : min((int)floorf((float)q * s.sw[i]), s.Wi[i] - 1);
    Vec8<T> t;
    t.load(reinterpret_cast<const T*>(s.p[i]) + (((long)b * s.Hi[i] + ri) * s.Wi[i] + qi) * s.cs[i] + v * 8);
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[k] = i == 0 ? t.get(k) : acc[k] + t.get(k);
  }
  Vec8<T> o;
#pragma unroll
  for (int k = 0; k < 8; ++k) o.set(k, acc[k]);
  o.store(y + (((long)b * H + r) * W + q) * yCs + v * 8);
}

extern "C" int ey_cbfuse(int dtype, int B, int H, int W, int C, int n, const ey_cbfuse_src* srcs, void* y, int y_cstride, ey_stream_t stream) {
  EY_CHECK(dtype == EY_F16 || dtype == EY_F32, "cbfuse: bad dtype");
  EY_CHECK(srcs && y, "cbfuse: null pointer");
  EY_CHECK(n >= 1 && n <= EY_CBFUSE_MAX, "cbfuse: %d sources (1..%d)", n, EY_CBFUSE_MAX);
  EY_CHECK(B > 0 && H > 0 && W > 0 && C > 0 && C % 8 == 0, "cbfuse: B=%d %dx%d C=%d (C a multiple of 8)", B, H, W, C);
  const size_t es = dtype == EY_F16 ? 2 : 4;
  EY_CHECK(y_cstride >= C && ((size_t)y_cstride * es) % 16 == 0 && ey_aligned(y, 16), "cbfuse: output view not 16-byte aligned");
  cbfuse_args s = {};
  for (int i = 0; i < n; ++i) {
    EY_CHECK(srcs[i].ptr && srcs[i].Hi > 0 && srcs[i].Wi > 0, "cbfuse: source %d: null pointer or empty map", i);
    EY_CHECK(srcs[i].cstride >= C && ((size_t)srcs[i].cstride * es) % 16 == 0 && ey_aligned(srcs[i].ptr, 16), "cbfuse: source %d view not 16-byte aligned", i);
    s.p[i] = srcs[i].ptr;
    s.cs[i] = srcs[i].cstride;
    s.Hi[i] = srcs[i].Hi;
    s.Wi[i] = srcs[i].Wi;
    s.sh[i] = (float)srcs[i].Hi / (float)H;
    s.sw[i] = (float)srcs[i].Wi / (float)W;
  }
  const long total = (long)B * H * W * (C / 8);
  if ((total + 255) / 256 >= (1L << 31)) return ey_set_error(EY_EUNSUPPORTED, "cbfuse: too many pixels");
  hipStream_t st = (hipStream_t)stream;
  const unsigned blocks = (unsigned)((total + 255) / 256);
  if (dtype == EY_F16) hipLaunchKernelGGL(cbfuse_kernel<f16>, dim3(blocks), dim3(256), 0, st, total, H, W, C / 8, n, s, (f16*)y, y_cstride);
  else hipLaunchKernelGGL(cbfuse_kernel<float>, dim3(blocks), dim3(256), 0, st, total, H, W, C / 8, n, s, (float*)y, y_cstride);
  EY_LAUNCH_CHECK("ey_cbfuse");
  return EY_OK;
}
