// Operators of the classic families (YOLOv3, YOLOv5, YOLOv6): the image stems that are not 3x3 stride 2 -- Conv(3, c, 6, 2, 2) of YOLOv5,
// Conv(3, c, 3, 1, 1) of YOLOv3 and Conv(3, 64, 7, 2, 3) of the ResNet stem (resnet.hip) -- read from the planar NCHW image and written NHWC, and the 2x2 max-pool of YOLOv3-tiny with explicit ZERO
// padding (nn.ZeroPad2d in front of nn.MaxPool2d).
#include "common.h"
#include "tune.h"
#include "stem_ks.inc.h"

// ============================================================================ stems: NCHW image -> NHWC, (k, s, p) = (6, 2, 2), (3, 1, 1), (7, 2, 3)
// Same two forms as the 3x3 stride-2 stem of ops_misc.hip.  The 6x6 window is NOT centred: output pixel o reads the input columns
// 2o - 2 ... 2o + 3 (pad 2 in front, taps 0 ... 5).
// (geometry and the per-pixel device functions: stem_ks.inc.h, shared with the single-launch ResNet stem of resnet.hip)

// MFMA form (f16 image -> f16 NHWC, Cin = 3, W % 8 == 0).  A workgroup stages the 3 x HR x (8 NVC) input patch of an 8 x 64 output tile into LDS
// with range-checked 16-byte loads of the planar image (out of range = the zero padding), then every lane gathers its taps
// (k = c K K + ky K + kx, the OIHW order) with 2-byte LDS reads -- 4-byte reads of tap pairs where window, stride and padding are even --;
// the weights are rounded to f16 once per wave into the A fragments.
template <int NT, int K, int S, int P>
__global__ __launch_bounds__(256) void stem_ks_mfma_kernel(int B, int H, int W, int Ho, int Wo, int act, const f16* __restrict__ x, unsigned xbytes,
                                                           const float* __restrict__ w, const float* __restrict__ bias, f16* __restrict__ y, int yCs) {
  using G = SkGeo<K, S, P>;
  constexpr int HR = G::HR, LW = G::LW, KC = G::KC;
  __shared__ __attribute__((aligned(16))) f16 s_in[3 * HR * LW];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, g = lane >> 4;
  const int tilesX = (Wo + SK_TC - 1) / SK_TC, tilesY = (Ho + SK_TR - 1) / SK_TR;
  const int b = blockIdx.x / (tilesX * tilesY), trem = blockIdx.x - b * (tilesX * tilesY);
  const int oy0 = (trem / tilesX) * SK_TR, ox0 = (trem % tilesX) * SK_TC;
  sk_stage<K, S, P>(s_in, ey_rsrc(x, xbytes), b, H, W, oy0, ox0, tid);
  Vec8<f16> af[NT][KC];
  int off[KC][8];
  float bs[NT][4];
  sk_frags<NT, K, S, P>(w, bias, r, g, af, off, bs);
  __syncthreads();
  // wave w: output rows 2w, 2w+1 of the tile, 4 column blocks of 16 pixels each
#pragma unroll 1
  for (int blk = 0; blk < 8; ++blk) {
    const int rr = 2 * wave + (blk >> 2), j = (blk & 3) * 16 + r;
    f32x4 acc[NT];
    sk_px16<NT, K, S, P>(s_in + (S * rr) * LW + S * j + (8 - P), off, af, acc);
    const int oy = oy0 + rr, ox = ox0 + j;
    if (oy < Ho && ox < Wo) {
      f16* yp = y + (((long)b * Ho + oy) * Wo + ox) * yCs + 4 * g;
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) *reinterpret_cast<f16x4*>(yp + nt * 16) = sk_out(acc[nt], bs[nt], act);
    }
  }
}

// VALU form (fp32, Cin 1..4, any width): the exact-f32 parity mode.  One thread = one output pixel x 16 output channels (sk_valu_px).
template <typename TI, typename TO, int K, int S, int P>
__global__ __launch_bounds__(256) void stem_ks_kernel(int B, int Cin, int H, int W, int Ho, int Wo, int act, const TI* __restrict__ x, unsigned xbytes,
                                                      const float* __restrict__ w, const float* __restrict__ bias, TO* __restrict__ y, int yCs) {
  const long npix = (long)B * Ho * Wo;
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= npix) return;
  const int co0 = blockIdx.y * 16;
  const int ox = (int)(t % Wo);
  const long tt = t / Wo;
  const int oy = (int)(tt % Ho), b = (int)(tt / Ho);
  float acc[16];
  sk_valu_px<TI, K, S, P>(ey_rsrc(x, xbytes), b, Cin, H, W, oy, ox, co0, w, bias, act, acc);
  TO* yp = y + t * yCs + co0;
  Vec8<TO> v;
#pragma unroll
  for (int o = 0; o < 8; ++o) v.set(o, acc[o]);
  v.store(yp);
#pragma unroll
  for (int o = 0; o < 8; ++o) v.set(o, acc[8 + o]);
  v.store(yp + 8);
}

static int g_stem_ks_variant = 0;  // form of the last launch, 1: MFMA, 0: VALU (process-wide, not synchronised: developer tools and tests)
extern "C" int ey_stem_conv_ks_last_variant(void) { return g_stem_ks_variant; }

template <int K, int S, int P>
static int stem_ks_mfma_launch(int B, int H, int W, int Ho, int Wo, int Cout, int act, const void* x, const float* w, const float* bias, void* y, int yCs, hipStream_t st) {
  const long tiles = (long)B * ((Wo + SK_TC - 1) / SK_TC) * ((Ho + SK_TR - 1) / SK_TR);
  if (tiles >= (1L << 31)) return ey_set_error(EY_EUNSUPPORTED, "stem_ks: too many tiles");
#define SKM(NT)                                                                                                                                     \
  hipLaunchKernelGGL((stem_ks_mfma_kernel<NT, K, S, P>), dim3((unsigned)tiles), dim3(256), 0, st, B, H, W, Ho, Wo, act, (const f16*)x, \
                     (unsigned)((long)B * 3 * H * W * 2), w, bias, (f16*)y, yCs)
  switch (Cout / 16) {  // fp32-accumulated f16 products; the weights are rounded to f16 like every other conv of the f16 mode
    case 1: SKM(1); break;
    case 2: SKM(2); break;
    case 3: SKM(3); break;
    case 4: SKM(4); break;
    default: SKM(5); break;
  }
#undef SKM
  EY_LAUNCH_CHECK("ey_stem_conv_ks(mfma)");
  g_stem_ks_variant = 1;
  return EY_OK;
}

template <typename TI, typename TO, int K, int S, int P>
static int stem_ks_launch(int B, int Cin, int H, int W, int Ho, int Wo, int Cout, int act, const void* x, const float* w, const float* bias, void* y, int yCs,
                          hipStream_t st) {
  const long npix = (long)B * Ho * Wo;
  const long xbytes = (long)B * Cin * H * W * (long)sizeof(TI);
  if (xbytes >= (1L << 31) || (npix + 255) / 256 >= (1L << 31)) return ey_set_error(EY_EUNSUPPORTED, "stem_ks: input batch larger than 2 GiB");
  dim3 grid((unsigned)((npix + 255) / 256), Cout / 16);
  hipLaunchKernelGGL((stem_ks_kernel<TI, TO, K, S, P>), grid, dim3(256), 0, st, B, Cin, H, W, Ho, Wo, act, (const TI*)x, (unsigned)xbytes, w, bias, (TO*)y, yCs);
  EY_LAUNCH_CHECK("ey_stem_conv_ks");
  g_stem_ks_variant = 0;
  return EY_OK;
}

template <int K, int S, int P>
static int stem_ks_typed(int x_dtype, int y_dtype, int B, int Cin, int H, int W, int Cout, int act, const void* x, const float* w, const float* bias, void* y,
                         int yCs, hipStream_t st) {
  const int Ho = (H + 2 * P - K) / S + 1, Wo = (W + 2 * P - K) / S + 1;
  if (x_dtype == EY_F16 && y_dtype == EY_F16 && Cin == 3 && W % 8 == 0 && Cout <= 80 && ey_aligned(x, 16) && tune().stem_mfma && (long)B * 3 * H * W * 2 < (1L << 31))
    return stem_ks_mfma_launch<K, S, P>(B, H, W, Ho, Wo, Cout, act, x, w, bias, y, yCs, st);
  if (x_dtype == EY_F16 && y_dtype == EY_F16) return stem_ks_launch<f16, f16, K, S, P>(B, Cin, H, W, Ho, Wo, Cout, act, x, w, bias, y, yCs, st);
  if (x_dtype == EY_F32 && y_dtype == EY_F16) return stem_ks_launch<float, f16, K, S, P>(B, Cin, H, W, Ho, Wo, Cout, act, x, w, bias, y, yCs, st);
  if (x_dtype == EY_F16 && y_dtype == EY_F32) return stem_ks_launch<f16, float, K, S, P>(B, Cin, H, W, Ho, Wo, Cout, act, x, w, bias, y, yCs, st);
  return stem_ks_launch<float, float, K, S, P>(B, Cin, H, W, Ho, Wo, Cout, act, x, w, bias, y, yCs, st);
}

extern "C" int ey_stem_conv_ks(int x_dtype, int y_dtype, int B, int Cin, int H, int W, int Cout, int k, int stride, int pad, int act, const void* x,
                               const float* w, const float* bias, void* y, int y_cstride, ey_stream_t stream) {
  EY_CHECK(x && w && y, "stem_ks: null pointer");
  const bool k6 = k == 6 && stride == 2 && pad == 2, k3 = k == 3 && stride == 1 && pad == 1, k7 = k == 7 && stride == 2 && pad == 3;
  if (!k6 && !k3 && !k7)
    return ey_set_error(EY_EUNSUPPORTED, "stem_ks: (k, s, p) = (%d, %d, %d); (6, 2, 2), (3, 1, 1) and (7, 2, 3) are built, (3, 2, 1) is ey_stem_conv", k, stride, pad);
  EY_CHECK((x_dtype == EY_F16 || x_dtype == EY_F32) && (y_dtype == EY_F16 || y_dtype == EY_F32), "stem_ks: bad dtype");
  EY_CHECK(Cin >= 1 && Cin <= 4 && Cout % 16 == 0 && Cout > 0, "stem_ks: Cin=%d (1..4) Cout=%d (multiple of 16)", Cin, Cout);
  EY_CHECK(B > 0 && H > 0 && W > 0 && H + 2 * pad >= k && W + 2 * pad >= k, "stem_ks: bad extent");
  const int es = y_dtype == EY_F16 ? 2 : 4;
  EY_CHECK(y_cstride >= Cout && (y_cstride * es) % 16 == 0 && ey_aligned(y, 16), "stem_ks: output view not 16-byte aligned");
  EY_CHECK(ey_aligned(x, x_dtype == EY_F16 ? 2 : 4), "stem_ks: image not aligned to its element size");
  hipStream_t st = (hipStream_t)stream;
  if (k7) return stem_ks_typed<7, 2, 3>(x_dtype, y_dtype, B, Cin, H, W, Cout, act, x, w, bias, y, y_cstride, st);
  return k6 ? stem_ks_typed<6, 2, 2>(x_dtype, y_dtype, B, Cin, H, W, Cout, act, x, w, bias, y, y_cstride, st)
            : stem_ks_typed<3, 1, 1>(x_dtype, y_dtype, B, Cin, H, W, Cout, act, x, w, bias, y, y_cstride, st);
}

// ============================================================================ max-pool k 1 / 2, stride 1 / 2, explicit zero padding
// y[b, oy, ox, c] = max over the k x k window at (oy s - pt, ox s - pl) of the map padded with ZEROS by (pl, pr, pt, pb): the padded cells take
// part in the maximum with value 0 (nn.ZeroPad2d in front of nn.MaxPool2d), so an all-negative border gives 0.  Floor output size.  k = 1 is
// the zero-padded copy.  Memory-bound: one thread = one output pixel x 8 channels, range-checked 16-byte loads (out of range = the zero cell),
// work taken in XCD-contiguous order so that the rows two neighbouring outputs share come from one L2.
template <typename T, int K>
__global__ __launch_bounds__(256) void maxpool_kernel(int B, int H, int W, int C, int Ho, int Wo, int s, int pl, int pt, int xcd, const T* __restrict__ x, int xCs,
                                                      unsigned xBytes, T* __restrict__ y, int yCs) {
  const int cv = C >> 3;
  const long idx = (long)(xcd ? ey_xcd_block(blockIdx.x, gridDim.x) : blockIdx.x) * 256 + threadIdx.x;
  if (idx >= (long)B * Ho * Wo * cv) return;
  const int c8 = (int)(idx % cv) * 8;
  const long m = idx / cv;
  const int ox = (int)(m % Wo);
  const long t = m / Wo;
  const int oy = (int)(t % Ho), b = (int)(t / Ho);
  const __amdgpu_buffer_rsrc_t rx = ey_rsrc(x, xBytes);
  Vec8<T> in[K][K];
#pragma unroll
  for (int ky = 0; ky < K; ++ky) {
    const int iy = oy * s - pt + ky;
    const bool yok = iy >= 0 && iy < H;
#pragma unroll
    for (int kx = 0; kx < K; ++kx) {
      const int ix = ox * s - pl + kx;
      const long e = (((long)b * H + iy) * W + ix) * xCs + c8;
      BufLoad8<T>::load(in[ky][kx], rx, (yok && ix >= 0 && ix < W) ? (unsigned)(e * (long)sizeof(T)) : EY_OOB);
    }
  }
  Vec8<T> o;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    float v = in[0][0].get(i);
#pragma unroll
    for (int q = 1; q < K * K; ++q) v = fmaxf(v, in[q / K][q % K].get(i));
    o.set(i, v);
  }
  o.store(y + m * yCs + c8);
}

template <typename T>
static int maxpool_launch(int B, int H, int W, int C, int k, int s, int pl, int pt, int Ho, int Wo, const void* x, int xCs, void* y, int yCs, hipStream_t st) {
  const long total = (long)B * Ho * Wo * (C / 8);
  const long xbytes = (((long)B * H * W - 1) * xCs + C) * (long)sizeof(T);
  if (xbytes >= (1L << 31) || (total + 255) / 256 >= (1L << 31)) return ey_set_error(EY_EUNSUPPORTED, "maxpool2d: view larger than 2 GiB");
  const dim3 grid((unsigned)((total + 255) / 256));
  const int xcd = (int)(tune().xcd_map & 1);
  if (k == 1) hipLaunchKernelGGL((maxpool_kernel<T, 1>), grid, dim3(256), 0, st, B, H, W, C, Ho, Wo, s, pl, pt, xcd, (const T*)x, xCs, (unsigned)xbytes, (T*)y, yCs);
  else hipLaunchKernelGGL((maxpool_kernel<T, 2>), grid, dim3(256), 0, st, B, H, W, C, Ho, Wo, s, pl, pt, xcd, (const T*)x, xCs, (unsigned)xbytes, (T*)y, yCs);
  EY_LAUNCH_CHECK("ey_maxpool2d");
  return EY_OK;
}

extern "C" int ey_maxpool2d(int dtype, int B, int H, int W, int C, int k, int stride, int pad_l, int pad_r, int pad_t, int pad_b, const void* x, int x_cstride,
                            void* y, int y_cstride, ey_stream_t stream) {
  EY_CHECK(x && y, "maxpool2d: null pointer");
  EY_CHECK(dtype == EY_F16 || dtype == EY_F32, "maxpool2d: bad dtype");
  if (!((k == 2 && (stride == 1 || stride == 2)) || (k == 1 && stride == 1)))
    return ey_set_error(EY_EUNSUPPORTED, "maxpool2d: k=%d stride=%d; k = 2 with stride 1 or 2 and the padded copy k = 1, stride 1 are built", k, stride);
  EY_CHECK(pad_l >= 0 && pad_r >= 0 && pad_t >= 0 && pad_b >= 0, "maxpool2d: negative padding");
  EY_CHECK(B > 0 && H > 0 && W > 0 && H + pad_t + pad_b >= k && W + pad_l + pad_r >= k, "maxpool2d: a %dx%d map padded by (%d,%d,%d,%d) has no %dx%d window", H, W, pad_l,
           pad_r, pad_t, pad_b, k, k);
  EY_CHECK(C > 0 && C % 8 == 0, "maxpool2d: C=%d must be a multiple of 8", C);
  const int es = dtype == EY_F16 ? 2 : 4;
  EY_CHECK(x_cstride >= C && y_cstride >= C && (x_cstride * es) % 16 == 0 && (y_cstride * es) % 16 == 0 && ey_aligned(x, 16) && ey_aligned(y, 16),
           "maxpool2d: views must be 16-byte aligned");
  const int Ho = (H + pad_t + pad_b - k) / stride + 1, Wo = (W + pad_l + pad_r - k) / stride + 1;
  return dtype == EY_F16 ? maxpool_launch<f16>(B, H, W, C, k, stride, pad_l, pad_t, Ho, Wo, x, x_cstride, y, y_cstride, (hipStream_t)stream)
                         : maxpool_launch<float>(B, H, W, C, k, stride, pad_l, pad_t, Ho, Wo, x, x_cstride, y, y_cstride, (hipStream_t)stream);
}
