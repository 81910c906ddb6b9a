// Operators of the ResNet classification backbones (ResNetLayer of yolov8-cls-resnet50 / -resnet101).  Layer 0 of a ResNet is a 7x7 stride-2
// convolution from the image followed by a 3x3 stride-2 max-pool; the convolution is the (7, 2, 3) case of ey_stem_conv_ks (classic.hip), the
// pool and the two of them as one launch are here, and so is the closing 1x1 of the bottleneck blocks behind it.
//
// ey_resnet_stem: layer 0 as ONE launch.  A workgroup owns a pooled tile of 3 x 30 pixels.  It computes the 7 x 61 convolution outputs under
//   it -- as an 8 x 64 tile whose first column is 4 columns left of the window, so that the staged image patch starts at a multiple of 8 --
//   with the device functions of ey_stem_conv_ks (stem_ks.inc.h: the same taps in the same order, bias, activation, one rounding), writes them
//   to an LDS tile of 8 x 64 pixels x 64 channels in the output type instead of to memory (convolution outputs outside the map become -inf),
//   and pools from that tile with the compare chain of ey_maxpool3x3s2.  Only the quarter-resolution map is written: bit-identical to
//   ey_stem_conv_ks followed by ey_maxpool3x3s2.  MFMA form (f16, Cin = 3, W % 8 == 0): 19 KiB of staged image + 64 KiB of tile; VALU form
//   (fp32, or f16 at any width): a 128 KiB (f16: 64 KiB) tile; both are dynamic LDS above 64 KiB.  Recomputed: one halo row in seven, and
//   the 8th row and 3 of 64 columns of the tile are not used.
//
// ey_maxpool3x3s2: nn.MaxPool2d(3, 2, 1) on an NHWC map.  Unlike ey_maxpool2d, whose padding is an explicit nn.ZeroPad2d and therefore a ring
//   of ZEROS that take part in the maximum, this is torch's own padding: the cells outside the map are left out of the maximum, so the border
//   of an all-negative map stays negative.  Output size floor((H - 1) / 2) + 1; every window holds at least the cell (2 oy, 2 ox), which is
//   always inside the map.  The maximum is taken the way torch's CPU kernel takes it -- the window is walked row by row and a cell replaces the
//   running maximum only when it is greater or a NaN -- so the result equals F.max_pool2d(x, 3, 2, 1) bit for bit.
//
// ey_resnet_tail: the closing 1x1 of a bottleneck block, y = relu(W [t ; x|s] + b + res), f16 on the MFMA.  The residual is added BEFORE the
//   activation, which the `res` of ey_conv2d (added behind it) cannot express.  Identity block: one source t = cv2(cv1(x)), `res` is the block
//   input, added in fp32 before the ReLU, one f16 rounding.  Projection block: the second source is the block input read at pixel stride
//   s = 1 | 2 -- pixel (s oy, s ox) of x for output pixel (oy, ox) --, the weights are [W3 | Ws] concatenated along K, the bias is b3 + bs and
//   there is no `res`: the shortcut convolution's output never exists.  No LDS: A fragments (weights, row-major [Cout][K]) and B fragments
//   (pixels, NHWC) of the 16x16x32 MFMA both take 8 consecutive k per lane, so both come by 16-byte global loads; a wave owns 32 pixels x 64
//   channels, a workgroup 32 pixels x 256 channels (Cout = 4 C2 is a multiple of 256).
#include "common.h"
#include "tune.h"
#include "stem_ks.inc.h"

// one step of the window walk: a cell replaces the running maximum when it is greater or a NaN (torch: val > max || isnan(val))
__device__ __forceinline__ float mp_step(float v, float c) { return (c > v || c != c) ? c : v; }

// Memory-bound: one thread = one output pixel x 8 channels, nine range-checked 16-byte loads (a cell outside the map loads nothing and counts
// as -inf), work taken in XCD-contiguous order so that the rows two neighbouring outputs share come from one L2.
template <typename T>
__global__ __launch_bounds__(256) void maxpool3x3s2_kernel(int B, int H, int W, int C, int Ho, int Wo, int xcd, const T* __restrict__ x, int xCs, unsigned xBytes,
                                                           T* __restrict__ y, int yCs) {
  const int cv = C >> 3;
  const long idx = (long)(xcd ? ey_xcd_block(blockIdx.x, gridDim.x) : blockIdx.x) * 256 + threadIdx.x;
  if (idx >= (long)B * Ho * Wo * cv) return;
  const int c8 = (int)(idx % cv) * 8;
  const long m = idx / cv;
  const int ox = (int)(m % Wo);
  const long t = m / Wo;
  const int oy = (int)(t % Ho), b = (int)(t / Ho);
  const __amdgpu_buffer_rsrc_t rx = ey_rsrc(x, xBytes);
  Vec8<T> in[3][3];
  bool ok[3][3];
#pragma unroll
  for (int ky = 0; ky < 3; ++ky) {
    const int iy = 2 * oy - 1 + ky;
    const bool yok = iy >= 0 && iy < H;
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
      const int ix = 2 * ox - 1 + kx;
      ok[ky][kx] = yok && ix >= 0 && ix < W;
      const long e = (((long)b * H + iy) * W + ix) * xCs + c8;
      BufLoad8<T>::load(in[ky][kx], rx, ok[ky][kx] ? (unsigned)(e * (long)sizeof(T)) : EY_OOB);
    }
  }
  Vec8<T> o;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    float v = -INFINITY;
#pragma unroll
    for (int q = 0; q < 9; ++q) v = mp_step(v, ok[q / 3][q % 3] ? in[q / 3][q % 3].get(i) : -INFINITY);
    o.set(i, v);
  }
  o.store(y + m * yCs + c8);
}

template <typename T>
static int maxpool3x3s2_launch(int B, int H, int W, int C, int Ho, int Wo, const void* x, int xCs, void* y, int yCs, hipStream_t st) {
  const long total = (long)B * Ho * Wo * (C / 8);
  const long xbytes = (((long)B * H * W - 1) * xCs + C) * (long)sizeof(T);
  const long ybytes = (((long)B * Ho * Wo - 1) * yCs + C) * (long)sizeof(T);
  if (xbytes >= (1L << 31) || ybytes >= (1L << 31) || (total + 255) / 256 >= (1L << 31)) return ey_set_error(EY_EUNSUPPORTED, "maxpool3x3s2: view larger than 2 GiB");
  const dim3 grid((unsigned)((total + 255) / 256));
  const int xcd = (int)(tune().xcd_map & 1);
  hipLaunchKernelGGL(maxpool3x3s2_kernel<T>, grid, dim3(256), 0, st, B, H, W, C, Ho, Wo, xcd, (const T*)x, xCs, (unsigned)xbytes, (T*)y, yCs);
  EY_LAUNCH_CHECK("ey_maxpool3x3s2");
  return EY_OK;
}

extern "C" int ey_maxpool3x3s2(int dtype, int B, int H, int W, int C, const void* x, int x_cstride, void* y, int y_cstride, ey_stream_t stream) {
  EY_CHECK(x && y, "maxpool3x3s2: null pointer");
  EY_CHECK(dtype == EY_F16 || dtype == EY_F32, "maxpool3x3s2: bad dtype");
  EY_CHECK(B > 0 && H > 0 && W > 0, "maxpool3x3s2: bad extent B=%d H=%d W=%d", B, H, W);
  if (C <= 0 || C % 8) return ey_set_error(EY_EUNSUPPORTED, "maxpool3x3s2: C=%d (multiples of 8 are built)", C);
  const int es = dtype == EY_F16 ? 2 : 4;
  if (x_cstride < C || y_cstride < C || (x_cstride * es) % 16 || (y_cstride * es) % 16 || !ey_aligned(x, 16) || !ey_aligned(y, 16))
    return ey_set_error(EY_EUNSUPPORTED, "maxpool3x3s2: the views must be 16-byte aligned channel slots (cstride %d / %d, C=%d)", x_cstride, y_cstride, C);
  const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
  return dtype == EY_F16 ? maxpool3x3s2_launch<f16>(B, H, W, C, Ho, Wo, x, x_cstride, y, y_cstride, (hipStream_t)stream)
                         : maxpool3x3s2_launch<float>(B, H, W, C, Ho, Wo, x, x_cstride, y, y_cstride, (hipStream_t)stream);
}

// ============================================================================ layer 0 as one launch: conv 7x7 / 2 / 3 -> LDS tile -> max-pool 3x3 / 2 / 1
#define RS_T 3   // pooled rows of a tile: conv rows 2 T ty - 1 ... 2 T ty + 2 T - 1 (7 of the 8 of the conv tile)
#define RS_U 30  // pooled columns of a tile: the conv tile starts at column 2 U tx - 4, the window at 2 U tx - 1
#define RS_C 64  // channels

// pool a conv tile [SK_TR][SK_TC][RS_C] in LDS (cells outside the map hold -inf): one work item = one pooled pixel x 8 channels
template <typename T>
__device__ __forceinline__ void rs_pool(const T* tile, int b, int py0, int px0, int Hp, int Wp, T* __restrict__ y, int yCs, int tid) {
  for (int it = tid; it < RS_T * RS_U * (RS_C / 8); it += 256) {
    const int c8 = (it % (RS_C / 8)) * 8, pp = it / (RS_C / 8), px = pp % RS_U, py = pp / RS_U;
    if (py0 + py >= Hp || px0 + px >= Wp) continue;
    Vec8<T> in[9];
#pragma unroll
    for (int q = 0; q < 9; ++q) in[q].load(tile + ((2 * py + q / 3) * SK_TC + 2 * px + 3 + q % 3) * RS_C + c8);
    Vec8<T> o;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      float v = -INFINITY;
#pragma unroll
      for (int q = 0; q < 9; ++q) v = mp_step(v, in[q].get(i));
      o.set(i, v);
    }
    o.store(y + (((long)b * Hp + py0 + py) * Wp + px0 + px) * yCs + c8);
  }
}

__global__ __launch_bounds__(256) void resnet_stem_mfma_kernel(int B, int H, int W, int Ho, int Wo, int Hp, int Wp, int act, const f16* __restrict__ x, unsigned xbytes,
                                                               const float* __restrict__ w, const float* __restrict__ bias, f16* __restrict__ y, int yCs) {
  constexpr int K = 7, S = 2, P = 3, NT = RS_C / 16;
  using G = SkGeo<K, S, P>;
  constexpr int HR = G::HR, LW = G::LW, KC = G::KC;
  extern __shared__ __attribute__((aligned(16))) unsigned char rs_lds[];
  f16* s_in = reinterpret_cast<f16*>(rs_lds);                      // 3 HR LW halves = 19 152 bytes (a multiple of 16)
  f16* tile = reinterpret_cast<f16*>(rs_lds) + 3 * HR * LW;        // [8][64][64] halves
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, g = lane >> 4;
  const int tilesX = (Wp + RS_U - 1) / RS_U, tilesY = (Hp + RS_T - 1) / RS_T;
  const int b = blockIdx.x / (tilesX * tilesY), trem = blockIdx.x - b * (tilesX * tilesY);
  const int ty = trem / tilesX, tx = trem - ty * tilesX;
  const int oy0 = 2 * RS_T * ty - 1, ox0 = 2 * RS_U * tx - 4;  // (S ox0 is a multiple of 8)
  sk_stage<K, S, P>(s_in, ey_rsrc(x, xbytes), b, H, W, oy0, ox0, tid);
  Vec8<f16> af[NT][KC];
  int off[KC][8];
  float bs[NT][4];
  sk_frags<NT, K, S, P>(w, bias, r, g, af, off, bs);
  __syncthreads();
  const f16 ninf = (f16)(-INFINITY);
#pragma unroll 1
  for (int blk = 0; blk < 8; ++blk) {
    const int rr = 2 * wave + (blk >> 2), j = (blk & 3) * 16 + r;
    f32x4 acc[NT];
    sk_px16<NT, K, S, P>(s_in + (S * rr) * LW + S * j + (8 - P), off, af, acc);
    const int oy = oy0 + rr, ox = ox0 + j;
    const bool in = oy >= 0 && oy < Ho && ox >= 0 && ox < Wo;
    f16* tp = tile + (rr * SK_TC + j) * RS_C + 4 * g;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const f16x4 o = sk_out(acc[nt], bs[nt], act);
      const f16x4 m = {ninf, ninf, ninf, ninf};
      *reinterpret_cast<f16x4*>(tp + nt * 16) = in ? o : m;
    }
  }
  __syncthreads();
  rs_pool<f16>(tile, b, RS_T * ty, RS_U * tx, Hp, Wp, y, yCs, tid);
}

template <typename T>
__global__ __launch_bounds__(256) void resnet_stem_kernel(int B, int Cin, int H, int W, int Ho, int Wo, int Hp, int Wp, int act, const T* __restrict__ x, unsigned xbytes,
                                                          const float* __restrict__ w, const float* __restrict__ bias, T* __restrict__ y, int yCs) {
  extern __shared__ __attribute__((aligned(16))) unsigned char rs_lds[];
  T* tile = reinterpret_cast<T*>(rs_lds);  // [8][64][64]
  const int tid = threadIdx.x;
  const int tilesX = (Wp + RS_U - 1) / RS_U, tilesY = (Hp + RS_T - 1) / RS_T;
  const int b = blockIdx.x / (tilesX * tilesY), trem = blockIdx.x - b * (tilesX * tilesY);
  const int ty = trem / tilesX, tx = trem - ty * tilesX;
  const int oy0 = 2 * RS_T * ty - 1, ox0 = 2 * RS_U * tx - 4;
  const __amdgpu_buffer_rsrc_t rs = ey_rsrc(x, xbytes);
  // one work item = one conv pixel of rows 0 ... 2 T of the tile x 16 channels (pixels fastest: the 16 weights stay wave-uniform)
#pragma unroll 1
  for (int it = tid; it < (2 * RS_T + 1) * SK_TC * (RS_C / 16); it += 256) {
    const int pix = it % ((2 * RS_T + 1) * SK_TC), co0 = (it / ((2 * RS_T + 1) * SK_TC)) * 16;
    const int rr = pix / SK_TC, j = pix - rr * SK_TC, oy = oy0 + rr, ox = ox0 + j;
    const bool in = oy >= 0 && oy < Ho && ox >= 0 && ox < Wo;
    float acc[16];
    if (in) sk_valu_px<T, 7, 2, 3>(rs, b, Cin, H, W, oy, ox, co0, w, bias, act, acc);
    else {
#pragma unroll
      for (int o = 0; o < 16; ++o) acc[o] = -INFINITY;
    }
    T* tp = tile + (rr * SK_TC + j) * RS_C + co0;
    Vec8<T> v;
#pragma unroll
    for (int o = 0; o < 8; ++o) v.set(o, acc[o]);
    v.store(tp);
#pragma unroll
    for (int o = 0; o < 8; ++o) v.set(o, acc[8 + o]);
    v.store(tp + 8);
  }
  __syncthreads();
  rs_pool<T>(tile, b, RS_T * ty, RS_U * tx, Hp, Wp, y, yCs, tid);
}

static int g_resnet_stem_variant = 0;  // form of the last launch, 1: MFMA, 0: VALU (process-wide, not synchronised: developer tools and tests)
extern "C" int ey_resnet_stem_last_variant(void) { return g_resnet_stem_variant; }

template <typename KernelT>
static bool rs_raise_lds(KernelT kernel, size_t lds) {
  return lds <= 64 * 1024 || hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) == hipSuccess;
}

extern "C" int ey_resnet_stem(int x_dtype, int y_dtype, int B, int Cin, int H, int W, int Cout, int act, const void* x, const float* w, const float* bias, void* y,
                              int y_cstride, ey_stream_t stream) {
  EY_CHECK(x && w && y, "resnet_stem: null pointer");
  EY_CHECK((x_dtype == EY_F16 || x_dtype == EY_F32) && (y_dtype == EY_F16 || y_dtype == EY_F32), "resnet_stem: bad dtype");
  EY_CHECK(B > 0 && H > 0 && W > 0, "resnet_stem: bad extent B=%d H=%d W=%d", B, H, W);
  if (x_dtype != y_dtype) return ey_set_error(EY_EUNSUPPORTED, "resnet_stem: image and output of one type are built (f16 -> f16, fp32 -> fp32)");
  if (Cout != RS_C || Cin < 1 || Cin > 4) return ey_set_error(EY_EUNSUPPORTED, "resnet_stem: Cin=%d Cout=%d (Cin 1..4 and 64 output channels are built)", Cin, Cout);
  const int es = y_dtype == EY_F16 ? 2 : 4;
  if (y_cstride < Cout || (y_cstride * es) % 16 || !ey_aligned(y, 16) || !ey_aligned(x, es))
    return ey_set_error(EY_EUNSUPPORTED, "resnet_stem: the output must be a 16-byte aligned channel slot, the image aligned to its element size");
  const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1, Hp = (Ho - 1) / 2 + 1, Wp = (Wo - 1) / 2 + 1;
  const long tiles = (long)B * ((Hp + RS_T - 1) / RS_T) * ((Wp + RS_U - 1) / RS_U);
  const long xbytes = (long)B * Cin * H * W * es;
  if (tiles >= (1L << 31) || xbytes >= (1L << 31)) return ey_set_error(EY_EUNSUPPORTED, "resnet_stem: input batch larger than 2 GiB");
  hipStream_t st = (hipStream_t)stream;
  const size_t tile_bytes = (size_t)SK_TR * SK_TC * RS_C * es;
  if (x_dtype == EY_F16 && Cin == 3 && W % 8 == 0 && ey_aligned(x, 16) && tune().stem_mfma) {  // (the condition under which ey_stem_conv_ks takes its MFMA form)
    using G = SkGeo<7, 2, 3>;
    const size_t lds = (size_t)3 * G::HR * G::LW * 2 + tile_bytes;
    if (!rs_raise_lds(resnet_stem_mfma_kernel, lds)) return ey_set_error(EY_EUNSUPPORTED, "resnet_stem: %zu bytes of LDS refused by the runtime", lds);
    hipLaunchKernelGGL(resnet_stem_mfma_kernel, dim3((unsigned)tiles), dim3(256), lds, st, B, H, W, Ho, Wo, Hp, Wp, act, (const f16*)x, (unsigned)xbytes, w, bias, (f16*)y, y_cstride);
    g_resnet_stem_variant = 1;
  } else if (x_dtype == EY_F16) {
    if (!rs_raise_lds(resnet_stem_kernel<f16>, tile_bytes)) return ey_set_error(EY_EUNSUPPORTED, "resnet_stem: %zu bytes of LDS refused by the runtime", tile_bytes);
    hipLaunchKernelGGL(resnet_stem_kernel<f16>, dim3((unsigned)tiles), dim3(256), tile_bytes, st, B, Cin, H, W, Ho, Wo, Hp, Wp, act, (const f16*)x, (unsigned)xbytes, w, bias, (f16*)y, y_cstride);
    g_resnet_stem_variant = 0;
  } else {
    if (!rs_raise_lds(resnet_stem_kernel<float>, tile_bytes)) return ey_set_error(EY_EUNSUPPORTED, "resnet_stem: %zu bytes of LDS refused by the runtime", tile_bytes);
    hipLaunchKernelGGL(resnet_stem_kernel<float>, dim3((unsigned)tiles), dim3(256), tile_bytes, st, B, Cin, H, W, Ho, Wo, Hp, Wp, act, (const float*)x, (unsigned)xbytes, w, bias, (float*)y, y_cstride);
    g_resnet_stem_variant = 0;
  }
  EY_LAUNCH_CHECK("ey_resnet_stem");
  return EY_OK;
}

// ============================================================================ block tail: relu(W [t ; x|s] + b + res)
#define RT_MT 2  // 16-pixel blocks per wave
#define RT_NT 4  // 16-channel blocks per wave
__global__ __launch_bounds__(256) void resnet_tail_kernel(int M, int HoWo, int Wo, int H, int W, int s, int C2, int C1, const f16* __restrict__ t, int tCs,
                                                          const f16* __restrict__ x, int xCs, const f16* __restrict__ w, const float* __restrict__ bias,
                                                          const f16* __restrict__ res, int resCs, f16* __restrict__ y, int yCs) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
  const int m0 = blockIdx.x * (16 * RT_MT), n0 = blockIdx.y * (64 * RT_NT) + wave * (16 * RT_NT);
  const int K = C2 + C1;
  const f16* tp[RT_MT];
  const f16* xp[RT_MT];
#pragma unroll
  for (int mt = 0; mt < RT_MT; ++mt) {
    const int m = min(m0 + mt * 16 + r, M - 1);  // (rows past the map repeat the last pixel; they are not stored)
    tp[mt] = t + (long)m * tCs + 8 * g;
    const int b = m / HoWo, rem = m - b * HoWo, oy = rem / Wo, ox = rem - oy * Wo;
    xp[mt] = C1 ? x + (((long)b * H + s * oy) * W + s * ox) * xCs + 8 * g : nullptr;
  }
  const f16* wp[RT_NT];
#pragma unroll
  for (int nt = 0; nt < RT_NT; ++nt) wp[nt] = w + (long)(n0 + nt * 16 + r) * K + 8 * g;
  f32x4 acc[RT_MT][RT_NT];
#pragma unroll
  for (int mt = 0; mt < RT_MT; ++mt)
#pragma unroll
    for (int nt = 0; nt < RT_NT; ++nt) acc[mt][nt] = (f32x4)0.f;
  for (int k = 0; k < C2; k += 32) {
    f16x8 a[RT_NT], bq[RT_MT];
#pragma unroll
    for (int nt = 0; nt < RT_NT; ++nt) a[nt] = *reinterpret_cast<const f16x8*>(wp[nt] + k);
#pragma unroll
    for (int mt = 0; mt < RT_MT; ++mt) bq[mt] = *reinterpret_cast<const f16x8*>(tp[mt] + k);
#pragma unroll
    for (int mt = 0; mt < RT_MT; ++mt)
#pragma unroll
      for (int nt = 0; nt < RT_NT; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[nt], bq[mt], acc[mt][nt], 0, 0, 0);
  }
  for (int k = 0; k < C1; k += 32) {
    f16x8 a[RT_NT], bq[RT_MT];
#pragma unroll
    for (int nt = 0; nt < RT_NT; ++nt) a[nt] = *reinterpret_cast<const f16x8*>(wp[nt] + C2 + k);
#pragma unroll
    for (int mt = 0; mt < RT_MT; ++mt) bq[mt] = *reinterpret_cast<const f16x8*>(xp[mt] + k);
#pragma unroll
    for (int mt = 0; mt < RT_MT; ++mt)
#pragma unroll
      for (int nt = 0; nt < RT_NT; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[nt], bq[mt], acc[mt][nt], 0, 0, 0);
  }
  // lane (r, g) holds channels n0 + 16 nt + 4 g + j of pixel m0 + 16 mt + r
#pragma unroll
  for (int mt = 0; mt < RT_MT; ++mt) {
    const int m = m0 + mt * 16 + r;
    if (m >= M) continue;
#pragma unroll
    for (int nt = 0; nt < RT_NT; ++nt) {
      const int ch = n0 + nt * 16 + 4 * g;
      const f32x4 bv = *reinterpret_cast<const f32x4*>(bias + ch);
      float v[4] = {acc[mt][nt][0] + bv[0], acc[mt][nt][1] + bv[1], acc[mt][nt][2] + bv[2], acc[mt][nt][3] + bv[3]};
      if (res) {
        const f16x4 rv = *reinterpret_cast<const f16x4*>(res + (long)m * resCs + ch);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] += (float)rv[j];
      }
      const f16x4 o = {(f16)fmaxf(v[0], 0.f), (f16)fmaxf(v[1], 0.f), (f16)fmaxf(v[2], 0.f), (f16)fmaxf(v[3], 0.f)};
      *reinterpret_cast<f16x4*>(y + (long)m * yCs + ch) = o;
    }
  }
}

extern "C" int ey_resnet_tail(int dtype, int B, int H, int W, int stride, int C1, int C2, const void* t, int t_cstride, const void* x, int x_cstride, const void* w,
                              const float* bias, const void* res, int res_cstride, void* y, int y_cstride, ey_stream_t stream) {
  EY_CHECK(t && w && bias && y, "resnet_tail: null pointer");
  EY_CHECK(B > 0 && H > 0 && W > 0, "resnet_tail: bad extent B=%d H=%d W=%d", B, H, W);
  if (dtype != EY_F16) return ey_set_error(EY_EUNSUPPORTED, "resnet_tail: f16 is built (fp32 takes the composed form)");
  if (C2 != 64 && C2 != 128 && C2 != 256 && C2 != 512) return ey_set_error(EY_EUNSUPPORTED, "resnet_tail: C2=%d (64, 128, 256 and 512 are built)", C2);
  if (C1 < 0 || C1 % 32 || C1 > 2048) return ey_set_error(EY_EUNSUPPORTED, "resnet_tail: C1=%d (0 = identity block, else multiples of 32 up to 2048)", C1);
  if (stride != 1 && stride != 2) return ey_set_error(EY_EUNSUPPORTED, "resnet_tail: stride %d (1 and 2 are built)", stride);
  if (C1 == 0 && (stride != 1 || !res || x)) return ey_set_error(EY_EUNSUPPORTED, "resnet_tail: an identity block has stride 1, a residual and no second source");
  if (C1 > 0 && (!x || res)) return ey_set_error(EY_EUNSUPPORTED, "resnet_tail: a projection block has a second source and no residual");
  const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1, Cout = 4 * C2;
  const long M = (long)B * Ho * Wo;
  if (t_cstride < C2 || (t_cstride * 2) % 16 || !ey_aligned(t, 16) || (C1 && (x_cstride < C1 || (x_cstride * 2) % 16 || !ey_aligned(x, 16))) || !ey_aligned(w, 16) ||
      !ey_aligned(bias, 16) || y_cstride < Cout || (y_cstride * 2) % 8 || !ey_aligned(y, 8) || (res && (res_cstride < Cout || (res_cstride * 2) % 8 || !ey_aligned(res, 8))))
    return ey_set_error(EY_EUNSUPPORTED, "resnet_tail: sources must be 16-byte, output and residual 8-byte aligned channel slots");
  if (M >= (1L << 31) || (M + 31) / 32 >= (1L << 31)) return ey_set_error(EY_EUNSUPPORTED, "resnet_tail: map too large");
  const dim3 grid((unsigned)((M + 16 * RT_MT - 1) / (16 * RT_MT)), Cout / (64 * RT_NT));
  hipLaunchKernelGGL(resnet_tail_kernel, grid, dim3(256), 0, (hipStream_t)stream, (int)M, Ho * Wo, Wo, H, W, stride, C2, C1, (const f16*)t, t_cstride, (const f16*)x, x_cstride,
                     (const f16*)w, bias, (const f16*)res, res_cstride, (f16*)y, y_cstride);
  EY_LAUNCH_CHECK("ey_resnet_tail");
  return EY_OK;
}
