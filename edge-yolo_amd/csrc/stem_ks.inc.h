// Per-pixel arithmetic of the image stems (ey_stem_conv_ks, classic.hip), shared with the single-launch ResNet stem (ey_resnet_stem, resnet.hip):
// the same device functions in the same k order, so a convolution output is the same bits wherever it is computed.
#pragma once
#include "common.h"

#define SK_TR 8
#define SK_TC 64
template <int K, int S, int P>
struct SkGeo {
  static constexpr int HR = S * (SK_TR - 1) + K;                    // staged input rows of a tile: 2 TR + 4 at (6, 2, 2)
  static constexpr int NVC = (8 - P + S * (SK_TC - 1) + K + 7) / 8;  // staged 8-column vectors of a row; the first starts at S ox0 - 8
  static constexpr int LW = NVC * 8 + 8;                              // LDS row stride (elements)
  static constexpr int KK = 3 * K * K;                                // GEMM K: 108 / 27 / 147
  static constexpr int KC = (KK + 31) / 32;                           // 16x16x32 MFMAs per 16 pixels x 16 channels: 4 / 1 / 5 (147 zero-filled to 160)
};

// ---- MFMA form.  Stage the 3 x HR x (8 NVC) input patch of the 8 x 64 output tile at (oy0, ox0) -- S ox0 a multiple of 8 -- into LDS with
// range-checked 16-byte loads of the planar image (out of range = the zero padding; W % 8 == 0: a vector is entirely inside or outside).
template <int K, int S, int P>
__device__ __forceinline__ void sk_stage(f16* s_in, __amdgpu_buffer_rsrc_t rs, int b, int H, int W, int oy0, int ox0, int tid) {
  using G = SkGeo<K, S, P>;
  constexpr int HR = G::HR, NVC = G::NVC, LW = G::LW, NV = 3 * HR * NVC;
  const int iy0 = S * oy0 - P, ixa = S * ox0 - 8;  // first staged input row / (8-aligned) column
#pragma unroll
  for (int u = 0; u < (NV + 255) / 256; ++u) {
    const int v = tid + u * 256;
    if (v < NV) {
      const int c = v / (HR * NVC), rem = v - c * (HR * NVC), row = rem / NVC, vc = rem - row * NVC;
      const int iy = iy0 + row, ix = ixa + 8 * vc;
      const bool ok = iy >= 0 && iy < H && ix >= 0 && ix < W;
      Vec8<f16> t;
      BufLoad8<f16>::load(t, rs, ok ? (unsigned)(((((long)b * 3 + c) * H + iy) * W + ix) * 2) : EY_OOB);
      t.store(s_in + (c * HR + row) * LW + 8 * vc);
    }
  }
}

// A fragments (weights, fp32 OIHW -> f16), this lane's tap offsets (k = 32 kc + 8 g + t = c K K + ky K + kx) and its biases
template <int NT, int K, int S, int P>
__device__ __forceinline__ void sk_frags(const float* __restrict__ w, const float* __restrict__ bias, int r, int g, Vec8<f16> (&af)[NT][SkGeo<K, S, P>::KC],
                                         int (&off)[SkGeo<K, S, P>::KC][8], float (&bs)[NT][4]) {
  using G = SkGeo<K, S, P>;
  constexpr int HR = G::HR, LW = G::LW, KK = G::KK, KC = G::KC;
#pragma unroll
  for (int kc = 0; kc < KC; ++kc)
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      const int k = 32 * kc + 8 * g + t, c = k / (K * K), ky = (k - K * K * c) / K, kx = k - K * K * c - K * ky;
      off[kc][t] = k < KK ? (c * HR + ky) * LW + kx : -1;
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) af[nt][kc].v[t] = k < KK ? (f16)w[(nt * 16 + r) * KK + k] : (f16)0.f;
    }
#pragma unroll
  for (int nt = 0; nt < NT; ++nt)
#pragma unroll
    for (int j = 0; j < 4; ++j) bs[nt][j] = bias ? bias[nt * 16 + 4 * g + j] : 0.f;
}

// 16 pixels x 16 NT channels: bp = this lane's pixel in the staged patch (s_in + (S rr) LW + S j + (8 - P))
template <int NT, int K, int S, int P>
__device__ __forceinline__ void sk_px16(const f16* bp, const int (&off)[SkGeo<K, S, P>::KC][8], const Vec8<f16> (&af)[NT][SkGeo<K, S, P>::KC], f32x4 (&acc)[NT]) {
  constexpr int KC = SkGeo<K, S, P>::KC;
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) acc[nt] = (f32x4)0.f;
#pragma unroll
  for (int kc = 0; kc < KC; ++kc) {
    Vec8<f16> bq;
    if constexpr (K % 2 == 0 && S % 2 == 0 && P % 2 == 0) {
      // an even window at an even stride: the taps (kx, kx + 1) of an even kx are neighbours in k and in LDS, and every offset is even --
      // four 4-byte reads instead of eight 2-byte reads and their packing
      ey_u32x4 u;
#pragma unroll
      for (int t = 0; t < 4; ++t) u[t] = off[kc][2 * t] >= 0 ? *reinterpret_cast<const unsigned*>(bp + off[kc][2 * t]) : 0u;
      bq.v = __builtin_bit_cast(f16x8, u);
    } else {
#pragma unroll
      for (int t = 0; t < 8; ++t) bq.v[t] = off[kc][t] >= 0 ? bp[off[kc][t]] : (f16)0.f;
    }
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[nt][kc].v, bq.v, acc[nt], 0, 0, 0);
  }
}

// bias, activation in fp32, one rounding to f16: the four channels 16 nt + 4 g + j of this lane's pixel
__device__ __forceinline__ f16x4 sk_out(const f32x4& a, const float (&bs)[4], int act) {
  float v4[4] = {a[0] + bs[0], a[1] + bs[1], a[2] + bs[2], a[3] + bs[3]};
  ey_act_n(v4, act);
  const f16x4 o = {(f16)v4[0], (f16)v4[1], (f16)v4[2], (f16)v4[3]};
  return o;
}

// ---- VALU form (fp32, Cin 1..4, any width): one output pixel x 16 output channels; the K x K window of one input channel at a time comes by
// range-checked buffer loads (the zero padding and the right / bottom edges need no branches), the weights are wave-uniform.
template <typename TI> struct SkLoad;
template <> struct SkLoad<f16> {
  static __device__ __forceinline__ float at(__amdgpu_buffer_rsrc_t r, long e, bool ok) {
    const unsigned short s = __builtin_amdgcn_raw_buffer_load_b16(r, ok ? (unsigned)(e * 2) : EY_OOB, 0, 0);
    return (float)__builtin_bit_cast(f16, s);
  }
};
template <> struct SkLoad<float> {
  static __device__ __forceinline__ float at(__amdgpu_buffer_rsrc_t r, long e, bool ok) {
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, ok ? (unsigned)(e * 4) : EY_OOB, 0, 0));
  }
};

// acc[o] = act(bias[co0 + o] + sum_c sum_ky sum_kx x w) for output pixel (b, oy, ox), o = 0 ... 15
template <typename TI, int K, int S, int P>
__device__ __forceinline__ void sk_valu_px(__amdgpu_buffer_rsrc_t rs, int b, int Cin, int H, int W, int oy, int ox, int co0, const float* __restrict__ w,
                                           const float* __restrict__ bias, int act, float (&acc)[16]) {
#pragma unroll
  for (int o = 0; o < 16; ++o) acc[o] = bias ? bias[co0 + o] : 0.f;
  for (int c = 0; c < Cin; ++c) {
    float in[K][K];
#pragma unroll
    for (int ky = 0; ky < K; ++ky) {
      const int iy = oy * S - P + ky;
      const bool rowok = iy >= 0 && iy < H;
      const long rowbase = (((long)b * Cin + c) * H + iy) * W;
#pragma unroll
      for (int kx = 0; kx < K; ++kx) {
        const int ix = ox * S - P + kx;
        in[ky][kx] = SkLoad<TI>::at(rs, rowbase + ix, rowok && ix >= 0 && ix < W);
      }
    }
#pragma unroll
    for (int o = 0; o < 16; ++o) {
      const float* wo = w + ((long)(co0 + o) * Cin + c) * (K * K);
#pragma unroll
      for (int ky = 0; ky < K; ++ky)
#pragma unroll
        for (int kx = 0; kx < K; ++kx) acc[o] = __builtin_fmaf(in[ky][kx], wo[ky * K + kx], acc[o]);
    }
  }
  ey_act_n(acc, act);
}
