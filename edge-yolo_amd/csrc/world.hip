// Max-sigmoid attention of YOLO-World's C2fAttn (reference ultralytics/nn/modules/block.py:558-576, after the `gl` linear and the
// proj_conv).  Per image b, pixel p and head m (channels m*32 .. m*32+31):
//   aw = sigmoid( max_n( E[b,p,m,:] . G[bg,n,m,:] ) / sqrt(32) + bias[m] ) * scale[m],     Y[b,p,m,:] = P[b,p,m,:] * aw
// A pixels x texts GEMM with K = 32 whose rows are reduced by a maximum: the score matrix never leaves the registers.
//
// f16: a wave owns 16 pixels of ONE image (tiles never straddle images, so per-image guides need no second operand).  Per head, one
// mfma_f32_16x16x32_f16 per tile of 16 texts covers the head's whole K: A = texts (row = text), B = pixels (column = pixel), so lane
// (col, kq) ends with 4 text scores of pixel `col`; the running maximum goes over the registers and the text tiles, two xor-shuffles
// finish it across kq, and the division / bias / sigmoid / scale tail runs once per pixel and head.  The same lane then owns channels
// m*32 + 8kq .. +7 of its pixel: one 16-byte load of P and one 16-byte store of Y.
// Padded text rows (a tile past n) load text n-1 again: a duplicate of a real score cannot change the maximum, whereas a zero row would
// win whenever every real score is negative.  The same holds for the whole tiles the two-tile unroll may add.
// fp32: one thread per (pixel, head), a 32-step fmaf chain per text (fp32 products and sums), the same tail.
// No atomics, no workspace, fixed evaluation order: the output is the same from run to run, and the launch is graph-capturable.
#include "common.h"

#define MSA_HC 32
#define MSA_PIX 64  // pixels per workgroup: 4 waves x one 16-pixel MFMA tile

__device__ __forceinline__ float msa_gate(float mx, float bias, float scale) {
  // aw / hc**0.5 + bias, sigmoid, * scale: the reference's operations in its order; sqrt(32) rounded to fp32 as torch's scalar is
  return ey_sigmoid(mx / 5.656854249492381f + bias) * scale;
}

// e, p, y: [B][HW][*Cs] windows; g: [Bg][n][C]; gstride = n * C (Bg == B) or 0 (one vocabulary).  grid (tiles of an image, B).
__global__ __launch_bounds__(256) void msa_f16_kernel(int HW, int nh, int n, const f16* __restrict__ e, int eCs, const f16* __restrict__ p, int pCs,
                                                      const f16* __restrict__ g, long gstride, const float* __restrict__ bias,
                                                      const float* __restrict__ scale, f16* __restrict__ y, int yCs) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = lane & 15, kq = lane >> 4;
  const int b = blockIdx.y;
  const int pix = blockIdx.x * MSA_PIX + wave * 16 + col;
  if (blockIdx.x * MSA_PIX + wave * 16 >= HW) return;  // (whole wave past the image: no barrier below)
  const bool live = pix < HW;
  const long row = (long)b * HW + (live ? pix : HW - 1);  // tile tail: a valid address, the result is never stored
  const int C = nh * MSA_HC;
  const f16* ep = e + row * eCs + kq * 8;
  const f16* pp = p + row * pCs + kq * 8;
  f16* yp = y + row * yCs + kq * 8;
  const f16* gb = g + (long)b * gstride + kq * 8;
  const int ntile = (n + 15) >> 4;
  for (int m = 0; m < nh; ++m) {
    Vec8<f16> px, pv;
    px.load(ep + m * MSA_HC);
    pv.load(pp + m * MSA_HC);
    float mx = -INFINITY;
    for (int t = 0; t < ntile; t += 2) {
      const int r0 = min(t * 16 + col, n - 1), r1 = min(t * 16 + 16 + col, n - 1);
      Vec8<f16> a0, a1;
      a0.load(gb + (long)r0 * C + m * MSA_HC);
      a1.load(gb + (long)r1 * C + m * MSA_HC);
      const f32x4 s0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(a0.v, px.v, (f32x4)0.f, 0, 0, 0);
      const f32x4 s1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(a1.v, px.v, (f32x4)0.f, 0, 0, 0);
      mx = fmaxf(mx, fmaxf(fmaxf(fmaxf(s0[0], s0[1]), fmaxf(s0[2], s0[3])), fmaxf(fmaxf(s1[0], s1[1]), fmaxf(s1[2], s1[3]))));
    }
    mx = fmaxf(mx, __shfl_xor(mx, 16));
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    const float aw = msa_gate(mx, bias[m], scale ? scale[m] : 1.f);
    if (live) {
      Vec8<f16> o;
#pragma unroll
      for (int i = 0; i < 8; ++i) o.set(i, pv.get(i) * aw);
      o.store(yp + m * MSA_HC);
    }
  }
}

// grid (pixel blocks of an image, nh, B): one thread per pixel, the head is block-uniform (the guide rows are scalar-broadcast loads)
__global__ __launch_bounds__(256) void msa_f32_kernel(int HW, int nh, int n, const float* __restrict__ e, int eCs, const float* __restrict__ p, int pCs,
                                                      const float* __restrict__ g, long gstride, const float* __restrict__ bias,
                                                      const float* __restrict__ scale, float* __restrict__ y, int yCs) {
  const int pix = blockIdx.x * 256 + threadIdx.x, m = blockIdx.y, b = blockIdx.z;
  if (pix >= HW) return;
  const long row = (long)b * HW + pix;
  const int C = nh * MSA_HC;
  const float* ep = e + row * eCs + m * MSA_HC;
  Vec8<float> x[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) x[q].load(ep + q * 8);
  const float* gp = g + (long)b * gstride + m * MSA_HC;
  float mx = -INFINITY;
  for (int t = 0; t < n; ++t, gp += C) {
    float s = 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      Vec8<float> w;
      w.load(gp + q * 8);
#pragma unroll
      for (int i = 0; i < 8; ++i) s = __builtin_fmaf(x[q].get(i), w.get(i), s);
    }
    mx = fmaxf(mx, s);
  }
  const float aw = msa_gate(mx, bias[m], scale ? scale[m] : 1.f);
  const float* pp = p + row * pCs + m * MSA_HC;
  float* yp = y + row * yCs + m * MSA_HC;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    Vec8<float> v, o;
    v.load(pp + q * 8);
#pragma unroll
    for (int i = 0; i < 8; ++i) o.set(i, v.get(i) * aw);
    o.store(yp + q * 8);
  }
}

extern "C" int ey_max_sigmoid_attn(int dtype, int B, int HW, int nh, int hc, int C, int n, int Bg, const void* e, int e_cstride, const void* p,
                                   int p_cstride, const void* g, const float* bias, const float* scale, void* y, int y_cstride, ey_stream_t stream) {
  EY_CHECK(e && p && g && bias && y, "max_sigmoid_attn: null pointer");
  EY_CHECK(dtype == EY_F16 || dtype == EY_F32, "max_sigmoid_attn: bad dtype");
  EY_CHECK(B > 0 && HW > 0 && nh > 0 && n > 0, "max_sigmoid_attn: B=%d HW=%d nh=%d n=%d", B, HW, nh, n);
  EY_CHECK(Bg == 1 || Bg == B, "max_sigmoid_attn: Bg=%d (1, or B=%d for per-image guides)", Bg, B);
  if (hc != MSA_HC) return ey_set_error(EY_EUNSUPPORTED, "max_sigmoid_attn: hc=%d (head width 32 is built)", hc);
  if (C != nh * MSA_HC) return ey_set_error(EY_EUNSUPPORTED, "max_sigmoid_attn: C=%d is not 32 * nh (nh=%d)", C, nh);
  if (n > EY_MSA_MAX_TEXTS) return ey_set_error(EY_EUNSUPPORTED, "max_sigmoid_attn: n=%d texts (at most %d)", n, EY_MSA_MAX_TEXTS);
  EY_CHECK(e_cstride >= C && p_cstride >= C && y_cstride >= C, "max_sigmoid_attn: a pixel stride is below C=%d", C);
  const size_t es = dtype == EY_F16 ? 2 : 4;
  if (!ey_aligned(e, 16) || !ey_aligned(p, 16) || !ey_aligned(y, 16) || !ey_aligned(g, 16) || ((size_t)e_cstride * es) % 16 ||
      ((size_t)p_cstride * es) % 16 || ((size_t)y_cstride * es) % 16)
    return ey_set_error(EY_EUNSUPPORTED, "max_sigmoid_attn: e, p, y and g must be 16-byte aligned (pixel strides multiples of 16 bytes)");
  const long npix = (long)B * HW;
  const long cs = e_cstride > p_cstride ? (e_cstride > y_cstride ? e_cstride : y_cstride) : (p_cstride > y_cstride ? p_cstride : y_cstride);
  if (npix * cs * (long)es >= (1L << 31) || B > 65535 || nh > 65535)
    return ey_set_error(EY_EUNSUPPORTED, "max_sigmoid_attn: tensor too large (B=%d HW=%d pixel stride %ld)", B, HW, cs);
  const long gstride = Bg == 1 ? 0 : (long)n * C;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == EY_F16)
    hipLaunchKernelGGL(msa_f16_kernel, dim3((unsigned)ey_cdiv(HW, MSA_PIX), (unsigned)B), dim3(256), 0, st, HW, nh, n, (const f16*)e, e_cstride,
                       (const f16*)p, p_cstride, (const f16*)g, gstride, bias, scale, (f16*)y, y_cstride);
  else
    hipLaunchKernelGGL(msa_f32_kernel, dim3((unsigned)ey_cdiv(HW, 256), (unsigned)nh, (unsigned)B), dim3(256), 0, st, HW, nh, n, (const float*)e,
                       e_cstride, (const float*)p, p_cstride, (const float*)g, gstride, bias, scale, (float*)y, y_cstride);
  EY_LAUNCH_CHECK("ey_max_sigmoid_attn");
  return EY_OK;
}
