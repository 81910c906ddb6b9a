// DySample (reference ultralytics/nn/modules/dysample.py): content-aware x2 upsampling.  A 1x1 conv predicts, per input pixel, 2*G*4
// sampling offsets (G channel groups x the 4 output pixels of the 2x2 cell x (x, y)); every output pixel of a group is the bilinear
// sample of the group's channels at (w + O_x, h + O_y), clamped to the map (grid_sample, align_corners=False, padding_mode="border",
// written in pixel coordinates).  One launch: phase 1 runs the skinny GEMM [pixels x C] . [C x 8G] of a 64-pixel tile on MFMA (a second
// one + sigmoid for the `dyscope` form) and leaves the offsets in LDS; phase 2 gathers.  Offsets and coordinates are fp32 in both
// storage types (a deliberate departure from the reference's f16 pass, which rounds its normalised grid to f16: in [0.5, 1) that grid has
// steps of 2^-11, i.e. W/4096 px -- 0.04 px on a 160-pixel side).  No atomics, fixed summation order: the output is the same run to run.
#include "common.h"

#define DYS_PIX 64  // input pixels per workgroup: 4 waves x one 16-pixel MFMA tile

__device__ __forceinline__ f32x4 dys_mma(const Vec8<f16>& a, const Vec8<f16>& b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(a.v, b.v, c, 0, 0, 0);
}
// exact f32: a k-ordered fmaf chain (8 steps of 4 k each; lane (r, q) holds k = 8q .. 8q+7 of both operands, so the pairing is right)
__device__ __forceinline__ f32x4 dys_mma(const Vec8<float>& a, const Vec8<float>& b, f32x4 c) {
#pragma unroll
  for (int j = 0; j < 4; ++j) c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.lo[j], b.lo[j], c, 0, 0, 0);
#pragma unroll
  for (int j = 0; j < 4; ++j) c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.hi[j], b.hi[j], c, 0, 0, 0);
  return c;
}

// NT = 8G / 16 offset-channel tiles.  x [npix][xCs] (C channels used), y [4 npix][yCs]; w_off / w_scope [8G][C] in T, bias / init_pos
// fp32 [8G]; offset channel n = xy * 4G + grp * 4 + i * 2 + j.
template <typename T, int NT, bool SCOPE>
__global__ __launch_bounds__(256) void dysample_kernel(int npix, int H, int W, int C, const T* __restrict__ x, int xCs, const T* __restrict__ w_off,
                                                       const float* __restrict__ bias, const T* __restrict__ w_scope, const float* __restrict__ init_pos,
                                                       T* __restrict__ y, int yCs) {
  constexpr int N = 16 * NT, G = 2 * NT, PITCH = N + 4;
  __shared__ __attribute__((aligned(16))) float offs[DYS_PIX * PITCH];
  __shared__ int pix_h[DYS_PIX], pix_w[DYS_PIX];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int p0 = (int)ey_xcd_block(blockIdx.x, gridDim.x) * DYS_PIX;

  // ---- phase 1: offsets of pixels p0 .. p0+63.  A = weights (row = offset channel), B = pixels: lane (col, kq) holds channels
  // k0 + 8kq .. +7 of pixel `col`; the result has the pixel on the lane and 4 consecutive offset channels in the registers.
  {
    const int col = lane & 15, kq = lane >> 4;
    const int pl = wave * 16 + col;
    int p = p0 + pl;
    if (p >= npix) p = npix - 1;  // tile tail: a valid address, the result is never used
    const T* xp = x + (long)p * xCs + kq * 8;
    const T* wp = w_off + (long)col * C + kq * 8;
    const T* sp = SCOPE ? w_scope + (long)col * C + kq * 8 : nullptr;
    f32x4 acc[NT], sacc[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) { acc[nt] = (f32x4)0.f; sacc[nt] = (f32x4)0.f; }
    for (int k0 = 0; k0 < C; k0 += 32) {
      const bool in = k0 + kq * 8 < C;  // K tail (C % 32 != 0): whole octets, zero in both operands
      Vec8<T> b;
      if (in) b.load(xp + k0); else b.zero();
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        Vec8<T> a;
        if (in) a.load(wp + (long)nt * 16 * C + k0); else a.zero();
        acc[nt] = dys_mma(a, b, acc[nt]);
        if constexpr (SCOPE) {
          if (in) a.load(sp + (long)nt * 16 * C + k0); else a.zero();
          sacc[nt] = dys_mma(a, b, sacc[nt]);
        }
      }
    }
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const int n0 = nt * 16 + kq * 4;
      f32x4 o;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float v = acc[nt][r] + bias[n0 + r];
        o[r] = (SCOPE ? v * ey_sigmoid(sacc[nt][r]) * 0.5f : v * 0.25f) + init_pos[n0 + r];
      }
      *reinterpret_cast<f32x4*>(&offs[pl * PITCH + n0]) = o;
    }
    if (tid < DYS_PIX) {
      int q = p0 + tid;
      if (q >= npix) q = npix - 1;
      pix_w[tid] = q % W;
      pix_h[tid] = (q / W) % H;
    }
  }
  __syncthreads();

  // ---- phase 2: work item = (row parity i, pixel of the tile, column parity j, channel octet), octet fastest: a wave's stores walk
  // the 2 x C contiguous output channels of consecutive input pixels of a row.  256 * C/8 items per tile = C/8 per thread.
  const int noct = C >> 3, octs_per_grp = noct / G;
  const int step_o = 256 % noct, step_r = 256 / noct;
  int oct = tid % noct, r = tid / noct;
  for (int it = 0; it < noct; ++it) {
    const int j = r & 1, pl = (r >> 1) & (DYS_PIX - 1), i = r >> 7;
    const int p = p0 + pl;
    if (p < npix) {
      const int grp = oct / octs_per_grp, sub = i * 2 + j;
      const int h = pix_h[pl], w = pix_w[pl];
      const float ox = offs[pl * PITCH + grp * 4 + sub], oy = offs[pl * PITCH + 4 * G + grp * 4 + sub];
      const float fx = fminf(fmaxf((float)w + ox, 0.f), (float)(W - 1)), fy = fminf(fmaxf((float)h + oy, 0.f), (float)(H - 1));
      int x0 = (int)fx, y0 = (int)fy;  // (fx, fy >= 0: truncation is floor)
      x0 = min(max(x0, 0), W - 1);
      y0 = min(max(y0, 0), H - 1);
      const int x1 = min(x0 + 1, W - 1), y1 = min(y0 + 1, H - 1);
      const float lx = fx - (float)x0, ly = fy - (float)y0;
      const float w00 = (1.f - lx) * (1.f - ly), w01 = lx * (1.f - ly), w10 = (1.f - lx) * ly, w11 = lx * ly;
      const long img = (long)(p - h * W - w);  // first pixel of this image
      const T* xb = x + oct * 8;
      Vec8<T> v00, v01, v10, v11;
      v00.load(xb + (img + (long)y0 * W + x0) * xCs);
      v01.load(xb + (img + (long)y0 * W + x1) * xCs);
      v10.load(xb + (img + (long)y1 * W + x0) * xCs);
      v11.load(xb + (img + (long)y1 * W + x1) * xCs);
      Vec8<T> o;
#pragma unroll
      for (int e = 0; e < 8; ++e) o.set(e, w00 * v00.get(e) + w01 * v01.get(e) + w10 * v10.get(e) + w11 * v11.get(e));
      o.store(y + (4 * img + (long)(2 * h + i) * (2 * W) + 2 * w + j) * yCs + oct * 8);
    }
    oct += step_o;
    r += step_r;
    if (oct >= noct) { oct -= noct; ++r; }
  }
}

template <typename T>
static void dys_launch(int G, bool scope, dim3 grid, hipStream_t st, int npix, int H, int W, int C, const void* x, int xCs, const void* w_off, const float* bias,
                       const void* w_scope, const float* init_pos, void* y, int yCs) {
#define DYS(NT, S)                                                                                                                                   \
  hipLaunchKernelGGL((dysample_kernel<T, NT, S>), grid, dim3(256), 0, st, npix, H, W, C, (const T*)x, xCs, (const T*)w_off, bias, (const T*)w_scope, \
                     init_pos, (T*)y, yCs)
  if (G == 2) { if (scope) DYS(1, true); else DYS(1, false); }
  else if (G == 4) { if (scope) DYS(2, true); else DYS(2, false); }
  else { if (scope) DYS(4, true); else DYS(4, false); }
#undef DYS
}

extern "C" int ey_dysample(int dtype, int B, int H, int W, int C, int scale, int groups, const void* x, int x_cstride, const void* w_offset, const float* bias,
                           const void* w_scope, const float* init_pos, void* y, int y_cstride, ey_stream_t stream) {
  EY_CHECK(x && w_offset && bias && init_pos && y, "dysample: null pointer");
  EY_CHECK(dtype == EY_F16 || dtype == EY_F32, "dysample: bad dtype");
  EY_CHECK(B > 0 && H > 0 && W > 0 && C > 0 && x_cstride >= C && y_cstride >= C, "dysample: B=%d H=%d W=%d C=%d", B, H, W, C);
  if (scale != 2) return ey_set_error(EY_EUNSUPPORTED, "dysample: scale=%d (2 is built)", scale);
  if (groups != 2 && groups != 4 && groups != 8) return ey_set_error(EY_EUNSUPPORTED, "dysample: groups=%d (2, 4 and 8 are built)", groups);
  if (C % groups || (C / groups) % 8)
    return ey_set_error(EY_EUNSUPPORTED, "dysample: C=%d with groups=%d: the channels of a group must be a multiple of 8", C, groups);
  const size_t es = dtype == EY_F16 ? 2 : 4;
  if (!ey_aligned(x, 16) || !ey_aligned(y, 16) || ((size_t)x_cstride * es) % 16 || ((size_t)y_cstride * es) % 16)
    return ey_set_error(EY_EUNSUPPORTED, "dysample: x and y must be 16-byte aligned channel windows (pixel strides multiples of 16 bytes)");
  EY_CHECK(ey_aligned(w_offset, 16) && (!w_scope || ey_aligned(w_scope, 16)), "dysample: weights must be 16-byte aligned");
  const long npix = (long)B * H * W;
  if (npix * 4 >= (1L << 31)) return ey_set_error(EY_EUNSUPPORTED, "dysample: tensor too large (%ld output pixels)", npix * 4);
  const dim3 grid((unsigned)ey_cdiv(npix, DYS_PIX));
  hipStream_t st = (hipStream_t)stream;
  if (dtype == EY_F16) dys_launch<f16>(groups, w_scope != nullptr, grid, st, (int)npix, H, W, C, x, x_cstride, w_offset, bias, w_scope, init_pos, y, y_cstride);
  else dys_launch<float>(groups, w_scope != nullptr, grid, st, (int)npix, H, W, C, x, x_cstride, w_offset, bias, w_scope, init_pos, y, y_cstride);
  EY_LAUNCH_CHECK("ey_dysample");
  return EY_OK;
}
