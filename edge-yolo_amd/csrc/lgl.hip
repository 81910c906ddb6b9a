// The small kernels of the Local-Global-Local block (LGLBlock = LocalAgg + SelfAttn, reference block.py:3042-3210) that no other model
// needs: depthwise 9x9 / 3x3 with a sigmoid-gate or residual epilogue, the per-channel CMlp stencil, LayerNorm over the channels of a
// pixel (optionally fused with the ceil-mode 2x2 average pool in front of the attention), the depthwise transposed 2x2 un-pool fused with
// the LayerNorm behind it, and the exact (erf) GELU.  All statistics, gates and stencil sums are fp32 in both storage types; every
// kernel writes its channel window only.
#include "common.h"

// 8 consecutive channels of one pixel <-> fp32 registers.  vec: 16-byte transactions (the host checked alignment), else element-wise.
template <typename T>
__device__ __forceinline__ void lgl_ld8(const T* p, bool vec, float (&o)[8]) {
  if (vec) {
    Vec8<T> t;
    t.load(p);
#pragma unroll
    for (int i = 0; i < 8; ++i) o[i] = t.get(i);
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i) o[i] = to_f(p[i]);
  }
}
template <typename T>
__device__ __forceinline__ void lgl_st8(T* p, bool vec, const float (&o)[8]) {
  if (vec) {
    Vec8<T> t;
#pragma unroll
    for (int i = 0; i < 8; ++i) t.set(i, o[i]);
    t.store(p);
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i) p[i] = from_f<T>(o[i]);
  }
}
template <typename T>
static bool lgl_vec_ok(const void* p, int cstride) {
  return ey_aligned(p, 16) && ((size_t)cstride * sizeof(T)) % 16 == 0;
}
// x + x * (sigmoid(g) - 1/2): the gate of all three LocalAgg steps (block.py:3093-3095)
__device__ __forceinline__ float lgl_gate(float x, float g) { return x + x * (ey_sigmoid(g) - 0.5f); }
__device__ __forceinline__ float lgl_gelu(float x) { return 0.5f * x * (1.f + erff(x * 0.70710678118654752440f)); }

// ---- depthwise K x K, stride 1, pad K/2, + bias, one thread per (pixel, channel octet); taps summed in fp32 in row-major order.
// mode 0: y = dw(x) + b      1: y = gate(x, dw(x) + b)      2: y = x + (dw(x) + b)
template <typename T, int K>
__global__ __launch_bounds__(256) void lgl_dw_kernel(int B, int H, int W, int C, int mode, bool vec, const T* __restrict__ x, int xCs, const T* __restrict__ w,
                                                      const float* __restrict__ bias, T* __restrict__ y, int yCs) {
  const int oct = C >> 3;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long)B * H * W * oct) return;
  const int c0 = (int)(idx % oct) * 8;
  const long pix = idx / oct;
  const int px = (int)(pix % W), py = (int)((pix / W) % H);
  const long img = pix / ((long)W * H) * H * W;
  float acc[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) acc[i] = bias ? bias[c0 + i] : 0.f;
  for (int dy = 0; dy < K; ++dy) {
    const int yy = py + dy - K / 2;
    if (yy < 0 || yy >= H) continue;
    for (int dx = 0; dx < K; ++dx) {
      const int xx = px + dx - K / 2;
      if (xx < 0 || xx >= W) continue;
      float a[8], f[8];
      lgl_ld8(x + (img + (long)yy * W + xx) * xCs + c0, vec, a);
      lgl_ld8(w + (dy * K + dx) * C + c0, true, f);
#pragma unroll
      for (int i = 0; i < 8; ++i) acc[i] = fmaf(a[i], f[i], acc[i]);
    }
  }
  if (mode) {
    float a[8];
    lgl_ld8(x + pix * xCs + c0, vec, a);
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] = mode == 1 ? lgl_gate(a[i], acc[i]) : a[i] + acc[i];
  }
  lgl_st8(y + pix * yCs + c0, vec, acc);
}

extern "C" int ey_dwconv_gate(int dtype, int B, int H, int W, int C, int k, int mode, const void* x, int x_cstride, const void* w_kkc, const float* bias,
                              void* y, int y_cstride, ey_stream_t stream) {
  EY_CHECK(x && w_kkc && y, "dwconv_gate: null pointer");
  EY_CHECK(dtype == EY_F16 || dtype == EY_F32, "dwconv_gate: bad dtype");
  EY_CHECK(B > 0 && H > 0 && W > 0 && C > 0 && x_cstride >= C && y_cstride >= C, "dwconv_gate: B=%d H=%d W=%d C=%d", B, H, W, C);
  EY_CHECK(mode >= 0 && mode <= 2, "dwconv_gate: mode %d", mode);
  if (k != 3 && k != 9) return ey_set_error(EY_EUNSUPPORTED, "dwconv_gate: k=%d (3 and 9 are built)", k);
  if (C % 8) return ey_set_error(EY_EUNSUPPORTED, "dwconv_gate: C=%d is not a multiple of 8", C);
  EY_CHECK(ey_aligned(w_kkc, 32), "dwconv_gate: weights must be 32-byte aligned");
  const long total = (long)B * H * W * (C / 8);
  if ((long)B * H * W * (long)(x_cstride > y_cstride ? x_cstride : y_cstride) >= (1L << 31) || total >= (1L << 39))
    return ey_set_error(EY_EUNSUPPORTED, "dwconv_gate: tensor too large");
  const dim3 grid((unsigned)((total + 255) / 256));
  hipStream_t st = (hipStream_t)stream;
#define DWG(T, K)                                                                                                                              \
  hipLaunchKernelGGL((lgl_dw_kernel<T, K>), grid, dim3(256), 0, st, B, H, W, C, mode, lgl_vec_ok<T>(x, x_cstride) && lgl_vec_ok<T>(y, y_cstride), \
                     (const T*)x, x_cstride, (const T*)w_kkc, bias, (T*)y, y_cstride)
  if (dtype == EY_F16) { if (k == 9) DWG(f16, 9); else DWG(f16, 3); }
  else { if (k == 9) DWG(float, 9); else DWG(float, 3); }
#undef DWG
  EY_LAUNCH_CHECK("ey_dwconv_gate");
  return EY_OK;
}

// ---- element-wise: OP 0: y = gate(x, g)    OP 1: y = GELU(x) (exact, erf).  Any C; one thread per element.
template <typename T, int OP>
__global__ __launch_bounds__(256) void lgl_eltwise_kernel(long total, int C, const T* x, int xCs, const T* g, int gCs, T* y,
                                                           int yCs) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int c = (int)(idx % C);
  const long pix = idx / C;
  const float a = to_f(x[pix * xCs + c]);
  y[pix * yCs + c] = from_f<T>(OP == 0 ? lgl_gate(a, to_f(g[pix * gCs + c])) : lgl_gelu(a));
}

static int lgl_eltwise(int op, int dtype, int B, int H, int W, int C, const void* x, int xCs, const void* g, int gCs, void* y, int yCs, ey_stream_t stream,
                       const char* name) {
  EY_CHECK(x && y && (op || g), "%s: null pointer", name);
  EY_CHECK(dtype == EY_F16 || dtype == EY_F32, "%s: bad dtype", name);
  EY_CHECK(B > 0 && H > 0 && W > 0 && C > 0 && xCs >= C && yCs >= C && (op || gCs >= C), "%s: B=%d H=%d W=%d C=%d", name, B, H, W, C);
  const long total = (long)B * H * W * C;
  if (total >= (1L << 39)) return ey_set_error(EY_EUNSUPPORTED, "%s: tensor too large", name);
  const dim3 grid((unsigned)((total + 255) / 256));
  hipStream_t st = (hipStream_t)stream;
#define ELT(T, OP) hipLaunchKernelGGL((lgl_eltwise_kernel<T, OP>), grid, dim3(256), 0, st, total, C, (const T*)x, xCs, (const T*)g, gCs, (T*)y, yCs)
  if (dtype == EY_F16) { if (op == 0) ELT(f16, 0); else ELT(f16, 1); }
  else { if (op == 0) ELT(float, 0); else ELT(float, 1); }
#undef ELT
  EY_LAUNCH_CHECK(name);
  return EY_OK;
}
extern "C" int ey_sigmoid_gate(int dtype, int B, int H, int W, int C, const void* x, int x_cstride, const void* g, int g_cstride, void* y, int y_cstride,
                               ey_stream_t stream) {
  return lgl_eltwise(0, dtype, B, H, W, C, x, x_cstride, g, g_cstride, y, y_cstride, stream, "ey_sigmoid_gate");
}
extern "C" int ey_gelu(int dtype, int B, int H, int W, int C, const void* x, int x_cstride, void* y, int y_cstride, ey_stream_t stream) {
  return lgl_eltwise(1, dtype, B, H, W, C, x, x_cstride, nullptr, 0, y, y_cstride, stream, "ey_gelu");
}

// ---- CMlp (block.py:3060-3076) behind an input affine, per channel: a = scale * x + shift inside the map and ZERO outside it (the
// reference pads the BatchNorm's output), hidden_j = GELU(b1_j + 3x3_j(a)) for the R maps of the channel, zero outside the map too
// (fc2's padding), o = b2 + sum_j 3x3_j(hidden_j).  One thread per (pixel, channel): the 5x5 window of a and the 9 x R hidden values
// it needs live in registers.  gate: y = gate(x, o) instead of o.  Weights fp32: w1 / w2 [R][9][C], b1 [R][C], b2 / scale / shift [C].
#define CMLP_MAXR 8
template <typename T, int RT>
__global__ __launch_bounds__(256) void lgl_cmlp_kernel(int B, int H, int W, int C, int rr, int gate, const T* __restrict__ x, int xCs, const float* __restrict__ scale,
                                                        const float* __restrict__ shift, const float* __restrict__ w1, const float* __restrict__ b1,
                                                        const float* __restrict__ w2, const float* __restrict__ b2, T* __restrict__ y, int yCs) {
  const int R = RT ? RT : rr;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long)B * H * W * C) return;
  const int c = (int)(idx % C);
  const long pix = idx / C;
  const int px = (int)(pix % W), py = (int)((pix / W) % H);
  const long img = pix / ((long)W * H) * H * W;
  const float sc = scale ? scale[c] : 1.f, sh = shift ? shift[c] : 0.f;
  float a[5][5];
#pragma unroll
  for (int dy = 0; dy < 5; ++dy)
#pragma unroll
    for (int dx = 0; dx < 5; ++dx) {
      const int yy = py + dy - 2, xx = px + dx - 2;
      a[dy][dx] = (yy >= 0 && yy < H && xx >= 0 && xx < W) ? fmaf(to_f(x[(img + (long)yy * W + xx) * xCs + c]), sc, sh) : 0.f;
    }
  float o = b2[c];
#pragma unroll 1
  for (int j = 0; j < R; ++j) {
    float f1[9], f2[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) { f1[t] = w1[(j * 9 + t) * C + c]; f2[t] = w2[(j * 9 + t) * C + c]; }
    const float bj = b1[j * C + c];
#pragma unroll
    for (int hy = 0; hy < 3; ++hy)
#pragma unroll
      for (int hx = 0; hx < 3; ++hx) {
        const int yy = py + hy - 1, xx = px + hx - 1;
        if (yy < 0 || yy >= H || xx < 0 || xx >= W) continue;  // hidden map zero-padded
        float s = bj;
#pragma unroll
        for (int t = 0; t < 9; ++t) s = fmaf(f1[t], a[hy + t / 3][hx + t % 3], s);
        o = fmaf(f2[hy * 3 + hx], lgl_gelu(s), o);
      }
  }
  y[pix * yCs + c] = from_f<T>(gate ? lgl_gate(to_f(x[pix * xCs + c]), o) : o);
}

extern "C" int ey_cmlp(int dtype, int B, int H, int W, int C, int r, int gate, const void* x, int x_cstride, const float* scale, const float* shift,
                       const float* w1, const float* b1, const float* w2, const float* b2, void* y, int y_cstride, ey_stream_t stream) {
  EY_CHECK(x && y && w1 && b1 && w2 && b2, "cmlp: null pointer");
  EY_CHECK(dtype == EY_F16 || dtype == EY_F32, "cmlp: bad dtype");
  EY_CHECK(B > 0 && H > 0 && W > 0 && C > 0 && x_cstride >= C && y_cstride >= C, "cmlp: B=%d H=%d W=%d C=%d", B, H, W, C);
  if (r < 1 || r > CMLP_MAXR) return ey_set_error(EY_EUNSUPPORTED, "cmlp: %d hidden maps per channel (1..%d are built)", r, CMLP_MAXR);
  const long total = (long)B * H * W * C;
  if (total >= (1L << 39)) return ey_set_error(EY_EUNSUPPORTED, "cmlp: tensor too large");
  const dim3 grid((unsigned)((total + 255) / 256));
  hipStream_t st = (hipStream_t)stream;
#define CMLP(T, RT) \
  hipLaunchKernelGGL((lgl_cmlp_kernel<T, RT>), grid, dim3(256), 0, st, B, H, W, C, r, gate, (const T*)x, x_cstride, scale, shift, w1, b1, w2, b2, (T*)y, y_cstride)
  if (dtype == EY_F16) { if (r == 4) CMLP(f16, 4); else CMLP(f16, 0); }
  else { if (r == 4) CMLP(float, 4); else CMLP(float, 0); }
#undef CMLP
  EY_LAUNCH_CHECK("ey_cmlp");
  return EY_OK;
}

// ---- LayerNorm over the C channels of a pixel: LPP = 2..16 lanes share a pixel, a lane holds up to 3 channel octets in registers
// (C <= 384), mean and variance in two passes over those registers with xor-shuffle sums inside the lane group.
#define LN_MAXC 384
static int ln_lpp(int C) {
  int l = 1;
  while (l < C / 8 && l < 16) l <<= 1;
  return l;
}
// v: this lane's octets sub, sub + lpp, ... of one pixel; normalised in place: (v - mean) * rstd * gamma + beta
__device__ __forceinline__ void ln_normalise(float (&v)[3][8], int C, int sub, int lpp, float eps, const float* __restrict__ gamma, const float* __restrict__ beta) {
  const int noct = C >> 3;
  float s = 0.f;
#pragma unroll
  for (int u = 0; u < 3; ++u)
    if (sub + u * lpp < noct) {
#pragma unroll
      for (int i = 0; i < 8; ++i) s += v[u][i];
    }
  for (int o = 1; o < lpp; o <<= 1) s += __shfl_xor(s, o);
  const float mean = s / (float)C;
  float q = 0.f;
#pragma unroll
  for (int u = 0; u < 3; ++u)
    if (sub + u * lpp < noct) {
#pragma unroll
      for (int i = 0; i < 8; ++i) { const float d = v[u][i] - mean; q = fmaf(d, d, q); }
    }
  for (int o = 1; o < lpp; o <<= 1) q += __shfl_xor(q, o);
  const float rstd = 1.f / sqrtf(q / (float)C + eps);
#pragma unroll
  for (int u = 0; u < 3; ++u)
    if (sub + u * lpp < noct) {
      const int c0 = (sub + u * lpp) * 8;
#pragma unroll
      for (int i = 0; i < 8; ++i) v[u][i] = (v[u][i] - mean) * rstd * gamma[c0 + i] + beta[c0 + i];
    }
}

// pool 0: y[p] = LN(x[p]).  pool 1: AvgPool2d(2, 2, ceil_mode=True) of LN(x): y[i][j] = mean over the in-bounds pixels of the window at
// (2i, 2j) of their normalised values (a partial window divides by its in-bounds count), Ho = ceil(H/2), Wo = ceil(W/2).
template <typename T>
__global__ __launch_bounds__(256) void lgl_layernorm_kernel(int B, int H, int W, int C, int pool, int lpp, float eps, bool vec, const T* __restrict__ x, int xCs,
                                                             const float* __restrict__ gamma, const float* __restrict__ beta, T* __restrict__ y, int yCs) {
  const int Ho = pool ? (H + 1) >> 1 : H, Wo = pool ? (W + 1) >> 1 : W;
  const long gid = ((long)blockIdx.x * 256 + threadIdx.x) / lpp;
  const int sub = threadIdx.x % lpp, noct = C >> 3;
  // (a whole lane group leaves together: lpp divides 256 and the shuffles below stay inside converged groups)
  if (gid >= (long)B * Ho * Wo) return;
  const int ox = (int)(gid % Wo), oy = (int)((gid / Wo) % Ho);
  const long b = gid / ((long)Wo * Ho);
  float out[3][8];
#pragma unroll
  for (int u = 0; u < 3; ++u)
#pragma unroll
    for (int i = 0; i < 8; ++i) out[u][i] = 0.f;
  const int win = pool ? 2 : 1;
  int cnt = 0;
  for (int dy = 0; dy < win; ++dy)
    for (int dx = 0; dx < win; ++dx) {
      const int yy = oy * win + dy, xx = ox * win + dx;
      if (yy >= H || xx >= W) continue;  // uniform in the lane group
      const T* p = x + ((b * H + yy) * W + xx) * xCs;
      float v[3][8];
#pragma unroll
      for (int u = 0; u < 3; ++u)
        if (sub + u * lpp < noct) lgl_ld8(p + (sub + u * lpp) * 8, vec, v[u]);
      ln_normalise(v, C, sub, lpp, eps, gamma, beta);
#pragma unroll
      for (int u = 0; u < 3; ++u)
#pragma unroll
        for (int i = 0; i < 8; ++i) out[u][i] += v[u][i];
      ++cnt;
    }
  if (pool) {
    const float inv = 1.f / (float)cnt;  // 1, 1/2, 1/4: exact
#pragma unroll
    for (int u = 0; u < 3; ++u)
#pragma unroll
      for (int i = 0; i < 8; ++i) out[u][i] *= inv;
  }
  T* q = y + ((b * Ho + oy) * Wo + ox) * yCs;
#pragma unroll
  for (int u = 0; u < 3; ++u)
    if (sub + u * lpp < noct) lgl_st8(q + (sub + u * lpp) * 8, vec, out[u]);
}

static int ln_check(const char* name, int dtype, int B, int H, int W, int C, const void* x, int xCs, const float* gamma, const float* beta, const void* y, int yCs) {
  EY_CHECK(x && y && gamma && beta, "%s: null pointer", name);
  EY_CHECK(dtype == EY_F16 || dtype == EY_F32, "%s: bad dtype", name);
  EY_CHECK(B > 0 && H > 0 && W > 0 && C > 0 && xCs >= C && yCs >= C, "%s: B=%d H=%d W=%d C=%d", name, B, H, W, C);
  if (C % 8 || C > LN_MAXC) return ey_set_error(EY_EUNSUPPORTED, "%s: C=%d (multiples of 8 up to %d are built)", name, C, LN_MAXC);
  return EY_OK;
}

extern "C" int ey_layernorm_channels(int dtype, int B, int H, int W, int C, float eps, int pool, const void* x, int x_cstride, const float* gamma,
                                     const float* beta, void* y, int y_cstride, ey_stream_t stream) {
  const int rc = ln_check("layernorm_channels", dtype, B, H, W, C, x, x_cstride, gamma, beta, y, y_cstride);
  if (rc) return rc;
  const int lpp = ln_lpp(C);
  const long groups = (long)B * (pool ? (H + 1) / 2 : H) * (pool ? (W + 1) / 2 : W);
  if (groups * lpp >= (1L << 39)) return ey_set_error(EY_EUNSUPPORTED, "layernorm_channels: tensor too large");
  const dim3 grid((unsigned)((groups * lpp + 255) / 256));
  hipStream_t st = (hipStream_t)stream;
  if (dtype == EY_F16)
    hipLaunchKernelGGL(lgl_layernorm_kernel<f16>, grid, dim3(256), 0, st, B, H, W, C, pool ? 1 : 0, lpp, eps, lgl_vec_ok<f16>(x, x_cstride) && lgl_vec_ok<f16>(y, y_cstride),
                       (const f16*)x, x_cstride, gamma, beta, (f16*)y, y_cstride);
  else
    hipLaunchKernelGGL(lgl_layernorm_kernel<float>, grid, dim3(256), 0, st, B, H, W, C, pool ? 1 : 0, lpp, eps,
                       lgl_vec_ok<float>(x, x_cstride) && lgl_vec_ok<float>(y, y_cstride), (const float*)x, x_cstride, gamma, beta, (float*)y, y_cstride);
  EY_LAUNCH_CHECK("ey_layernorm_channels");
  return EY_OK;
}

// ---- LocalProp + norm of GlobalSparseAttn (block.py:3155-3162): depthwise ConvTranspose2d(k 2, s 2, no bias) of t [B,Hs,Ws,C],
//   U[2i+a][2j+b][c] = t[i][j][c] * w[a][b][c],
// then, only when (2Hs, 2Ws) != (H, W) (an odd map), F.interpolate(U, (H, W), bilinear, align_corners=False) with the ATen source-index
// rule, then LayerNorm over the channels of each of the H x W pixels.  U is never written.  w: fp32 [2][2][C].
__device__ __forceinline__ void unpool_src(int o, int in, int out, int& i0, int& i1, float& l1) {
  float s = ((float)in / (float)out) * ((float)o + 0.5f) - 0.5f;
  if (s < 0.f) s = 0.f;
  i0 = (int)s;
  if (i0 > in - 1) i0 = in - 1;
  i1 = i0 + (i0 < in - 1 ? 1 : 0);
  l1 = s - (float)i0;
}
template <typename T>
__global__ __launch_bounds__(256) void lgl_unpool_ln_kernel(int B, int Hs, int Ws, int H, int W, int C, int lpp, float eps, bool vec, const T* __restrict__ t, int tCs,
                                                             const float* __restrict__ w, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                             T* __restrict__ y, int yCs) {
  const long gid = ((long)blockIdx.x * 256 + threadIdx.x) / lpp;
  const int sub = threadIdx.x % lpp, noct = C >> 3;
  if (gid >= (long)B * H * W) return;
  const int ox = (int)(gid % W), oy = (int)((gid / W) % H);
  const long b = gid / ((long)W * H);
  const bool exact = 2 * Hs == H && 2 * Ws == W;
  int ys[2], xs[2];
  float ly = 0.f, lx = 0.f;
  if (exact) {
    ys[0] = ys[1] = oy;
    xs[0] = xs[1] = ox;
  } else {
    unpool_src(oy, 2 * Hs, H, ys[0], ys[1], ly);
    unpool_src(ox, 2 * Ws, W, xs[0], xs[1], lx);
  }
  float v[3][8];
#pragma unroll
  for (int u = 0; u < 3; ++u) {
    if (sub + u * lpp >= noct) continue;
    const int c0 = (sub + u * lpp) * 8;
    float U[2][2][8];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        if (exact && (a || e)) continue;
        float tv[8];
        lgl_ld8(t + ((b * Hs + (ys[a] >> 1)) * Ws + (xs[e] >> 1)) * tCs + c0, vec, tv);
        const float* wp = w + ((ys[a] & 1) * 2 + (xs[e] & 1)) * C + c0;
#pragma unroll
        for (int i = 0; i < 8; ++i) U[a][e][i] = tv[i] * wp[i];
      }
#pragma unroll
    for (int i = 0; i < 8; ++i)
      v[u][i] = exact ? U[0][0][i] : (1.f - ly) * ((1.f - lx) * U[0][0][i] + lx * U[0][1][i]) + ly * ((1.f - lx) * U[1][0][i] + lx * U[1][1][i]);
  }
  ln_normalise(v, C, sub, lpp, eps, gamma, beta);
  T* q = y + ((b * H + oy) * W + ox) * yCs;
#pragma unroll
  for (int u = 0; u < 3; ++u)
    if (sub + u * lpp < noct) lgl_st8(q + (sub + u * lpp) * 8, vec, v[u]);
}

extern "C" int ey_unpool2_layernorm(int dtype, int B, int Hs, int Ws, int H, int W, int C, float eps, const void* t, int t_cstride, const float* w_abc,
                                    const float* gamma, const float* beta, void* y, int y_cstride, ey_stream_t stream) {
  const int rc = ln_check("unpool2_layernorm", dtype, B, H, W, C, t, t_cstride, gamma, beta, y, y_cstride);
  if (rc) return rc;
  EY_CHECK(w_abc, "unpool2_layernorm: null pointer");
  EY_CHECK(Hs == (H + 1) / 2 && Ws == (W + 1) / 2, "unpool2_layernorm: a %dx%d map does not un-pool to %dx%d", Hs, Ws, H, W);
  const int lpp = ln_lpp(C);
  const long groups = (long)B * H * W;
  if (groups * lpp >= (1L << 39)) return ey_set_error(EY_EUNSUPPORTED, "unpool2_layernorm: tensor too large");
  const dim3 grid((unsigned)((groups * lpp + 255) / 256));
  hipStream_t st = (hipStream_t)stream;
  if (dtype == EY_F16)
    hipLaunchKernelGGL(lgl_unpool_ln_kernel<f16>, grid, dim3(256), 0, st, B, Hs, Ws, H, W, C, lpp, eps, lgl_vec_ok<f16>(t, t_cstride) && lgl_vec_ok<f16>(y, y_cstride),
                       (const f16*)t, t_cstride, w_abc, gamma, beta, (f16*)y, y_cstride);
  else
    hipLaunchKernelGGL(lgl_unpool_ln_kernel<float>, grid, dim3(256), 0, st, B, Hs, Ws, H, W, C, lpp, eps,
                       lgl_vec_ok<float>(t, t_cstride) && lgl_vec_ok<float>(y, y_cstride), (const float*)t, t_cstride, w_abc, gamma, beta, (float*)y, y_cstride);
  EY_LAUNCH_CHECK("ey_unpool2_layernorm");
  return EY_OK;
}
