// Adaptive hypergraph convolution of YOLOv13's HyperACE (AdaHGConv, reference block.py:1640-1779): ey_hypergraph_conv.
//
// One image's N tokens are the pixels of an NHWC map (D channels, no transpose).  With E hyperedges and `heads` heads:
//   ctx    = [mean_N X ; max_N X]                                   (context "both"; "mean" / "max" take one half)
//   P      = prototype_base + context_net(ctx)                      (E x D per image)
//   logits = mean_h (Xp_h . P_h) / sqrt(D/heads),  Xp = pre_head_proj(X)
//          = (X . Q[e] + c[e]) / (sqrt(D/heads) * heads)  with  Q = P Wp,  c = P bp  (the heads collapse; Xp is folded away)
//   A      = softmax over the N tokens, per hyperedge
//   He'    = GELU(edge_proj(A^T X))
//   Y      = GELU(node_proj(A He')) + X
// Five launches, each whole-image reduction a launch seam (no grid barrier, no float atomics: every sum has a fixed order, so the
// result is identical run to run):
//   1 hg_stats_kernel     per (image, 256-token chunk): channel sums and maxima
//   2 hg_proto_kernel     per (image, edge): ctx from the chunk partials, P, then Q = P Wp and c = P bp
//   3 hg_softmax_kernel   per (image, 128-token chunk): logits (kept for launch 5) and online-softmax partials (max m, sum s, sum p X)
//   4 hg_edge_kernel      per (image, edge): merge the partials -> He = A^T X, then He' = GELU(edge_proj(He))
//   5 hg_expand_kernel    per token tile: A from the logits and the final (m, s), Z = A He' (rounded to the storage type, as the
//                         reference's bmm output is), node_proj (f16: MFMA 16x16x32, fp32: exact VALU) + bias, GELU, + X
// Everything but X, Y and (f16) the node_proj operands is fp32.
#include "common.h"
#include <math.h>

namespace {

constexpr int HG_STAT_CH = 256;  // tokens per stats partial (launch 1)
constexpr int HG_CHUNK = 128;    // tokens per softmax partial (launch 3): two sub-tiles of HG_TT
constexpr int HG_TT = 64;        // sub-tile of launch 3 (4 threads per token for the logits)
constexpr int HG_MAXD = 384;
constexpr int HG_MAXE = 16;

__host__ __device__ inline size_t hg_al16(size_t b) { return (b + 15) & ~size_t(15); }

struct HgWs {
  float *st, *Q, *c, *lg, *pm, *ps, *ph, *M, *S, *He;
  size_t bytes;
};

HgWs hg_layout(char* base, int B, int N, int D, int E) {
  const size_t Ts = (size_t)ey_cdiv(N, HG_STAT_CH), Tc = (size_t)ey_cdiv(N, HG_CHUNK);
  HgWs w;
  size_t off = 0;
  auto take = [&](float*& p, size_t n) {
    p = (float*)(base + off);
    off += hg_al16(n * sizeof(float));
  };
  take(w.st, (size_t)B * Ts * 2 * D);
  take(w.Q, (size_t)B * E * D);
  take(w.c, (size_t)B * E);
  take(w.lg, (size_t)B * N * E);
  take(w.pm, (size_t)B * Tc * E);
  take(w.ps, (size_t)B * Tc * E);
  take(w.ph, (size_t)B * Tc * E * D);
  take(w.M, (size_t)B * E);
  take(w.S, (size_t)B * E);
  take(w.He, (size_t)B * E * D);
  w.bytes = off;
  return w;
}

// nn.GELU() (approximate='none'): x/2 * (1 + erf(x/sqrt(2)))
__device__ __forceinline__ float hg_gelu(float x) { return x * 0.5f * (1.0f + erff(x * 0.70710678118654752f)); }

// ---- 1: per-chunk channel sums and maxima.  grid (Ts, B).  Channels on the threads (coalesced), G token lanes when D < 256.
template <typename T>
__global__ __launch_bounds__(256) void hg_stats_kernel(int N, int D, const T* __restrict__ x, int xcs, float* __restrict__ st) {
  __shared__ float ls[256], lm[256];
  const int t = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int n0 = t * HG_STAT_CH, n1 = min(N, n0 + HG_STAT_CH);
  const int cw = D < 256 ? D : 256, G = 256 / cw, g = tid / cw, dl = tid % cw;
  const T* xb = x + (long)b * N * xcs;
  float* out = st + ((long)b * gridDim.x + t) * 2 * D;
  for (int d0 = 0; d0 < D; d0 += cw) {
    const int d = d0 + dl;
    float s = 0.f, m = -INFINITY;
    if (g < G && d < D)
      for (int n = n0 + g; n < n1; n += G) {
        const float v = to_f(xb[(long)n * xcs + d]);
        s += v;
        m = fmaxf(m, v);
      }
    ls[tid] = s;
    lm[tid] = m;
    __syncthreads();
    if (g == 0 && d < D) {
      for (int j = 1; j < G; ++j) {
        s += ls[j * cw + dl];
        m = fmaxf(m, lm[j * cw + dl]);
      }
      out[d] = s;
      out[D + d] = m;
    }
    __syncthreads();
  }
}

// ---- 2: prototypes and the folded pre_head_proj.  grid (E, B).
//   ctx_wT: context_net.weight transposed, [K][E*D] (K = 2D for "both", else D); pre_w: pre_head_proj.weight [D out][D in].
__global__ __launch_bounds__(256) void hg_proto_kernel(int N, int D, int E, int Ts, int ctxmode, const float* __restrict__ st,
                                                       const float* __restrict__ base, const float* __restrict__ cwT, const float* __restrict__ cb,
                                                       const float* __restrict__ pw, const float* __restrict__ pb, float* __restrict__ Q,
                                                       float* __restrict__ c) {
  __shared__ float ctx[2 * HG_MAXD], P[HG_MAXD], red[256];
  const int e = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const float* sb = st + (long)b * Ts * 2 * D;
  for (int d = tid; d < D; d += 256) {
    float s = 0.f, m = -INFINITY;
    for (int t = 0; t < Ts; ++t) {
      s += sb[(long)t * 2 * D + d];
      m = fmaxf(m, sb[(long)t * 2 * D + D + d]);
    }
    const float mean = s / (float)N;
    if (ctxmode == 0) {
      ctx[d] = mean;
      ctx[D + d] = m;
    } else {
      ctx[d] = ctxmode == 1 ? mean : m;
    }
  }
  __syncthreads();
  const int K = ctxmode == 0 ? 2 * D : D;
  const long ED = (long)E * D;
  for (int d = tid; d < D; d += 256) {
    const long o = (long)e * D + d;
    float acc = 0.f;
    for (int k = 0; k < K; ++k) acc = fmaf(ctx[k], cwT[k * ED + o], acc);
    P[d] = base[o] + (acc + cb[o]);
  }
  __syncthreads();
  float* q = Q + ((long)b * E + e) * D;
  for (int j = tid; j < D; j += 256) {
    float acc = 0.f;
    for (int i = 0; i < D; ++i) acc = fmaf(P[i], pw[(long)i * D + j], acc);
    q[j] = acc;
  }
  float part = 0.f;
  for (int i = tid; i < D; i += 256) part = fmaf(P[i], pb[i], part);
  red[tid] = part;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  if (tid == 0) c[(long)b * E + e] = red[0];
}

// ---- 3: logits + online-softmax partials per 128-token chunk.  grid (Tc, B).
template <typename T>
__global__ __launch_bounds__(256) void hg_softmax_kernel(int N, int D, int E, float div, const T* __restrict__ x, int xcs, const float* __restrict__ Q,
                                                         const float* __restrict__ c, float* __restrict__ lg, float* __restrict__ pm,
                                                         float* __restrict__ ps, float* __restrict__ ph) {
  __shared__ float Qs[HG_MAXE * HG_MAXD];
  __shared__ float pl[HG_TT * HG_MAXE];  // logits, then exp(l - m)
  __shared__ float mrun[HG_MAXE], srun[HG_MAXE], alpha[HG_MAXE], cs[HG_MAXE];
  __shared__ float red[256 * HG_MAXE];
  const int t = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, Tc = gridDim.x;
  const T* xb = x + (long)b * N * xcs;
  for (int i = tid; i < E * D; i += 256) Qs[i] = Q[(long)b * E * D + i];
  if (tid < E) {
    cs[tid] = c[(long)b * E + tid];
    mrun[tid] = -INFINITY;
    srun[tid] = 0.f;
  }
  // phase-C ownership: channel d = dl (+256), token lane g of G
  const int cw = D < 256 ? D : 256, G = 256 / cw, g = tid / cw, dl = tid % cw;
  const bool own0 = g < G, own1 = g < G && dl + 256 < D;
  float h0[HG_MAXE], h1[HG_MAXE];
#pragma unroll
  for (int e = 0; e < HG_MAXE; ++e) h0[e] = h1[e] = 0.f;
  __syncthreads();
  const int c0 = t * HG_CHUNK, c1 = min(N, c0 + HG_CHUNK);
  for (int n0 = c0; n0 < c1; n0 += HG_TT) {
    const int nt = min(HG_TT, c1 - n0);
    {  // A: logits, 4 threads per token, each a quarter of the channels
      const int nl = tid >> 2, qq = tid & 3, dq = D >> 2;
      float acc[HG_MAXE];
#pragma unroll
      for (int e = 0; e < HG_MAXE; ++e) acc[e] = 0.f;
      if (nl < nt) {
        const T* xr = xb + (long)(n0 + nl) * xcs + qq * dq;
        for (int d = 0; d < dq; ++d) {
          const float v = to_f(xr[d]);
#pragma unroll
          for (int e = 0; e < HG_MAXE; ++e)
            if (e < E) acc[e] = fmaf(v, Qs[e * D + qq * dq + d], acc[e]);
        }
      }
#pragma unroll
      for (int e = 0; e < HG_MAXE; ++e) {
        acc[e] += __shfl_xor(acc[e], 1);
        acc[e] += __shfl_xor(acc[e], 2);
      }
      if (qq == 0 && nl < HG_TT) {
#pragma unroll
        for (int e = 0; e < HG_MAXE; ++e)
          if (e < E) {
            const float l = nl < nt ? (acc[e] + cs[e]) / div : -INFINITY;
            pl[nl * HG_MAXE + e] = l;
            if (nl < nt) lg[((long)b * N + n0 + nl) * E + e] = l;
          }
      }
    }
    __syncthreads();
    if (tid < E) {  // B: running max
      float m = mrun[tid];
      for (int n = 0; n < nt; ++n) m = fmaxf(m, pl[n * HG_MAXE + tid]);
      alpha[tid] = expf(mrun[tid] - m);  // exp(-inf) = 0 on the first sub-tile
      mrun[tid] = m;
    }
    __syncthreads();
    for (int i = tid; i < HG_TT * HG_MAXE; i += 256) {
      const int n = i / HG_MAXE, e = i % HG_MAXE;
      if (e < E) pl[i] = n < nt ? expf(pl[i] - mrun[e]) : 0.f;
    }
    __syncthreads();
    if (tid < E) {
      float s = srun[tid] * alpha[tid];
      for (int n = 0; n < nt; ++n) s += pl[n * HG_MAXE + tid];
      srun[tid] = s;
    }
    // C: h[e][d] = h * alpha + sum_n p[n][e] X[n][d]
#pragma unroll
    for (int e = 0; e < HG_MAXE; ++e)
      if (e < E) {
        h0[e] *= alpha[e];
        h1[e] *= alpha[e];
      }
    if (own0)
      for (int n = g; n < nt; n += G) {
        const T* xr = xb + (long)(n0 + n) * xcs;
        const float v0 = to_f(xr[dl]);
        const float v1 = own1 ? to_f(xr[dl + 256]) : 0.f;
#pragma unroll
        for (int e = 0; e < HG_MAXE; ++e)
          if (e < E) {
            const float p = pl[n * HG_MAXE + e];
            h0[e] = fmaf(p, v0, h0[e]);
            h1[e] = fmaf(p, v1, h1[e]);
          }
      }
    __syncthreads();
  }
  // token lanes -> one partial, fixed order
  float* out = ph + (((long)b * Tc + t) * E) * D;
  if (G > 1) {
    if (own0)
#pragma unroll
      for (int e = 0; e < HG_MAXE; ++e)
        if (e < E) red[(g * HG_MAXE + e) * cw + dl] = h0[e];
    __syncthreads();
    if (g == 0)
      for (int e = 0; e < E; ++e) {
        float s = red[e * cw + dl];
        for (int j = 1; j < G; ++j) s += red[(j * HG_MAXE + e) * cw + dl];
        out[(long)e * D + dl] = s;
      }
  } else if (own0) {
#pragma unroll
    for (int e = 0; e < HG_MAXE; ++e)
      if (e < E) {
        out[(long)e * D + dl] = h0[e];
        if (own1) out[(long)e * D + dl + 256] = h1[e];
      }
  }
  if (tid < E) {
    pm[((long)b * Tc + t) * E + tid] = mrun[tid];
    ps[((long)b * Tc + t) * E + tid] = srun[tid];
  }
}

// ---- 4: merge the chunk partials of (image, edge) -> He = A^T X -> He' = GELU(edge_proj(He)).  grid (E, B).
//   edge_wT: edge_proj.weight transposed, [D in][D out].
__global__ __launch_bounds__(256) void hg_edge_kernel(int D, int E, int Tc, const float* __restrict__ pm, const float* __restrict__ ps,
                                                      const float* __restrict__ ph, const float* __restrict__ ewT, const float* __restrict__ eb,
                                                      float* __restrict__ Mo, float* __restrict__ So, float* __restrict__ Heo) {
  __shared__ float He[HG_MAXD];
  const int e = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const float* pmb = pm + (long)b * Tc * E + e;
  const float* psb = ps + (long)b * Tc * E + e;
  float M = -INFINITY;
  for (int t = 0; t < Tc; ++t) M = fmaxf(M, pmb[(long)t * E]);
  float S = 0.f;
  for (int t = 0; t < Tc; ++t) S += psb[(long)t * E] * expf(pmb[(long)t * E] - M);
  for (int d = tid; d < D; d += 256) {
    float h = 0.f;
    for (int t = 0; t < Tc; ++t) h = fmaf(ph[(((long)b * Tc + t) * E + e) * D + d], expf(pmb[(long)t * E] - M), h);
    He[d] = h / S;
  }
  if (tid == 0) {
    Mo[(long)b * E + e] = M;
    So[(long)b * E + e] = S;
  }
  __syncthreads();
  for (int o = tid; o < D; o += 256) {
    float acc = 0.f;
    for (int d = 0; d < D; ++d) acc = fmaf(He[d], ewT[(long)d * D + o], acc);
    Heo[((long)b * E + e) * D + o] = hg_gelu(acc + eb[o]);
  }
}

// ---- 5: expansion.  grid (ceil(N / TT), B).  f16: TT = 32 tokens, node_proj on MFMA (node_w: f16 [D out][Kp], Kp = D rounded up to
// 32, zero tail); fp32: TT = 16 tokens, exact VALU (node_w: fp32 [D in][D out]).
template <typename T> struct HgExp;
template <> struct HgExp<f16> { static constexpr int TT = 32, ZP = 8; };
template <> struct HgExp<float> { static constexpr int TT = 16, ZP = 4; };

template <typename T>
__global__ __launch_bounds__(256) void hg_expand_kernel(int N, int D, int E, const T* __restrict__ x, int xcs, const float* __restrict__ lg,
                                                        const float* __restrict__ Mi, const float* __restrict__ Si, const float* __restrict__ Hei,
                                                        const void* __restrict__ node_w, const float* __restrict__ nb, T* __restrict__ y, int ycs) {
  constexpr int TT = HgExp<T>::TT;
  const int Kp = (D + 31) & ~31, zs = Kp + HgExp<T>::ZP;
  __shared__ float Hs[HG_MAXE * HG_MAXD];
  __shared__ float As[TT * HG_MAXE];
  __shared__ __attribute__((aligned(16))) T Z[TT * (((HG_MAXD + 31) & ~31) + HgExp<T>::ZP)];
  const int b = blockIdx.y, tid = threadIdx.x, n0 = blockIdx.x * TT;
  for (int i = tid; i < E * D; i += 256) Hs[i] = Hei[(long)b * E * D + i];
  for (int i = tid; i < TT * HG_MAXE; i += 256) {
    const int n = i / HG_MAXE, e = i % HG_MAXE;
    float a = 0.f;
    if (e < E && n0 + n < N) a = expf(lg[((long)b * N + n0 + n) * E + e] - Mi[(long)b * E + e]) / Si[(long)b * E + e];
    As[i] = a;
  }
  __syncthreads();
  for (int i = tid; i < TT * Kp; i += 256) {
    const int n = i / Kp, d = i % Kp;
    float z = 0.f;
    if (d < D)
      for (int e = 0; e < E; ++e) z = fmaf(As[n * HG_MAXE + e], Hs[e * D + d], z);
    Z[n * zs + d] = from_f<T>(z);
  }
  __syncthreads();
  const T* xb = x + (long)b * N * xcs;
  T* yb = y + (long)b * N * ycs;
  auto epi = [&](int n, int o, float acc) {
    if (n0 + n >= N) return;
    const float t = to_f(from_f<T>(acc + nb[o]));
    const float gl = to_f(from_f<T>(hg_gelu(t)));
    yb[(long)(n0 + n) * ycs + o] = from_f<T>(gl + to_f(xb[(long)(n0 + n) * xcs + o]));
  };
  if constexpr (sizeof(T) == 2) {
    // wave w: output column blocks ob = w, w + 4, ...; both 16-token row blocks; B fragments straight from global (L2)
    const int w = tid >> 6, l = tid & 63, r = l & 15, kh = (l >> 4) * 8;
    const f16* W = (const f16*)node_w;
    for (int ob = w; ob < D / 16; ob += 4) {
      f32x4 acc0 = (f32x4)0.f, acc1 = (f32x4)0.f;
      const f16* wr = W + (long)(ob * 16 + r) * Kp + kh;
      for (int k = 0; k < Kp; k += 32) {
        const f16x8 bf = *reinterpret_cast<const f16x8*>(wr + k);
        const f16x8 a0 = *reinterpret_cast<const f16x8*>(&Z[r * zs + k + kh]);
        const f16x8 a1 = *reinterpret_cast<const f16x8*>(&Z[(16 + r) * zs + k + kh]);
        acc0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(a0, bf, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(a1, bf, acc1, 0, 0, 0);
      }
      const int o = ob * 16 + r, rr = (l >> 4) * 4;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        epi(rr + i, o, acc0[i]);
        epi(16 + rr + i, o, acc1[i]);
      }
    }
  } else {
    const float* W = (const float*)node_w;
    for (int i = tid; i < TT * D; i += 256) {
      const int n = i / D, o = i % D;
      float acc = 0.f;
      for (int k = 0; k < D; ++k) acc = fmaf(Z[n * zs + k], W[(long)k * D + o], acc);
      epi(n, o, acc);
    }
  }
}

// byte windows of two channel-windowed NHWC views overlap (same-stride views with disjoint channel ranges do not)
bool hg_overlap(const void* a, int acs, const void* b, int bcs, long npix, int C, int es) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  const uintptr_t a1 = a0 + ((npix - 1) * acs + C) * (uintptr_t)es, b1 = b0 + ((npix - 1) * bcs + C) * (uintptr_t)es;
  if (a1 <= b0 || b1 <= a0) return false;
  if (acs != bcs) return true;
  const long diff = (long)(b0 > a0 ? b0 - a0 : a0 - b0);
  if (diff % es) return true;
  const long rel = (diff / es) % acs;
  return !(rel >= C && rel <= acs - C);
}

}  // namespace

extern "C" size_t ey_hypergraph_workspace_bytes(int B, int N, int D, int E) {
  if (B <= 0 || N <= 0 || D <= 0 || E <= 0) return 0;
  return hg_layout(nullptr, B, N, D, E).bytes;
}

extern "C" int ey_hypergraph_conv(int dtype, int B, int N, int D, int E, int heads, int context, const void* x, int x_cstride, void* y, int y_cstride,
                                  const float* proto_base, const float* ctx_wT, const float* ctx_b, const float* pre_w, const float* pre_b,
                                  const float* edge_wT, const float* edge_b, const void* node_w, const float* node_b, void* workspace,
                                  size_t workspace_bytes, ey_stream_t stream) {
  EY_CHECK(dtype == EY_F16 || dtype == EY_F32, "hypergraph_conv: bad dtype %d", dtype);
  EY_CHECK(B > 0 && N > 0, "hypergraph_conv: bad extent B=%d N=%d", B, N);
  EY_CHECK(D >= 16 && D <= HG_MAXD && D % 16 == 0, "hypergraph_conv: D=%d must be a multiple of 16 in [16, %d]", D, HG_MAXD);
  EY_CHECK(E >= 1 && E <= HG_MAXE, "hypergraph_conv: E=%d hyperedges, must be in [1, %d]", E, HG_MAXE);
  EY_CHECK(heads >= 1 && D % heads == 0, "hypergraph_conv: %d heads do not divide D=%d", heads, D);
  EY_CHECK(context >= 0 && context <= 2, "hypergraph_conv: context %d (0 both, 1 mean, 2 max)", context);
  EY_CHECK(x && y && proto_base && ctx_wT && ctx_b && pre_w && pre_b && edge_wT && edge_b && node_w && node_b && workspace,
           "hypergraph_conv: null pointer");
  EY_CHECK(x_cstride >= D && y_cstride >= D, "hypergraph_conv: channel stride below D");
  const int es = dtype == EY_F16 ? 2 : 4;
  EY_CHECK(!hg_overlap(x, x_cstride, y, y_cstride, (long)B * N, D, es), "hypergraph_conv: the x and y windows overlap");
  EY_CHECK(ey_aligned(workspace, 16), "hypergraph_conv: workspace must be 16-byte aligned");
  const HgWs ws = hg_layout((char*)workspace, B, N, D, E);
  EY_CHECK(workspace_bytes >= ws.bytes, "hypergraph_conv: workspace of %zu bytes, needs %zu (ey_hypergraph_workspace_bytes)", workspace_bytes, ws.bytes);
  if (dtype == EY_F16) EY_CHECK(ey_aligned(node_w, 16), "hypergraph_conv: f16 node_w must be 16-byte aligned");
  const int Ts = ey_cdiv(N, HG_STAT_CH), Tc = ey_cdiv(N, HG_CHUNK);
  const float div = sqrtf((float)(D / heads)) * (float)heads;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == EY_F16) {
    hipLaunchKernelGGL(hg_stats_kernel<f16>, dim3(Ts, B), dim3(256), 0, st, N, D, (const f16*)x, x_cstride, ws.st);
  } else {
    hipLaunchKernelGGL(hg_stats_kernel<float>, dim3(Ts, B), dim3(256), 0, st, N, D, (const float*)x, x_cstride, ws.st);
  }
  hipLaunchKernelGGL(hg_proto_kernel, dim3(E, B), dim3(256), 0, st, N, D, E, Ts, context, ws.st, proto_base, ctx_wT, ctx_b, pre_w, pre_b, ws.Q, ws.c);
  if (dtype == EY_F16) {
    hipLaunchKernelGGL(hg_softmax_kernel<f16>, dim3(Tc, B), dim3(256), 0, st, N, D, E, div, (const f16*)x, x_cstride, ws.Q, ws.c, ws.lg, ws.pm, ws.ps, ws.ph);
  } else {
    hipLaunchKernelGGL(hg_softmax_kernel<float>, dim3(Tc, B), dim3(256), 0, st, N, D, E, div, (const float*)x, x_cstride, ws.Q, ws.c, ws.lg, ws.pm, ws.ps,
                       ws.ph);
  }
  hipLaunchKernelGGL(hg_edge_kernel, dim3(E, B), dim3(256), 0, st, D, E, Tc, ws.pm, ws.ps, ws.ph, edge_wT, edge_b, ws.M, ws.S, ws.He);
  if (dtype == EY_F16) {
    hipLaunchKernelGGL(hg_expand_kernel<f16>, dim3(ey_cdiv(N, HgExp<f16>::TT), B), dim3(256), 0, st, N, D, E, (const f16*)x, x_cstride, ws.lg, ws.M, ws.S,
                       ws.He, node_w, node_b, (f16*)y, y_cstride);
  } else {
    hipLaunchKernelGGL(hg_expand_kernel<float>, dim3(ey_cdiv(N, HgExp<float>::TT), B), dim3(256), 0, st, N, D, E, (const float*)x, x_cstride, ws.lg, ws.M,
                       ws.S, ws.He, node_w, node_b, (float*)y, y_cstride);
  }
  EY_LAUNCH_CHECK("ey_hypergraph_conv");
  return EY_OK;
}

// ---- AvgPool2d(2) (floor) over NHWC windows: y[b,i,j,c] = (x[2i,2j] + x[2i,2j+1] + x[2i+1,2j] + x[2i+1,2j+1]) / 4, summed in fp32 in
// that order from +0 (the reference's CPU kernel), rounded once.
template <typename T>
__global__ __launch_bounds__(256) void avgpool2_kernel(long total, int H, int W, int Ho, int Wo, int C, const T* __restrict__ x, int xcs,
                                                       T* __restrict__ y, int ycs) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int c = (int)(idx % C);
  long p = idx / C;
  const int j = (int)(p % Wo);
  p /= Wo;
  const int i = (int)(p % Ho);
  const long b = p / Ho;
  const T* r0 = x + ((b * H + 2 * i) * W + 2 * j) * (long)xcs + c;
  const T* r1 = r0 + (long)W * xcs;
  float s = 0.f;
  s += to_f(r0[0]);
  s += to_f(r0[xcs]);
  s += to_f(r1[0]);
  s += to_f(r1[xcs]);
  y[((b * Ho + i) * Wo + j) * (long)ycs + c] = from_f<T>(s / 4.f);
}

extern "C" int ey_avgpool2(int dtype, int B, int H, int W, int C, const void* x, int x_cstride, void* y, int y_cstride, ey_stream_t stream) {
  EY_CHECK(x && y, "avgpool2: null pointer");
  EY_CHECK(dtype == EY_F16 || dtype == EY_F32, "avgpool2: bad dtype");
  EY_CHECK(B > 0 && H >= 2 && W >= 2 && C > 0 && x_cstride >= C && y_cstride >= C, "avgpool2: bad extent B=%d H=%d W=%d C=%d", B, H, W, C);
  const int Ho = H / 2, Wo = W / 2;
  const long total = (long)B * Ho * Wo * C;
  dim3 grid((unsigned)((total + 255) / 256));
  hipStream_t st = (hipStream_t)stream;
  if (dtype == EY_F16)
    hipLaunchKernelGGL(avgpool2_kernel<f16>, grid, dim3(256), 0, st, total, H, W, Ho, Wo, C, (const f16*)x, x_cstride, (f16*)y, y_cstride);
  else
    hipLaunchKernelGGL(avgpool2_kernel<float>, grid, dim3(256), 0, st, total, H, W, Ho, Wo, C, (const float*)x, x_cstride, (float*)y, y_cstride);
  EY_LAUNCH_CHECK("ey_avgpool2");
  return EY_OK;
}

// ---- Depthwise kxk, stride 2, pad k/2 (DSConv(c, c, k, 2).dw, reference conv.py:87-104): taps summed in fp32 in (ky, kx) order with
// fma, + bias, activation, rounded once.  w: [k][k][C] in the storage type.  Stride-1 depthwise stays on ey_dwconv.
template <typename T, int K>
__global__ __launch_bounds__(256) void dwconv_s2_kernel(long total, int H, int W, int Ho, int Wo, int C, int act, const T* __restrict__ x, int xcs,
                                                        const T* __restrict__ w, const float* __restrict__ bias, T* __restrict__ y, int ycs) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int c = (int)(idx % C);
  long p = idx / C;
  const int j = (int)(p % Wo);
  p /= Wo;
  const int i = (int)(p % Ho);
  const long b = p / Ho;
  float acc = 0.f;
#pragma unroll
  for (int ky = 0; ky < K; ++ky) {
    const int iy = 2 * i - K / 2 + ky;
    if (iy < 0 || iy >= H) continue;
#pragma unroll
    for (int kx = 0; kx < K; ++kx) {
      const int ix = 2 * j - K / 2 + kx;
      if (ix < 0 || ix >= W) continue;
      acc = fmaf(to_f(x[((b * H + iy) * W + ix) * (long)xcs + c]), to_f(w[(ky * K + kx) * C + c]), acc);
    }
  }
  if (bias) acc += bias[c];
  y[((b * Ho + i) * Wo + j) * (long)ycs + c] = from_f<T>(ey_act(acc, act));
}

template <typename T>
static void dwconv_s2_launch(int k, dim3 grid, hipStream_t st, long total, int H, int W, int Ho, int Wo, int C, int act, const void* x, int xcs, const void* w,
                             const float* bias, void* y, int ycs) {
  const T* xp = (const T*)x;
  const T* wp = (const T*)w;
  T* yp = (T*)y;
  if (k == 3) hipLaunchKernelGGL((dwconv_s2_kernel<T, 3>), grid, dim3(256), 0, st, total, H, W, Ho, Wo, C, act, xp, xcs, wp, bias, yp, ycs);
  else if (k == 5) hipLaunchKernelGGL((dwconv_s2_kernel<T, 5>), grid, dim3(256), 0, st, total, H, W, Ho, Wo, C, act, xp, xcs, wp, bias, yp, ycs);
  else hipLaunchKernelGGL((dwconv_s2_kernel<T, 7>), grid, dim3(256), 0, st, total, H, W, Ho, Wo, C, act, xp, xcs, wp, bias, yp, ycs);
}

extern "C" int ey_dwconv_s2(int dtype, int B, int H, int W, int C, int k, int act, const void* x, int x_cstride, const void* w_kkc, const float* bias,
                            void* y, int y_cstride, ey_stream_t stream) {
  EY_CHECK(x && w_kkc && y, "dwconv_s2: null pointer");
  EY_CHECK(dtype == EY_F16 || dtype == EY_F32, "dwconv_s2: bad dtype");
  EY_CHECK(k == 3 || k == 5 || k == 7, "dwconv_s2: k=%d (3, 5 or 7)", k);
  EY_CHECK(B > 0 && H > 0 && W > 0 && C > 0 && x_cstride >= C && y_cstride >= C, "dwconv_s2: bad extent");
  const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;  // (H + 2*(k/2) - k) / 2 + 1
  const long total = (long)B * Ho * Wo * C;
  dim3 grid((unsigned)((total + 255) / 256));
  hipStream_t st = (hipStream_t)stream;
  if (dtype == EY_F16) dwconv_s2_launch<f16>(k, grid, st, total, H, W, Ho, Wo, C, act, x, x_cstride, w_kkc, bias, y, y_cstride);
  else dwconv_s2_launch<float>(k, grid, st, total, H, W, Ho, Wo, C, act, x, x_cstride, w_kkc, bias, y, y_cstride);
  EY_LAUNCH_CHECK("ey_dwconv_s2");
  return EY_OK;
}
