// SCDown as ONE kernel (f16): the pointwise 1x1 conv + activation and the depthwise 3x3 stride-2 conv behind it,
//     y = act2( DWConv3x3s2_{pad 1}( round_f16( act1( Conv1x1_{C1->C2}(x) + b1 ) ) ) + b2 )
// = SCDown(c1, c2, 3, 2) of YOLOv10 (reference block.py:1174-1206: cv1 = Conv(c1, c2, 1, 1), cv2 = Conv(c2, c2, 3, 2, g=c2, act=False)) --
// layers 5, 7 and 20 of the yolov10 graphs.  The (B, C2, H, W) map between the two convs is the largest tensor the layer touches and has
// one consumer; as two launches (ey_conv2d + ey_dwconv_s2) it is written to memory and read straight back.  Here it lives in LDS only.
//
// What was chosen, and why:
//   * Work item = (tile of 8 x 8 output pixels, slab of 64 mid channels).  The tile's windows touch 17 x 17 mid pixels (1.13x the 16 x 16 a
//     stride-2 tile owns: the halo is recomputed, not exchanged); 289 pixels x 64 channels of f16 at a pixel pitch of 144 B are 41.6 KB.
//     64 channels = four 16-row blocks of the packed weight matrix: with the row permutation of ey_conv_pack_weight a lane then owns 16
//     consecutive mid channels of its pixel (two 16-byte LDS stores), and the slab's 64 weight rows are one contiguous block in memory.
//     A slab never straddles a block tile of the packing, so C2 must be a multiple of 64 and pack with NT = 4 or 8 (every yolov10 width).
//     The input tile is read once per slab (C2 / 64 times in all): those re-reads come from L2 / Infinity Cache, every slab walks the
//     tiles in the same order at the same time.  Holding all of C2 in LDS instead would fit 128 channels only.
//   * 256 threads = 4 waves; grid = (tiles walked with a stride, C2 / 64).  A workgroup stages its slab's 64 x C1 weights into LDS once
//     (row pitch 32 KS + 16 halves = 2 (mod 4) 16-byte units: conflict-free fragment reads, common.h) and keeps them for all its tiles:
//     C1 = 640 needs 84 KB + 41.6 KB + 1.2 KB = 126.7 KB (one workgroup per CU), C1 = 64 needs 53.0 KB (three per CU).
//   * phase 1 (MFMA): a wave takes every fourth block of 16 mid pixels; per 32-channel k-step one range-checked 16-byte buffer load per lane
//     (pixels outside the map and channel tails read zeros; the first four k-steps of a block are requested one block ahead), four A fragments from LDS, four v_mfma_f32_16x16x32_f16 -- the k-steps of the
//     stand-alone pointwise kernels (A = weights, B = pixels, ascending k, lane group g = channels 32 t + 8 g ...), so the fp32 sums have
//     the same bits; + bias, activation (SiLU as an fp32 value of its own, ey_silu_rn), rounded to f16 into the LDS tile.
//   * phase 2 (VALU): a thread owns 8 channels (the bias stays in registers, the slab's nine 16-byte weight vectors per channel group in LDS:
//     in registers they cost 36 VGPRs through phase 1) of two output pixels; taps in (ky, kx) order, fp32 fma, taps outside the map skipped -- dwconv_s2_kernel's arithmetic (hypergraph.hip) -- then
//     + bias, activation, one rounding, one 16-byte NHWC store into the caller's channel window.
//   * no atomics, no workspace, nothing data-dependent in the launch: deterministic and capturable.
// k = 5 / 7 are refused: a 21 x 21 mid tile for 8 x 8 outputs (halo 1.7x) wants another tile shape, i.e. another kernel, not a template argument.
// act2 = SiLU / Sigmoid are refused too (SCDown has none): the stand-alone kernel leaves the fusing of that multiply into the rounding to the
// compiler, so its bits are not pinned.
// Compiler resource remarks (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage): 114 VGPRs + 16 AGPRs, no scratch,
// no spills, 3 waves per SIMD (= 3 workgroups per CU, which is also what the LDS of the narrow layers allows); LDS is dynamic only:
// (64 x (32 ceil(C1 / 32) + 16) + 289 x 72 + 9 x 64) x 2 bytes = 53.0 KB at C1 = 64, 61.2 KB at 128, 77.6 KB at 256, 126.7 KB at 640.
#include "common.h"
#include "tune.h"

#define SCD_TH 8
#define SCD_TW 8
#define SCD_CP 72  // mid-tile pixel pitch (halves): 144 B

struct ScdP {
  int B, H, W, Ho, Wo, C1, C2, KS;
  const void* x; int xcs; unsigned xbytes;
  const void* w1; int Kpad; const float* b1; int act1;
  const void* w2; const float* b2; int act2;
  void* y; int ycs;
  int NT, LW, tilesX, tilesY, ntile;
};

__global__ __launch_bounds__(256) void scdown_kernel(ScdP p) {
  typedef f16 T;
  constexpr int SR = 2 * SCD_TH + 1, SW = 2 * SCD_TW + 1, NS = SR * SW, NB = (NS + 15) / 16, CP = SCD_CP;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  T* s_w = reinterpret_cast<T*>(smem);  // [64][LW]
  T* s_mid = s_w + 64 * p.LW;           // [NS][CP]
  T* s_w2 = s_mid + NS * CP;            // [9][64]: the slab's depthwise weights in slab channel order
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, g = lane >> 4;
  // this workgroup's slab: 16-row blocks nt0 .. nt0 + 3 of block tile nb of the packed weights (ey_conv_pack_weight: row 16 nt + 4 g + j of
  // block tile nb <-> channel nb * 16 NT + g * 4 NT + 4 nt + j)
  const int spb = p.NT >> 2, nb = blockIdx.y / spb, nt0 = (blockIdx.y - nb * spb) * 4;
  const int LW = p.LW, KS = p.KS;
  {
    const T* wr = (const T*)p.w1 + (long)(nb * 16 * p.NT + nt0 * 16) * p.Kpad;
    const int KV = KS * 4;
    for (int v = tid; v < 64 * KV; v += 256) {
      const int row = v / KV, kv = v - row * KV;
      Vec8<T> w;
      w.load(wr + (long)row * p.Kpad + kv * 8);
      w.store(s_w + row * LW + kv * 8);
    }
  }
  // phase 1: lane (r, g) ends with slab channels 16 g .. 16 g + 15 of its pixel = channels ch1 ...
  const int ch1 = nb * 16 * p.NT + g * 4 * p.NT + 4 * nt0;
  float bias1[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) bias1[i] = p.b1[ch1 + i];
  // phase 2: slab channels 8 cv .. 8 cv + 7 = channels ch2 ...
  const int cv = tid & 7, ch2 = nb * 16 * p.NT + (cv >> 1) * 4 * p.NT + 4 * nt0 + (cv & 1) * 8;
  if (tid < 72) {  // 9 taps x 8 vectors: vector v of a tap = slab channels 8 v ..
    const int tap = tid >> 3, v = tid & 7;
    Vec8<T> w;
    w.load((const T*)p.w2 + tap * p.C2 + nb * 16 * p.NT + (v >> 1) * 4 * p.NT + 4 * nt0 + (v & 1) * 8);
    w.store(s_w2 + tap * 64 + 8 * v);
  }
  float bias2[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) bias2[i] = p.b2 ? p.b2[ch2 + i] : 0.f;
  const __amdgpu_buffer_rsrc_t rs = ey_rsrc(p.x, p.xbytes);
  const int tiles_img = p.tilesX * p.tilesY;
  __syncthreads();  // weights staged
  for (int tile = blockIdx.x; tile < p.ntile; tile += gridDim.x) {
    const int b = tile / tiles_img, trem = tile - b * tiles_img;
    const int oy0 = (trem / p.tilesX) * SCD_TH, ox0 = (trem % p.tilesX) * SCD_TW;
    // ---- phase 1: the 1x1 conv on the 17 x 17 mid pixels of the tile -> LDS
    // the B fragments of a block's first four k-steps are requested one block ahead: they fly through the MFMAs, the SiLUs and the LDS
    // stores of the block before (a wave's blocks would otherwise each wait out a full memory round trip)
    auto block_off = [&](int blk) -> unsigned {
      const int pi = blk * 16 + r, pc = pi < NS ? pi : NS - 1;
      const int t = pc / SW, u = pc - t * SW;
      const int my = 2 * oy0 - 1 + t, mx = 2 * ox0 - 1 + u;
      const bool in = my >= 0 && my < p.H && mx >= 0 && mx < p.W;
      return in ? (unsigned)((((b * p.H + my) * p.W + mx) * p.xcs + 8 * g) * 2) : EY_OOB;
    };
    auto request = [&](Vec8<T> (&bf)[4], unsigned voff, int t0) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int ks = t0 + q;
        if (ks < KS) BufLoad8<T>::load(bf[q], rs, (ks * 32 + 8 * g < p.C1) ? voff : EY_OOB, ks * 64);  // (ks: wave-uniform)
      }
    };
    Vec8<T> bnext[4];
    unsigned voff_next = block_off(wave);
    request(bnext, voff_next, 0);
    for (int blk = wave; blk < NB; blk += 4) {
      const int pi = blk * 16 + r;
      const unsigned voff = voff_next;
      f32x4 acc[4];
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) acc[nt] = (f32x4)0.f;
      const T* ap = s_w + r * LW + 8 * g;
      for (int t0 = 0; t0 < KS; t0 += 4) {
        Vec8<T> bf[4];
        if (t0 == 0) {
#pragma unroll
          for (int q = 0; q < 4; ++q) bf[q] = bnext[q];
          if (blk + 4 < NB) {  // (wave-uniform)
            voff_next = block_off(blk + 4);
            request(bnext, voff_next, 0);
          }
        } else {
          request(bf, voff, t0);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int ks = t0 + q;
          if (ks < KS) {
            Vec8<T> af[4];
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) af[nt].load(ap + nt * 16 * LW + ks * 32);
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[nt].v, bf[q].v, acc[nt], 0, 0, 0);
          }
        }
      }
      float v[16];
#pragma unroll
      for (int nt = 0; nt < 4; ++nt)
#pragma unroll
        for (int j = 0; j < 4; ++j) v[4 * nt + j] = acc[nt][j] + bias1[4 * nt + j];
      if (p.act1 == EY_ACT_SILU) {
#pragma unroll
        for (int i = 0; i < 16; ++i) v[i] = ey_silu_rn(v[i]);
      } else if (p.act1 == EY_ACT_RELU) {
#pragma unroll
        for (int i = 0; i < 16; ++i) v[i] = fmaxf(v[i], 0.f);
      }
      if (pi < NS) {
        T* d = s_mid + pi * CP + 16 * g;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          Vec8<T> o;
#pragma unroll
          for (int j = 0; j < 8; ++j) o.set(j, v[8 * h + j]);
          o.store(d + 8 * h);
        }
      }
    }
    ey_lds_barrier();
    // ---- phase 2: depthwise 3x3 stride 2 from the LDS tile; mid pixels outside the map are never read
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const int opx = (tid >> 3) + 32 * it, oyl = opx / SCD_TW, oxl = opx - oyl * SCD_TW;
      const int oy = oy0 + oyl, ox = ox0 + oxl;
      if (oy < p.Ho && ox < p.Wo) {
        float a[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) a[i] = 0.f;
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
          const int iy = 2 * oy - 1 + ky;
          if (iy < 0 || iy >= p.H) continue;
#pragma unroll
          for (int kx = 0; kx < 3; ++kx) {
            const int ix = 2 * ox - 1 + kx;
            if (ix < 0 || ix >= p.W) continue;
            Vec8<T> m, wk;
            m.load(s_mid + ((2 * oyl + ky) * SW + 2 * oxl + kx) * CP + 8 * cv);
            wk.load(s_w2 + (ky * 3 + kx) * 64 + 8 * cv);
            ey_fma8_mix(m, wk, a);
          }
        }
        if (p.b2) {
#pragma unroll
          for (int i = 0; i < 8; ++i) a[i] += bias2[i];
        }
        if (p.act2 == EY_ACT_RELU) {
#pragma unroll
          for (int i = 0; i < 8; ++i) a[i] = fmaxf(a[i], 0.f);
        }
        Vec8<T> o;
#pragma unroll
        for (int i = 0; i < 8; ++i) o.set(i, a[i]);
        o.store((T*)p.y + (((long)b * p.Ho + oy) * p.Wo + ox) * p.ycs + ch2);
      }
    }
    ey_lds_barrier();  // phase 2 reads of the tile are done before the next phase 1 overwrites it
  }
}

extern "C" int ey_scdown(int dtype, int B, int H, int W, int C1, int C2, int k, const void* x, int x_cstride, const void* w1_packed, const float* bias1, int act1,
                         const void* w2_kkc, const float* bias2, int act2, void* y, int y_cstride, ey_stream_t stream) {
  EY_CHECK(x && w1_packed && w2_kkc && y, "scdown: null pointer");
  EY_CHECK(B > 0 && H > 0 && W > 0 && C1 > 0 && C2 > 0, "scdown: bad extent");
  EY_CHECK(x_cstride >= C1 && y_cstride >= C2, "scdown: cstride");
  const long px = (long)B * H * W;
  const long xbytes = ((px - 1) * x_cstride + C1) * 2;
  const int KS = (C1 + 31) / 32, LW = KS * 32 + 16;
  const size_t lds = ((size_t)64 * LW + (size_t)(2 * SCD_TH + 1) * (2 * SCD_TW + 1) * SCD_CP + 9 * 64) * 2;
  const int NT = ey_conv_pack_nt(C2);
  const bool fits = tune().scdown && dtype == EY_F16 && k == 3 && C1 % 8 == 0 && C2 % 64 == 0 && (NT == 4 || NT == 8) && lds <= 160 * 1024 && bias1 &&
                    (act1 == EY_ACT_NONE || act1 == EY_ACT_RELU || act1 == EY_ACT_SILU) && (act2 == EY_ACT_NONE || act2 == EY_ACT_RELU) &&
                    px >= tune().scdown_min_px && xbytes < (1L << 31) && (x_cstride * 2) % 16 == 0 && (y_cstride * 2) % 16 == 0 && ey_aligned(x, 16) && ey_aligned(y, 16) &&
                    ey_aligned(w1_packed, 16) && ey_aligned(w2_kkc, 16);
  if (!fits)
    return ey_set_error(EY_EUNSUPPORTED, "scdown: outside the fused kernel (f16, k = 3, C1 %% 8 == 0, C2 %% 64 == 0, bias1, act2 none / ReLU, 16-byte aligned views)");
  ScdP p;
  p.B = B; p.H = H; p.W = W; p.Ho = (H - 1) / 2 + 1; p.Wo = (W - 1) / 2 + 1; p.C1 = C1; p.C2 = C2; p.KS = KS;
  p.x = x; p.xcs = x_cstride; p.xbytes = (unsigned)xbytes;
  p.w1 = w1_packed; p.Kpad = ey_conv_kpad(C1, 2); p.b1 = bias1; p.act1 = act1;
  p.w2 = w2_kkc; p.b2 = bias2; p.act2 = act2;
  p.y = y; p.ycs = y_cstride;
  p.NT = NT; p.LW = LW;
  p.tilesX = (p.Wo + SCD_TW - 1) / SCD_TW; p.tilesY = (p.Ho + SCD_TH - 1) / SCD_TH;
  const long ntile = (long)B * p.tilesX * p.tilesY;
  if (ntile >= (1L << 30)) return ey_set_error(EY_EUNSUPPORTED, "scdown: too many tiles");
  p.ntile = (int)ntile;
  static int ncu = 0;
  if (!ncu) {
    int dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) ncu = prop.multiProcessorCount;
    if (ncu < 1) ncu = 256;
  }
  if (!ey_lds_reserve<scdown_kernel>(lds)) return ey_set_error(EY_ELAUNCH, "scdown: cannot reserve %zu B of LDS", lds);
  const int nslab = C2 / 64;
  long occ = (160 * 1024) / (long)lds;  // workgroups of a CU by LDS (256 threads: registers allow 4 and more)
  if (occ > 4) occ = 4;
  long gx = (occ * ncu + nslab - 1) / nslab;  // resident slots shared by the slabs; every workgroup stages its weights once
  if (gx > ntile) gx = ntile;
  if (gx < 1) gx = 1;
  hipLaunchKernelGGL(scdown_kernel, dim3((unsigned)gx, (unsigned)nslab), dim3(256), lds, (hipStream_t)stream, p);
  EY_LAUNCH_CHECK("ey_scdown");
  return EY_OK;
}
