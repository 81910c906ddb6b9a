// GhostConv(c1, c2, 1, 1) as ONE kernel (f16): the pointwise 1x1 conv, the depthwise 5x5 "cheap operation" behind it, the channel concat of
// the two and -- for the closing GhostConv of a GhostBottleneck -- the block's residual add,
//     y1 = round_f16( act( Conv1x1_{C1->Ch}(x) + b1 ) ),   y2 = round_f16( act( DW5x5_{s1, pad 2}(y1) + b2 ) ),   out = cat(y1, y2) [+ res]
// (reference conv.py:180-193, block.py:446-464).  As separate launches the closing GhostConv of a bottleneck is ey_conv2d into a scratch map,
// ey_dwconv and an elementwise add over the whole map -- the residual cannot ride in the 1x1's epilogue, the depthwise stage reads y1
// before x is added --: 5.0 passes over a 2 Ch-channel map against 2.5 here, and three launches against one.
//
// What was chosen, and why:
//   * Work item = (tile of TH x TW output pixels, slab of SB 16-row blocks of the packed weight matrix).  The depthwise stage is per channel,
//     so slabs are independent.  A 16-row block (block tile nb, n-block nt of ey_conv_pack_weight) holds the channels nb 16 NT + g 4 NT + 4 nt + j
//     (g, j = 0..3): four runs of FOUR consecutive channels, whatever NT the width was packed with (1, 2, 4, 5 or 8).  The whole kernel
//     therefore works in 4-channel groups -- 8-byte LDS accesses and 8-byte global loads / stores -- which is also what a hidden width of
//     4, 12, 20 ... (Ch % 8 == 4: every ghost model at the n, m and x scales) needs: the second half of the output pixel then starts at an
//     8-byte boundary only.  One path serves every width; there is no 16-byte special case to keep in step.
//   * SB = 1, 2, 4 (template): Ch <= 16 -> one block, <= 32 -> two, else four (64 channels, as ey_scdown) -- halved while tiles x slabs stay
//     below two workgroups per CU (measured at batch 32: 256 -> 2 x 64 on 20 x 20 is 128 tiles, half the chip with one 64-channel slab;
//     the bits do not depend on SB; the tunable ghost_sb = 1 / 2 / 4 caps the width instead of this rule).  The last slab of a width whose
//     block count is no multiple of SB (NT = 5: 72, 80, 160, 320) has empty blocks: their weight rows are staged as zeros, their channel
//     numbers lie beyond Ch and are never stored.
//   * The tile is at most 16 x 16 and balanced on the host: TH = ceil(H / ceil(H / 16)), so a 20 x 20 map is cut into four 10 x 10 tiles
//     (14 x 14 mid pixels each, 1.96x recompute) and not into four 16 x 16 tiles of which 61 % would be empty; an 80 x 80 or 160 x 160 map
//     gets 16 x 16 tiles (20 x 20 mid pixels, 1.56x).  The mid tile lives in LDS as f16 at a pixel pitch of 16 SB + 4 halves.
//   * 256 threads = 4 waves; grid = (tiles walked with a stride, slabs).  A workgroup stages its slab's 16 SB x C1 weights into LDS once (row
//     pitch 32 KS + 16 halves = 2 (mod 4) 16-byte units: conflict-free fragment reads, common.h) and keeps them for all its tiles.
//   * phase 1 (MFMA) is ey_scdown's: a wave takes every fourth block of 16 mid pixels; per 32-channel k-step one range-checked 16-byte buffer
//     load per lane (pixels outside the map and channel tails read zeros; the first four k-steps of a block are requested one block ahead),
//     SB A fragments from LDS, SB v_mfma_f32_16x16x32_f16 -- the k-steps of the stand-alone pointwise kernels (A = weights, B = pixels,
//     ascending k), so the fp32 sums have the same bits; + bias, activation (SiLU as an fp32 value of its own, ey_silu_rn), rounded to f16.
//   * phase 2 (VALU): a work item is (output pixel, 4-channel group), groups fastest: neighbouring lanes read neighbouring 8 bytes of LDS.
//     dwconv_kernel<f16, 5>'s arithmetic (ops_misc.hip): the sum starts from the bias, taps in (ky, kx) order, fp32 fma, taps outside the
//     map skipped, then the activation and one rounding; the bias and the channel numbers of a thread's group stay in registers.  y1 is
//     the centre pixel of the LDS tile.  With res, both halves are round_f16(f32(y) + f32(res)) -- an f16 add as torch does it -- so out
//     may be res itself (the in-place chain of C3Ghost).
//   * no atomics, no workspace, nothing data-dependent in the launch: deterministic and capturable.
// LDS (dynamic only): (16 SB x (32 ceil(C1 / 32) + 16) + NS x (16 SB + 4) + 25 x 16 SB) x 2 bytes, NS = (TH + 4)(TW + 4) <= 400:
//   Ch = 4, C1 = 16 (SB 1):  1.5 + 15.6 + 0.8 = 17.9 KB        Ch = 32, C1 = 64 (SB 2): 5.0 + 28.1 + 1.6 = 34.7 KB
//   Ch = 64, C1 = 128 (SB 4): 18.0 + 53.1 + 3.1 = 74.2 KB      Ch = 320, C1 = 640 (SB 4): 82.0 + 53.1 + 3.1 = 138.2 KB
// C1 above 832 does not fit next to a full tile and is refused.
// Compiler resource remarks (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage), no scratch and no spills in any of them:
//   SB = 1:  74 VGPRs +  4 AGPRs, 101 SGPRs, 6 waves per SIMD        SB = 2:  86 VGPRs +  8 AGPRs, 102 SGPRs, 5 waves per SIMD
//   SB = 4: 108 VGPRs + 16 AGPRs, 104 SGPRs, 4 waves per SIMD (the LDS of its layers allows two workgroups per CU at most)
#include "common.h"
#include "tune.h"

#define GH_TMAX 16  // largest tile edge (output pixels)
#define GH_HALO 2

struct GhP {
  int B, H, W, C1, Ch, KS;
  const void* x; int xcs; unsigned xbytes;
  const void* w1; int Kpad; const float* b1;
  const void* w2; const float* b2; int act;
  const void* res; int rcs;
  void* y; int ycs;
  int NT, nrb, LW, TH, TW, tilesX, tilesY, ntile;
};

// first channel of the run of four that row 4 g .. 4 g + 3 of 16-row block rb of the packed weights holds (ey_conv_pack_weight)
__device__ __forceinline__ int gh_chan(int rb, int g, int NT) {
  const int nb = rb / NT, nt = rb - nb * NT;
  return nb * 16 * NT + g * 4 * NT + 4 * nt;
}

template <int SB>
__global__ __launch_bounds__(256) void ghost_conv_kernel(GhP p) {
  typedef f16 T;
  constexpr int CS = 16 * SB, CP = CS + 4, NG = 4 * SB;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int SH = p.TH + 2 * GH_HALO, SW = p.TW + 2 * GH_HALO, NS = SH * SW, NB = (NS + 15) >> 4;
  const int LW = p.LW, KS = p.KS;
  T* s_w = reinterpret_cast<T*>(smem);                  // [CS][LW]
  T* s_mid = s_w + CS * LW;                             // [NS][CP]
  T* s_w2 = s_mid + NS * CP;                            // [25][CS]: the slab's depthwise weights in slab order
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, g = lane >> 4;
  const int rb0 = blockIdx.y * SB;
  {
    const T* wr = (const T*)p.w1 + (long)rb0 * 16 * p.Kpad;
    const int KV = KS * 4, rows = (p.nrb - rb0 < SB ? p.nrb - rb0 : SB) * 16;
    for (int v = tid; v < CS * KV; v += 256) {
      const int row = v / KV, kv = v - row * KV;
      Vec8<T> w;
      if (row < rows) w.load(wr + (long)row * p.Kpad + kv * 8);
      else w.zero();
      w.store(s_w + row * LW + kv * 8);
    }
  }
  for (int v = tid; v < 25 * NG; v += 256) {  // slab order: local channel 16 blk + 4 g + j
    const int tap = v / NG, q = v - tap * NG;
    const int ch = gh_chan(rb0 + (q >> 2), q & 3, p.NT);
    f16x4 w = (f16x4)(f16)0;
    if (ch < p.Ch) w = *reinterpret_cast<const f16x4*>((const T*)p.w2 + tap * p.Ch + ch);
    *reinterpret_cast<f16x4*>(s_w2 + tap * CS + 4 * q) = w;
  }
  // phase 2: the items of a thread are 256 apart and NG divides 256, so a thread keeps ONE channel group: slab group q2 = channels ch2 ...
  const int q2 = tid & (NG - 1), ch2 = gh_chan(rb0 + (q2 >> 2), q2 & 3, p.NT);
  float bias2[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) bias2[i] = (p.b2 && ch2 < p.Ch) ? p.b2[ch2 + i] : 0.f;
  // phase 1: lane (r, g) ends with rows 4 g .. 4 g + 3 of each of the slab's blocks for its pixel
  float bias1[SB][4];
#pragma unroll
  for (int nt = 0; nt < SB; ++nt) {
    const int ch = gh_chan(rb0 + nt, g, p.NT);
#pragma unroll
    for (int j = 0; j < 4; ++j) bias1[nt][j] = (p.b1 && ch + j < p.Ch) ? p.b1[ch + j] : 0.f;
  }
  const __amdgpu_buffer_rsrc_t rs = ey_rsrc(p.x, p.xbytes);
  const int tiles_img = p.tilesX * p.tilesY;
  __syncthreads();  // weights staged
  for (int tile = blockIdx.x; tile < p.ntile; tile += gridDim.x) {
    const int b = tile / tiles_img, trem = tile - b * tiles_img;
    const int oy0 = (trem / p.tilesX) * p.TH, ox0 = (trem % p.tilesX) * p.TW;
    // ---- phase 1: the 1x1 conv on the (TH + 4) x (TW + 4) mid pixels of the tile -> LDS
    auto block_off = [&](int blk) -> unsigned {
      const int pi = blk * 16 + r, pc = pi < NS ? pi : NS - 1;
      const int t = pc / SW, u = pc - t * SW;
      const int my = oy0 - GH_HALO + t, mx = ox0 - GH_HALO + u;
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
    if (wave < NB) request(bnext, voff_next, 0);
    for (int blk = wave; blk < NB; blk += 4) {
      const int pi = blk * 16 + r;
      const unsigned voff = voff_next;
      f32x4 acc[SB];
#pragma unroll
      for (int nt = 0; nt < SB; ++nt) acc[nt] = (f32x4)0.f;
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
            Vec8<T> af[SB];
#pragma unroll
            for (int nt = 0; nt < SB; ++nt) af[nt].load(ap + nt * 16 * LW + ks * 32);
#pragma unroll
            for (int nt = 0; nt < SB; ++nt) acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[nt].v, bf[q].v, acc[nt], 0, 0, 0);
          }
        }
      }
      float v[SB][4];
#pragma unroll
      for (int nt = 0; nt < SB; ++nt)
#pragma unroll
        for (int j = 0; j < 4; ++j) v[nt][j] = acc[nt][j] + bias1[nt][j];
      if (p.act == EY_ACT_SILU) {
#pragma unroll
        for (int nt = 0; nt < SB; ++nt)
#pragma unroll
          for (int j = 0; j < 4; ++j) v[nt][j] = ey_silu_rn(v[nt][j]);
      } else if (p.act == EY_ACT_RELU) {
#pragma unroll
        for (int nt = 0; nt < SB; ++nt)
#pragma unroll
          for (int j = 0; j < 4; ++j) v[nt][j] = fmaxf(v[nt][j], 0.f);
      }
      if (pi < NS) {
        T* d = s_mid + pi * CP + 4 * g;
#pragma unroll
        for (int nt = 0; nt < SB; ++nt) {
          f16x4 o;
#pragma unroll
          for (int j = 0; j < 4; ++j) o[j] = (f16)v[nt][j];
          *reinterpret_cast<f16x4*>(d + 16 * nt) = o;
        }
      }
    }
    ey_lds_barrier();
    // ---- phase 2: depthwise 5x5 from the LDS tile; mid pixels outside the map are never read
    const int npx = p.TH * p.TW;
    for (int px = tid / NG; px < npx; px += 256 / NG) {
      const int q = q2, ch = ch2;
      const int oyl = px / p.TW, oxl = px - oyl * p.TW;
      const int oy = oy0 + oyl, ox = ox0 + oxl;
      if (oy < p.H && ox < p.W && ch < p.Ch) {
        float a[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) a[i] = bias2[i];
#pragma unroll
        for (int ky = 0; ky < 5; ++ky) {
          const int iy = oy - 2 + ky;
          if (iy < 0 || iy >= p.H) continue;
#pragma unroll
          for (int kx = 0; kx < 5; ++kx) {
            const int ix = ox - 2 + kx;
            if (ix < 0 || ix >= p.W) continue;
            const f16x4 m = *reinterpret_cast<const f16x4*>(s_mid + ((oyl + ky) * SW + oxl + kx) * CP + 4 * q);
            const f16x4 wk = *reinterpret_cast<const f16x4*>(s_w2 + (ky * 5 + kx) * CS + 4 * q);
#pragma unroll
            for (int i = 0; i < 4; ++i) a[i] += (float)m[i] * (float)wk[i];
          }
        }
        ey_act_n(a, p.act);
        f16x4 y2;
#pragma unroll
        for (int i = 0; i < 4; ++i) y2[i] = (f16)a[i];
        f16x4 y1 = *reinterpret_cast<const f16x4*>(s_mid + ((oyl + GH_HALO) * SW + oxl + GH_HALO) * CP + 4 * q);
        const long pix = ((long)b * p.H + oy) * p.W + ox;
        if (p.res) {
          const T* rp = (const T*)p.res + pix * p.rcs + ch;
          const f16x4 r1 = *reinterpret_cast<const f16x4*>(rp), r2 = *reinterpret_cast<const f16x4*>(rp + p.Ch);
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            y1[i] = (f16)((float)y1[i] + (float)r1[i]);
            y2[i] = (f16)((float)y2[i] + (float)r2[i]);
          }
        }
        T* yp = (T*)p.y + pix * p.ycs + ch;
        *reinterpret_cast<f16x4*>(yp) = y1;
        *reinterpret_cast<f16x4*>(yp + p.Ch) = y2;
      }
    }
    ey_lds_barrier();  // phase 2 reads of the tile are done before the next phase 1 overwrites it
  }
}

static int ghost_ncu() {
  static int ncu = 0;
  if (!ncu) {
    int dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) ncu = prop.multiProcessorCount;
    if (ncu < 1) ncu = 256;
  }
  return ncu;
}

template <int SB>
static int ghost_launch(const GhP& p, size_t lds, int nslab, hipStream_t st) {
  const int ncu = ghost_ncu();
  if (!ey_lds_reserve<ghost_conv_kernel<SB>>(lds)) return ey_set_error(EY_ELAUNCH, "ghost_conv: cannot reserve %zu B of LDS", lds);
  long occ = (160 * 1024) / (long)lds;  // workgroups of a CU by LDS (256 threads: registers allow 4 and more)
  if (occ > 8) occ = 8;
  if (occ < 1) occ = 1;
  long gx = (occ * ncu + nslab - 1) / nslab;  // resident slots shared by the slabs; every workgroup stages its weights once
  if (gx > p.ntile) gx = p.ntile;
  if (gx < 1) gx = 1;
  hipLaunchKernelGGL(ghost_conv_kernel<SB>, dim3((unsigned)gx, (unsigned)nslab), dim3(256), lds, st, p);
  EY_LAUNCH_CHECK("ey_ghost_conv");
  return EY_OK;
}

extern "C" int ey_ghost_conv(int dtype, int B, int H, int W, int C1, int Ch, int k, const void* x, int x_cstride, const void* w1_packed, const float* bias1,
                             const void* w2_kkc, const float* bias2, int act, const void* res, int res_cstride, void* y, int y_cstride, ey_stream_t stream) {
  EY_CHECK(x && w1_packed && w2_kkc && y, "ghost_conv: null pointer");
  EY_CHECK(B > 0 && H > 0 && W > 0 && C1 > 0 && Ch > 0, "ghost_conv: bad extent");
  EY_CHECK(x_cstride >= C1 && y_cstride >= 2 * Ch && (!res || res_cstride >= 2 * Ch), "ghost_conv: cstride");
  const long px = (long)B * H * W;
  const long xbytes = ((px - 1) * x_cstride + C1) * 2;
  const int KS = (C1 + 31) / 32, LW = KS * 32 + 16;
  const int NT = ey_conv_pack_nt(Ch), nrb = (Ch + 16 * NT - 1) / (16 * NT) * NT;
  const int TH = (H + (H + GH_TMAX - 1) / GH_TMAX - 1) / ((H + GH_TMAX - 1) / GH_TMAX), TW = (W + (W + GH_TMAX - 1) / GH_TMAX - 1) / ((W + GH_TMAX - 1) / GH_TMAX);
  // slab width: the widest that still leaves two workgroups per CU (a 20 x 20 map at batch 32 is 128 tiles: with 64-channel slabs a 64-wide
  // layer would occupy half the chip); narrower slabs re-read the input tile, from L2.  ghost_sb = 1, 2, 4 caps the width instead (sweeps, tests)
  const long ntile0 = (long)B * ((H + TH - 1) / TH) * ((W + TW - 1) / TW);
  int SB = Ch <= 16 ? 1 : Ch <= 32 ? 2 : 4;
  const long sbt = tune().ghost_sb;
  if (sbt == 1 || sbt == 2 || sbt == 4) {
    while (SB > sbt) SB >>= 1;
  } else {
    while (SB > 1 && ntile0 * ((nrb + SB - 1) / SB) < 2L * ghost_ncu()) SB >>= 1;
  }
  const size_t lds = ((size_t)16 * SB * LW + (size_t)(TH + 2 * GH_HALO) * (TW + 2 * GH_HALO) * (16 * SB + 4) + 25 * 16 * SB) * 2;
  // 4-channel groups: 8-byte alignment serves every view; where Ch % 8 == 0 the callers' views are 16-byte aligned anyway
  const size_t va = Ch % 8 ? 8 : 16;
  const bool fits = tune().ghost && dtype == EY_F16 && k == 5 && C1 % 8 == 0 && Ch % 4 == 0 && lds <= 160 * 1024 && bias1 &&
                    (act == EY_ACT_NONE || act == EY_ACT_RELU || act == EY_ACT_SILU) && px >= tune().ghost_min_px && xbytes < (1L << 31) &&
                    (x_cstride * 2) % 16 == 0 && ey_aligned(x, 16) && (y_cstride * 2) % va == 0 && ey_aligned(y, va) &&
                    (!res || ((res_cstride * 2) % va == 0 && ey_aligned(res, va))) && ey_aligned(w1_packed, 16) && ey_aligned(w2_kkc, 16);
  if (!fits)
    return ey_set_error(EY_EUNSUPPORTED, "ghost_conv: outside the fused kernel (f16, k = 5, C1 %% 8 == 0, Ch %% 4 == 0, bias1, act none / ReLU / SiLU, aligned views)");
  GhP p;
  p.B = B; p.H = H; p.W = W; p.C1 = C1; p.Ch = Ch; p.KS = KS;
  p.x = x; p.xcs = x_cstride; p.xbytes = (unsigned)xbytes;
  p.w1 = w1_packed; p.Kpad = ey_conv_kpad(C1, 2); p.b1 = bias1;
  p.w2 = w2_kkc; p.b2 = bias2; p.act = act;
  p.res = res; p.rcs = res_cstride;
  p.y = y; p.ycs = y_cstride;
  p.NT = NT; p.nrb = nrb; p.LW = LW; p.TH = TH; p.TW = TW;
  p.tilesX = (W + TW - 1) / TW; p.tilesY = (H + TH - 1) / TH;
  const long ntile = (long)B * p.tilesX * p.tilesY;
  if (ntile >= (1L << 30)) return ey_set_error(EY_EUNSUPPORTED, "ghost_conv: too many tiles");
  p.ntile = (int)ntile;
  const int nslab = (nrb + SB - 1) / SB;
  hipStream_t st = (hipStream_t)stream;
  switch (SB) {
    case 1: return ghost_launch<1>(p, lds, nslab, st);
    case 2: return ghost_launch<2>(p, lds, nslab, st);
    default: return ghost_launch<4>(p, lds, nslab, st);
  }
}
