// Block programs: a whole chain of layers on SMALL feature maps (20x20 at 640x640) as ONE launch.
//
// At batch 32 the 20x20 part of the network (stride-2 conv -> DSC3K2_Wavelet -> SPPF -> C2PSA_LinearAttention, the last neck
// block, the 20x20 head towers) is ~45 launches of 5-20 us that each move 1-6 MB: pure launch / ramp-up / tail latency.  Here ONE
// persistent 1024-thread workgroup per image walks a "program" of stages (conv 1x1/3x3 with the full ey_conv2d epilogue, depthwise
// kxk, Haar DWT, the SPPF pool chain, MFMA linear attention) with a workgroup barrier between stages.  Activations go through
// global memory (they stay in L2: 20x20x256 f16 = 200 KB per image), weights stream from L2, nothing returns to the host between
// layers; 32 images occupy 32 CUs and leave the other 224 to the pipeline stages that run beside it (large-map, HBM-bound layers).
//
// Same arithmetic as the stand-alone kernels: f16 storage between stages (the reference's intermediate tensors), fp32
// accumulation (v_mfma_f32_16x16x32_f16), fp32 epilogues; the K order of every contraction is (ky, kx, source, channel) like
// ey_conv2d.  f16 only (the fp32 parity mode keeps the per-layer kernels).
#include "common.h"
#include "tune.h"
#include "linattn_mfma.inc.h"
#include <string.h>

#define BLK_THREADS 1024
#define BLK_WAVES 16
#define BLK_LDS_BYTES (104 * 1024)
#define BLK_MAX_EXT 8

typedef ey_block_stage BlkStage;
struct BlkExt { char* p[BLK_MAX_EXT]; };

__device__ __forceinline__ void load4(const f16* p, float (&o)[4]) {
  const f16x4 v = *reinterpret_cast<const f16x4*>(p);
#pragma unroll
  for (int j = 0; j < 4; ++j) o[j] = (float)v[j];
}
__device__ __forceinline__ void store4(f16* p, const float* v) {
  const f16x4 o = {(f16)v[0], (f16)v[1], (f16)v[2], (f16)v[3]};
  *reinterpret_cast<f16x4*>(p) = o;
}
__device__ __forceinline__ const f16* blk_ptr(const BlkExt& e, int64_t addr, int ext) {
  return reinterpret_cast<const f16*>(ext >= 0 ? e.p[ext] + addr : reinterpret_cast<char*>(addr));
}

// ---------------------------------------------------------------------------------------------------------------- conv epilogue
// ey_conv2d's: y = res + out_scale * act(acc + bias + bilinear(addz)) for one pixel (m = oy*Wo + ox) and the 4*NTI consecutive
// channels a lane owns; the pointers are already offset to the lane's first channel.  One 4-channel quad at a time (small live set).
struct BlkEpi {
  const float* bias;
  f16* y;
  const f16* res;
  const f16* z;
  int y_cs, res_cs, addz_cs, Hz, Wz, act;
  int nq;  // TAIL: quads of the lane's 4*NTI channels that lie below Cout (a Cout that is not a multiple of 4*NTI ends inside a lane's run)
  float zsy, zsx, out_scale;
};
template <int NTI, bool TAIL = false>
__device__ __forceinline__ void blk_epilogue(const BlkEpi& e, const f32x4 (&acc)[NTI], int m, int oy, int ox, int yrow = -1, int rrow = -1) {
  // (yrow / rrow: row index inside an LDS-resident tile instead of the pixel index m, block_tile_kernel)
  long z00 = 0, z01 = 0, z10 = 0, z11 = 0;
  float ly0 = 0.f, ly1 = 0.f, lx0 = 0.f, lx1 = 0.f;
  if (e.z) {  // F.interpolate(size=(Ho,Wo), bilinear, align_corners=False): ATen area_pixel_compute_source_index, scale = in/out
    const float sy = fmaxf(e.zsy * (oy + 0.5f) - 0.5f, 0.f), sx = fmaxf(e.zsx * (ox + 0.5f) - 0.5f, 0.f);
    const int y0 = (int)sy, x0 = (int)sx;
    const int y1 = min(y0 + 1, e.Hz - 1), x1 = min(x0 + 1, e.Wz - 1);
    ly1 = sy - y0; lx1 = sx - x0; ly0 = 1.f - ly1; lx0 = 1.f - lx1;
    z00 = (long)(y0 * e.Wz + x0) * e.addz_cs; z01 = (long)(y0 * e.Wz + x1) * e.addz_cs;
    z10 = (long)(y1 * e.Wz + x0) * e.addz_cs; z11 = (long)(y1 * e.Wz + x1) * e.addz_cs;
  }
  f16* yp = e.y + (long)(yrow >= 0 ? yrow : m) * e.y_cs;
  const f16* rp = e.res ? e.res + (long)(rrow >= 0 ? rrow : m) * e.res_cs : nullptr;
#pragma unroll
  for (int q = 0; q < NTI; ++q) {
    if (TAIL && q >= e.nq) break;  // channels >= Cout: neither read (bias, res, addz) nor written
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = acc[q][j];
    if (e.bias) {
      const f32x4 bv = *reinterpret_cast<const f32x4*>(e.bias + 4 * q);
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] += bv[j];
    }
    if (e.z) {
      float a00[4], a01[4], a10[4], a11[4];
      load4(e.z + z00 + 4 * q, a00); load4(e.z + z01 + 4 * q, a01); load4(e.z + z10 + 4 * q, a10); load4(e.z + z11 + 4 * q, a11);
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] += ly0 * (lx0 * a00[j] + lx1 * a01[j]) + ly1 * (lx0 * a10[j] + lx1 * a11[j]);
    }
    if (e.act == EY_ACT_SILU && e.out_scale == 1.f) {
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = v[j] * ey_sigmoid(v[j]);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = ey_act(v[j], e.act) * e.out_scale;
    }
    if (rp) {
      float rr[4];
      load4(rp + 4 * q, rr);
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] += rr[j];
    }
    store4(yp + 4 * q, v);
  }
}

// ---------------------------------------------------------------------------------------------------------------- conv
// Work item = (group, MT pixel tiles of 16, NTI of the NT 16-channel MFMA row blocks of one packed block tile); the 16 waves walk
// the items round-robin, consecutive waves share a pixel tile (its fragments hit in L1).  A = packed weights (row permutation of
// ey_conv_pack_weight: lane (r, g) ends up with 4*NTI CONSECUTIVE channels of pixel r), B = pixels by range-checked buffer loads
// (padding taps, pixel tails and channel tails read zeros).
template <int MT, int NTI>
__device__ void blk_conv(const BlkStage& sg, const BlkExt& ext, int b) {
  // the stage descriptor lives in global memory: every field the loops use is read ONCE into (scalar) registers here
  const int H = sg.H, W = sg.W, Wo = sg.Wo, kk = sg.k, stride = sg.stride, nsrc = sg.nsrc, Cout = sg.Cout, kpad = sg.kpad;
  const int C0 = sg.src_C[0], C1 = sg.src_C[1], cs0 = sg.src_cs[0], cs1 = sg.src_cs[1];
  const int ngroup = sg.ngroup, w_gmax = sg.w_gmax, act = sg.act;
  const long src_g = sg.src_g, y_g = sg.y_g, w_g = sg.w_g;
  const f16* src0 = blk_ptr(ext, sg.src[0], sg.src_ext[0]) + (long)b * sg.src_img[0];
  const f16* src1 = nsrc > 1 ? blk_ptr(ext, sg.src[1], sg.src_ext[1]) + (long)b * sg.src_img[1] : src0;
  const f16* wptr = reinterpret_cast<const f16*>(sg.w);
  const float* bptr = reinterpret_cast<const float*>(sg.bias);
  f16* yptr = const_cast<f16*>(blk_ptr(ext, sg.y, sg.y_ext)) + (long)b * sg.y_img;
  const int y_cs = sg.y_cs, res_cs = sg.res_cs, addz_cs = sg.addz_cs, Hz = sg.addz_H, Wz = sg.addz_W;
  const f16* resptr = sg.has_res ? blk_ptr(ext, sg.res, sg.res_ext) + (long)b * sg.res_img : nullptr;
  const f16* zptr = sg.has_addz ? blk_ptr(ext, sg.addz, sg.addz_ext) + (long)b * sg.addz_img : nullptr;
  const float zsy = sg.zsy, zsx = sg.zsx, out_scale = sg.out_scale;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
  const int M = sg.Ho * Wo, NT = sg.nt_pack, BN = 16 * NT;
  const int mtiles = (M + 16 * MT - 1) / (16 * MT);
  const int nsub = NT / NTI, nblk = (Cout + BN - 1) / BN;
  const int nitems = ngroup * mtiles * nblk * nsub;
  const int pad = kk >> 1;
  const unsigned bytes0 = (unsigned)((((long)H * W - 1) * cs0 + C0) * 2), bytes1 = (unsigned)((((long)H * W - 1) * cs1 + C1) * 2);
  for (int it = wave; it < nitems; it += BLK_WAVES) {
    const int sub = it % nsub;
    int t = it / nsub;
    const int nb = t % nblk;
    t /= nblk;
    const int mt_i = t % mtiles, grp = t / mtiles;
    const int wset = min(grp, w_gmax);
    // ---- operands
    __amdgpu_buffer_rsrc_t rs[2];
    rs[0] = ey_rsrc(src0 + (long)grp * src_g, bytes0);
    rs[1] = ey_rsrc(src1, bytes1);
    const __amdgpu_buffer_rsrc_t rw = ey_rsrc(wptr + (long)wset * w_g, (unsigned)((long)nblk * BN * kpad * 2));
    unsigned woff[NTI];
#pragma unroll
    for (int nt = 0; nt < NTI; ++nt) woff[nt] = (unsigned)((((nb * BN + (sub * NTI + nt) * 16 + r) * kpad) + 8 * g) * 2);
    int oy[MT], ox[MT];
    bool pv[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      const int m = (mt_i * MT + mt) * 16 + r;
      pv[mt] = m < M;
      const int mm = pv[mt] ? m : 0;
      oy[mt] = mm / Wo;
      ox[mt] = mm - oy[mt] * Wo;
    }
    f32x4 acc[MT][NTI];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int nt = 0; nt < NTI; ++nt) acc[mt][nt] = (f32x4)0.f;
    // ---- K loop: k-steps = (ky, kx, source, 32-channel step), walked U at a time: the loads of U steps are issued back to back
    // (a lone step is one dependent round trip to L2, ~1 us: the loop would be pure latency), then their MFMAs
    constexpr int U = (MT + NTI <= 3) ? 4 : (MT + NTI <= 5) ? 3 : 2;
    int ky = 0, kx = 0, si = 0, c0 = 0, kofs = 0;
    bool more = true;
    while (more) {
      Vec8<f16> bf[U][MT], af[U][NTI];
      bool live[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        live[u] = more;
        if (more) {  // (wave-uniform)
          const int C = si == 0 ? C0 : C1, cs2 = (si == 0 ? cs0 : cs1) * 2;
          const bool chan_ok = c0 + 8 * g < C;  // channel tail of a source that is not a multiple of 32: zeros, not the neighbour's data
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) {
            const int iy = oy[mt] * stride - pad + ky, ix = ox[mt] * stride - pad + kx;
            const bool inb = chan_ok && pv[mt] && iy >= 0 && iy < H && ix >= 0 && ix < W;
            const unsigned po = inb ? (unsigned)(iy * W + ix) * (unsigned)cs2 + 16u * g : EY_OOB;
            if (si == 0) BufLoad8<f16>::load(bf[u][mt], rs[0], po, c0 * 2);
            else BufLoad8<f16>::load(bf[u][mt], rs[1], po, c0 * 2);
          }
#pragma unroll
          for (int nt = 0; nt < NTI; ++nt) BufLoad8<f16>::load(af[u][nt], rw, woff[nt], (kofs + c0) * 2);
          // advance the (wave-uniform) k-step iterator
          c0 += 32;
          if (c0 >= C) {
            kofs += C;
            c0 = 0;
            if (++si >= nsrc) {
              si = 0;
              if (++kx >= kk) {
                kx = 0;
                if (++ky >= kk) more = false;
              }
            }
          }
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (live[u]) {
#pragma unroll
          for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int nt = 0; nt < NTI; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[u][nt].v, bf[u][mt].v, acc[mt][nt], 0, 0, 0);
        }
      }
    }
    // ---- epilogue
    const int ch0 = nb * BN + g * 4 * NT + 4 * sub * NTI;
    if (ch0 >= Cout) continue;
    BlkEpi e;
    e.bias = bptr ? bptr + wset * Cout + ch0 : nullptr;
    e.y = yptr + (long)grp * y_g + ch0;
    e.res = resptr ? resptr + (long)grp * y_g + ch0 : nullptr;
    e.z = zptr ? zptr + (long)grp * y_g + ch0 : nullptr;
    e.y_cs = y_cs; e.res_cs = res_cs; e.addz_cs = addz_cs; e.Hz = Hz; e.Wz = Wz; e.act = act; e.zsy = zsy; e.zsx = zsx; e.out_scale = out_scale;
    e.nq = min(NTI, (Cout - ch0) >> 2);
    const bool tail = Cout % (4 * NTI) != 0;  // (uniform over the stage)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
      if (pv[mt]) {
        if (tail) blk_epilogue<NTI, true>(e, acc[mt], (mt_i * MT + mt) * 16 + r, oy[mt], ox[mt]);
        else blk_epilogue<NTI>(e, acc[mt], (mt_i * MT + mt) * 16 + r, oy[mt], ox[mt]);
      }
  }
}

// ---------------------------------------------------------------------------------------------------------------- depthwise
// y[p][c] = act(sum_taps x[p + tap][c] * w[tap][c] + bias[c]), k x k, stride 1, pad k/2; thread item = (pixel, 8 channels).
// DSConv.dw (conv.py:94-97,102; no bias, no activation, result rounded to f16 like the reference's intermediate tensor) and DWConv.
__device__ void blk_dw(const BlkStage& s, const BlkExt& ext, int b) {
  const int C = s.src_C[0], cv = C >> 3, H = s.H, W = s.W, HW = H * W, k = s.k, pad = k >> 1, xcs = s.src_cs[0], ycs = s.y_cs, act = s.act;
  const f16* xb = blk_ptr(ext, s.src[0], s.src_ext[0]) + (long)b * s.src_img[0];
  const __amdgpu_buffer_rsrc_t rx = ey_rsrc(xb, (unsigned)((((long)HW - 1) * xcs + C) * 2));
  const f16* w = reinterpret_cast<const f16*>(s.w);
  const float* bias = reinterpret_cast<const float*>(s.bias);
  f16* yb = const_cast<f16*>(blk_ptr(ext, s.y, s.y_ext)) + (long)b * s.y_img;
  for (int i = threadIdx.x; i < HW * cv; i += BLK_THREADS) {
    const int c8 = (i % cv) * 8, p = i / cv;
    const int py = p / W, px = p - py * W;
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.f;
    for (int ky = 0; ky < k; ++ky) {
      const int iy = py - pad + ky;
      for (int kx = 0; kx < k; ++kx) {
        const int ix = px - pad + kx;
        const bool inb = iy >= 0 && iy < H && ix >= 0 && ix < W;
        Vec8<f16> xv, wv;
        BufLoad8<f16>::load(xv, rx, inb ? (unsigned)(((iy * W + ix) * xcs + c8) * 2) : EY_OOB);
        wv.load(w + (ky * k + kx) * C + c8);
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] += xv.get(j) * wv.get(j);
      }
    }
    Vec8<f16> o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o.set(j, ey_act(acc[j] + (bias ? bias[c8 + j] : 0.f), act));
    o.store(yb + (long)p * ycs + c8);
  }
}

// ---------------------------------------------------------------------------------------------------------------- Haar DWT
// _PywtDWT2D.forward (block.py:3619-3642), same arithmetic as dwt_kernel: taps float32(1/sqrt2)^2; y = [LL | LH | HL | HH] channel blocks.
__device__ void blk_dwt(const BlkStage& s, const BlkExt& ext, int b) {
  const int C = s.src_C[0], cv = C >> 3, Ho = s.Ho, Wo = s.Wo, W = s.W, xcs = s.src_cs[0], ycs = s.y_cs;
  const f16* xb = blk_ptr(ext, s.src[0], s.src_ext[0]) + (long)b * s.src_img[0];
  f16* yb = const_cast<f16*>(blk_ptr(ext, s.y, s.y_ext)) + (long)b * s.y_img;
  const float sq = 0.70710678118654752440f, tp = sq * sq;
  for (int i = threadIdx.x; i < Ho * Wo * cv; i += BLK_THREADS) {
    const int c8 = (i % cv) * 8, m = i / cv;
    const int oy = m / Wo, ox = m - oy * Wo;
    const f16* p00 = xb + (long)((2 * oy) * W + 2 * ox) * xcs + c8;
    Vec8<f16> a, bq, c, d, ll, lh, hl, hh;
    a.load(p00); bq.load(p00 + xcs); c.load(p00 + (long)W * xcs); d.load(p00 + (long)(W + 1) * xcs);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float fa = a.get(j) * tp, fb = bq.get(j) * tp, fc = c.get(j) * tp, fd = d.get(j) * tp;
      ll.set(j, (fa + fb) + (fc + fd));
      lh.set(j, (fa - fb) + (fc - fd));
      hl.set(j, (fa + fb) - (fc + fd));
      hh.set(j, (fa - fb) - (fc - fd));
    }
    f16* yp = yb + (long)m * ycs + c8;
    ll.store(yp); lh.store(yp + C); hl.store(yp + 2 * C); hh.store(yp + 3 * C);
  }
}

// ---------------------------------------------------------------------------------------------------------------- SPPF pool chain
// y1 = mp5(x), y2 = mp5(y1), y3 = mp5(y2) (block.py:219-223; padding acts as -inf): per chunk of channel octets the H x W planes
// live in LDS (two buffers), separable max (row pass, column pass) three times; y_k = y + k*C channels of the concat buffer.
__device__ void blk_pool(const BlkStage& s, const BlkExt& ext, int b, char* smem) {
  const int C = s.src_C[0], cv = C >> 3, H = s.H, W = s.W, HW = H * W, xcs = s.src_cs[0], ycs = s.y_cs;
  const f16* xb = blk_ptr(ext, s.src[0], s.src_ext[0]) + (long)b * s.src_img[0];
  f16* yb = const_cast<f16*>(blk_ptr(ext, s.y, s.y_ext)) + (long)b * s.y_img;
  const int cvc = max(1, min(cv, (BLK_LDS_BYTES / 2) / (HW * 16)));  // channel octets per chunk (host checked that one fits)
  Vec8<f16>* A = reinterpret_cast<Vec8<f16>*>(smem);
  Vec8<f16>* Bf = A + cvc * HW;
  for (int cg0 = 0; cg0 < cv; cg0 += cvc) {
    const int ng = min(cvc, cv - cg0);
    __syncthreads();  // the previous chunk's LDS reads are done
    for (int i = threadIdx.x; i < ng * HW; i += BLK_THREADS) {
      const int cg = i % ng, p = i / ng;
      A[cg * HW + p].load(xb + (long)p * xcs + (cg0 + cg) * 8);
    }
    __syncthreads();
    for (int pass = 0; pass < 3; ++pass) {
      for (int i = threadIdx.x; i < ng * HW; i += BLK_THREADS) {  // rows
        const int cg = i / HW, p = i - cg * HW, yy = p / W, xx = p - yy * W;
        const Vec8<f16>* row = A + cg * HW + yy * W;
        Vec8<f16> mx = row[xx];
        for (int dx = -2; dx <= 2; ++dx) {
          const int x2 = xx + dx;
          if (dx == 0 || x2 < 0 || x2 >= W) continue;
          const Vec8<f16> o = row[x2];
#pragma unroll
          for (int j = 0; j < 8; ++j) mx.set(j, fmaxf(mx.get(j), o.get(j)));
        }
        Bf[i] = mx;
      }
      __syncthreads();
      for (int i = threadIdx.x; i < ng * HW; i += BLK_THREADS) {  // columns
        const int cg = i / HW, p = i - cg * HW, yy = p / W, xx = p - yy * W;
        const Vec8<f16>* pl = Bf + cg * HW;
        Vec8<f16> mx = pl[p];
        for (int dy = -2; dy <= 2; ++dy) {
          const int y2 = yy + dy;
          if (dy == 0 || y2 < 0 || y2 >= H) continue;
          const Vec8<f16> o = pl[y2 * W + xx];
#pragma unroll
          for (int j = 0; j < 8; ++j) mx.set(j, fmaxf(mx.get(j), o.get(j)));
        }
        mx.store(yb + (long)p * ycs + (long)pass * C + (cg0 + cg) * 8);  // y = the y1 slot; y2, y3 follow it at C-channel steps
        A[i] = mx;  // only element i of A is touched by this thread
      }
      __syncthreads();
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------- linear attention
// LinearAttention.forward core (block.py:3360-3373) for head_dim 64: two heads side by side (512 threads each).
__device__ void blk_linattn(const BlkStage& s, const BlkExt& ext, int b, char* smem) {
  LinAttnLds* S = reinterpret_cast<LinAttnLds*>(smem);
  const int N = s.H * s.W, C = s.Cout, half = threadIdx.x >> 9, tid = threadIdx.x & 511;
  const f16* qkv = blk_ptr(ext, s.src[0], s.src_ext[0]) + (long)b * s.src_img[0];
  f16* y = const_cast<f16*>(blk_ptr(ext, s.y, s.y_ext)) + (long)b * s.y_img;
  for (int h0 = 0; h0 < s.heads; h0 += 2) {
    const int h = h0 + half;
    __syncthreads();  // LDS of the previous pair is free
    const f16* qb = qkv + h * 64;
    linattn_mfma_head(S[half], N, qb, qb + C, qb + 2 * C, s.src_cs[0], y + h * 64, s.y_cs, tid);
  }
}

// ---------------------------------------------------------------------------------------------------------------- the kernel
template <int MT>
__device__ __forceinline__ void blk_conv_nti(const BlkStage& s, const BlkExt& ext, int b) {
  switch (s.nti) {
    case 1: blk_conv<MT, 1>(s, ext, b); break;
    case 2: blk_conv<MT, 2>(s, ext, b); break;
    case 4: if constexpr (MT <= 2) blk_conv<MT, 4>(s, ext, b); break;
    case 5: if constexpr (MT == 1) blk_conv<MT, 5>(s, ext, b); break;
    default: break;
  }
}

__global__ __launch_bounds__(BLK_THREADS) void block_kernel(const BlkStage* __restrict__ prog, int nstages, BlkExt ext, long long* __restrict__ tstamps) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int b = blockIdx.x;
  if (tstamps && b == 0 && threadIdx.x == 0) tstamps[0] = wall_clock64();
  for (int si = 0; si < nstages; ++si) {
    const BlkStage& s = prog[si];
    switch (s.op) {
      case EY_BLK_CONV:
        if (s.mt == 1) blk_conv_nti<1>(s, ext, b);
        else if (s.mt == 2) blk_conv_nti<2>(s, ext, b);
        else blk_conv_nti<4>(s, ext, b);
        break;
      case EY_BLK_DW: blk_dw(s, ext, b); break;
      case EY_BLK_DWT: blk_dwt(s, ext, b); break;
      case EY_BLK_POOL: blk_pool(s, ext, b, smem); break;
      case EY_BLK_LINATTN: blk_linattn(s, ext, b, smem); break;
      default: break;
    }
    __syncthreads();  // this stage's global writes are visible to the whole workgroup (one CU, one L1) before the next stage reads them
    if (tstamps && b == 0 && threadIdx.x == 0) tstamps[si + 1] = wall_clock64();  // (developer timing, ey_block_run_timed)
  }
}

// ---------------------------------------------------------------------------------------------------------------- pointwise chains
// A chain of 1x1 convs (every stage: k = 1, stride 1, one group, the same map) has no coupling between pixels, so it needs no
// per-image workgroup: one 256-thread workgroup per TILE_PX = 32 pixels walks the stages; its 4 waves split the output-channel blocks
// of a stage (2 pixel tiles x NTI row blocks per item: every weight fragment feeds two MFMAs).  Built for a short dependent chain per
// stage: the stage descriptors are resolved ONCE into LDS, intermediates that only the chain reads live in LDS (rows of C + 8
// halves: conflict-free 16-byte reads), the weight fragments of a whole item are requested in batches of 8 k-steps, and only the
// chain's outputs go to global memory.  C2PSA's proj -> ffn -> ffn -> cv2 tail, cv1 -> qkv, the enhancer tail -> DSC3k.cv1|cv2,
// DSC3k.cv3 -> DSC3K2.cv2 (block.py:3412-3497,1506-1562,3749-3788).
#define TILE_PX 32
#define TILE_MAX_STAGES 8
struct TStage {
  const f16* src[2]; const f16* w; const float* bias; f16* y; const f16* res; const f16* z;
  int src_lds[2], src_cs[2], src_C[2], nsrc;     // src_lds >= 0: element offset of the source's pixel row 0 in LDS (row stride src_cs)
  int y_lds, y_cs, res_lds, res_cs;               // same for the output / residual (y_lds >= 0: the stage writes LDS only)
  int kpad, nt_pack, nti, Cout, act, addz_cs, Hz, Wz;
  float zsy, zsx, out_scale;
};

template <int NTI>
__device__ __forceinline__ void tile_conv(const TStage& t, f16* lds, int b, int m0, int M, int Wo) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
  const int NT = t.nt_pack, BN = 16 * NT, nsub = NT / NTI, nblk = (t.Cout + BN - 1) / BN, nitems = nblk * nsub;
  const int C0 = t.src_C[0], C1 = t.nsrc > 1 ? t.src_C[1] : 0;
  const int nks0 = (C0 + 31) >> 5, nks = nks0 + ((C1 + 31) >> 5);
  const __amdgpu_buffer_rsrc_t rw = ey_rsrc(t.w, (unsigned)((long)nblk * BN * t.kpad * 2));
  const __amdgpu_buffer_rsrc_t rs0 = ey_rsrc(t.src[0], t.src_lds[0] >= 0 ? 0u : (unsigned)((((long)M - 1) * t.src_cs[0] + C0) * 2));
  const __amdgpu_buffer_rsrc_t rs1 = ey_rsrc(t.nsrc > 1 ? t.src[1] : t.src[0], (t.nsrc < 2 || t.src_lds[1] >= 0) ? 0u : (unsigned)((((long)M - 1) * t.src_cs[1] + C1) * 2));
  bool pv[2];
  int mm[2];
#pragma unroll
  for (int mt = 0; mt < 2; ++mt) { mm[mt] = m0 + mt * 16 + r; pv[mt] = mm[mt] < M; }
  for (int it = wave; it < nitems; it += 4) {
    const int sub = it % nsub, nb = it / nsub;
    unsigned woff[NTI];
#pragma unroll
    for (int nt = 0; nt < NTI; ++nt) woff[nt] = (unsigned)((((nb * BN + (sub * NTI + nt) * 16 + r) * t.kpad) + 8 * g) * 2);
    f32x4 acc[2][NTI];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int nt = 0; nt < NTI; ++nt) acc[mt][nt] = (f32x4)0.f;
    constexpr int U = NTI >= 4 ? 4 : 8;  // k-steps per batch of loads (U * NTI weight fragments + 2U pixel fragments in flight)
    for (int jb = 0; jb < nks; jb += U) {
      Vec8<f16> af[U][NTI], bf[U][2];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int j = jb + u;
        const bool on = j < nks, s1 = j >= nks0;                    // (wave-uniform)
        const int c0 = 32 * (s1 ? j - nks0 : j), Cs = s1 ? C1 : C0;
        const int kof = s1 ? C0 + c0 : c0;                          // k offset of this step in the packed row
#pragma unroll
        for (int nt = 0; nt < NTI; ++nt) BufLoad8<f16>::load(af[u][nt], rw, on ? woff[nt] : EY_OOB, kof * 2);
        const bool chan_ok = on && c0 + 8 * g < Cs;                 // channel tail of a source that is not a multiple of 32: zeros
        const int sl = s1 ? t.src_lds[1] : t.src_lds[0], cs = s1 ? t.src_cs[1] : t.src_cs[0];
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
          if (sl >= 0) {  // an intermediate of the chain: this tile's rows in LDS
            if (chan_ok) bf[u][mt].load(lds + sl + (mt * 16 + r) * cs + c0 + 8 * g);
            else bf[u][mt].zero();
          } else {
            const unsigned po = (chan_ok && pv[mt]) ? (unsigned)mm[mt] * (unsigned)(cs * 2) + 16u * g : EY_OOB;
            if (s1) BufLoad8<f16>::load(bf[u][mt], rs1, po, c0 * 2);
            else BufLoad8<f16>::load(bf[u][mt], rs0, po, c0 * 2);
          }
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (jb + u < nks) {
#pragma unroll
          for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int nt = 0; nt < NTI; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[u][nt].v, bf[u][mt].v, acc[mt][nt], 0, 0, 0);
        }
    }
    const int ch0 = nb * BN + g * 4 * NT + 4 * sub * NTI;
    if (ch0 >= t.Cout) continue;
    BlkEpi e;
    e.bias = t.bias ? t.bias + ch0 : nullptr;
    e.z = t.z ? t.z + ch0 : nullptr;
    e.addz_cs = t.addz_cs; e.Hz = t.Hz; e.Wz = t.Wz; e.act = t.act; e.zsy = t.zsy; e.zsx = t.zsx; e.out_scale = t.out_scale;
    e.y_cs = t.y_cs; e.res_cs = t.res_cs;
    e.nq = min(NTI, (t.Cout - ch0) >> 2);
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
      if (!pv[mt]) continue;
      // LDS-resident tensors are indexed by the pixel's position in the tile, global ones by the pixel
      const int row = mt * 16 + r;
      e.y = (t.y_lds >= 0 ? lds + t.y_lds : t.y) + ch0;
      e.res = t.res ? (t.res_lds >= 0 ? lds + t.res_lds : t.res) + ch0 : nullptr;
      const int oy = mm[mt] / Wo;
      const int yrow = t.y_lds >= 0 ? row : -1, rrow = (t.res && t.res_lds >= 0) ? row : -1;
      if (t.Cout % (4 * NTI) != 0) blk_epilogue<NTI, true>(e, acc[mt], mm[mt], oy, mm[mt] - oy * Wo, yrow, rrow);  // (uniform over the stage)
      else blk_epilogue<NTI>(e, acc[mt], mm[mt], oy, mm[mt] - oy * Wo, yrow, rrow);
    }
  }
}

__global__ __launch_bounds__(256) void block_tile_kernel(const BlkStage* __restrict__ prog, int nstages, BlkExt ext) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  TStage* ts = reinterpret_cast<TStage*>(smem);                                   // [TILE_MAX_STAGES]
  f16* lds = reinterpret_cast<f16*>(smem + TILE_MAX_STAGES * sizeof(TStage));     // the tile's chain-internal tensors
  const int b = blockIdx.y, m0 = blockIdx.x * TILE_PX;
  if ((int)threadIdx.x < nstages) {  // resolve every stage once (pointers of this image, LDS placement): no global round trip per stage later
    const BlkStage& s = prog[threadIdx.x];
    TStage t;
    for (int j = 0; j < 2; ++j) {
      const int jj = j < s.nsrc ? j : 0;
      t.src[j] = blk_ptr(ext, s.src[jj], s.src_ext[jj]) + (long)b * s.src_img[jj];
      t.src_lds[j] = s.tile_src_lds[jj]; t.src_cs[j] = s.tile_src_lds[jj] >= 0 ? s.tile_src_lcs[jj] : s.src_cs[jj]; t.src_C[j] = s.src_C[jj];
    }
    t.nsrc = s.nsrc;
    t.w = reinterpret_cast<const f16*>(s.w); t.bias = reinterpret_cast<const float*>(s.bias);
    t.y = const_cast<f16*>(blk_ptr(ext, s.y, s.y_ext)) + (long)b * s.y_img;
    t.y_lds = s.tile_y_lds; t.y_cs = s.tile_y_lds >= 0 ? s.tile_y_lcs : s.y_cs;
    t.res = s.has_res ? blk_ptr(ext, s.res, s.res_ext) + (long)b * s.res_img : nullptr;
    t.res_lds = s.has_res ? s.tile_res_lds : -1; t.res_cs = (s.has_res && s.tile_res_lds >= 0) ? s.tile_res_lcs : s.res_cs;
    t.z = s.has_addz ? blk_ptr(ext, s.addz, s.addz_ext) + (long)b * s.addz_img : nullptr;
    t.kpad = s.kpad; t.nt_pack = s.nt_pack; t.nti = s.tile_nti; t.Cout = s.Cout; t.act = s.act; t.addz_cs = s.addz_cs; t.Hz = s.addz_H; t.Wz = s.addz_W;
    t.zsy = s.zsy; t.zsx = s.zsx; t.out_scale = s.out_scale;
    ts[threadIdx.x] = t;
  }
  const int M = prog[0].Ho * prog[0].Wo, Wo = prog[0].Wo;
  __syncthreads();
  for (int si = 0; si < nstages; ++si) {
    const TStage& t = ts[si];
    switch (t.nti) {
      case 1: tile_conv<1>(t, lds, b, m0, M, Wo); break;
      case 2: tile_conv<2>(t, lds, b, m0, M, Wo); break;
      case 4: tile_conv<4>(t, lds, b, m0, M, Wo); break;
      case 5: tile_conv<5>(t, lds, b, m0, M, Wo); break;
      default: break;
    }
    __syncthreads();  // the tile's stage output (LDS, or global written by this workgroup) is visible to the next stage
  }
}

// ---------------------------------------------------------------------------------------------------------------- register-weight chains
// The same pointwise chains with the roles of conv_pwn_kernel: a 512-thread workgroup owns FAST_PX = 64 consecutive pixels of one image
// (4 MFMA pixel blocks); in every stage wave w owns the 16-row output blocks w, w + 8, ... and keeps ITS weight fragments in registers,
// so a fragment is read once per workgroup and feeds 4 MFMAs (block_tile_kernel: once per 32 pixels, 2 MFMAs).  No weight load waits
// for data: the fragments of stage 0 are requested first thing, those of stage s + 1 before stage s multiplies.  Every global tensor the
// chain reads (sources, residuals) and every bias is requested before the first barrier and goes to LDS once; a stage reads its pixel
// fragments and its residual there and writes its output there (dead tensors are aliased), from where a lane copies what the caller
// sees to global memory; ONE LDS-only barrier separates two stages.  Fragment counts index registers, so they are compile-time: a chain runs here when its
// (k-steps, row blocks per wave) list is one of FAST_CHAINS below (ey_block_fast_plan decides; everything else keeps block_tile_kernel).
// Arithmetic is tile_conv's: source 0 then source 1 in ascending 32-channel steps, one fp32 chain per output, blk_epilogue.
#define FAST_PX 64
#define FAST_WAVES 8
#define FAST_MAX_STAGES 4
#define FAST_MAX_JOBS 4
#define FAST_MAX_SLOTS 8               // 512-vector rounds of the preload (<= 4096 16-byte vectors per tile)
#define FAST_LDS_MAX (96 * 1024)

struct FJob {     // one 512-vector round of a global tensor tile -> LDS (C channels of the tile's pixels); unused rounds: nv = 0, nothing is read
  int64_t addr, img;     // (ext, addr) as in the program; the launch turns addr into the absolute address
  int32_t ext, cs, C, cv, inv, nv, lds, pitch, v0, bytes;  // cv = C / 8 vectors per pixel, inv = ceil(2^20 / cv), nv = 64 * cv, lds / pitch in elements, v0 = first vector of the round, bytes = extent of an image's view
};
struct FStage {
  const f16* w; const float* bias;
  int64_t y, y_img;
  int32_t y_ext, y_cs, y_glob, y_lds, y_pitch;   // y_glob: the caller sees the output (written to global memory behind its LDS slot)
  int32_t res_lds, res_pitch;                    // residual (always LDS-resident), -1 = none
  int32_t src_lds[2], src_pitch[2], nks0;        // nks0 = 32-channel steps of source 0
  int32_t bias_lds, bias_bytes;                  // fp32 index into the bias area (at bias_base elements), -1 = no bias; 4 * Cout or 0
  int32_t kpad, nt, nrb, Cout, act;
  float out_scale;
};
struct FPlan {
  int32_t sig, nstages, njobs, nslot, lds_bytes, M, bias_base, pad_;
  FJob slot[FAST_MAX_SLOTS];
  FStage st[FAST_MAX_STAGES];
};

typedef __attribute__((address_space(1))) f16 gf16;
typedef __attribute__((address_space(1))) f16x4 gf16x4;
template <int KS, int NRW> struct FS { static constexpr int ks = KS, nrw = NRW, nf = KS * NRW, code = KS * 8 + NRW; };
template <class A, class... R> struct FFirst { typedef A type; };

template <class S>
__device__ __forceinline__ void fast_wload(Vec8<f16> (&wf)[S::nf], const FStage& t) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
  const __amdgpu_buffer_rsrc_t rw = ey_rsrc(t.w, (unsigned)((long)t.nrb * 16 * t.kpad * 2));
#pragma unroll
  for (int i = 0; i < S::nrw; ++i) {
    const int rb = wave + FAST_WAVES * i;
    const unsigned off = rb < t.nrb ? (unsigned)(((rb * 16 + r) * t.kpad + 8 * g) * 2) : EY_OOB;
#pragma unroll
    for (int ks = 0; ks < S::ks; ++ks) BufLoad8<f16>::load(wf[ks * S::nrw + i], rw, off, ks * 64);
  }
}

template <class S>
__device__ __forceinline__ void fast_stage(const FStage& t, const Vec8<f16> (&wf)[S::nf], f16* lds, const float* lbias, int b, int m0, int M) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
  if (wave >= t.nrb) return;  // (fewer row blocks than waves: this wave owns none)
  f32x4 acc[S::nrw][4][1];
#pragma unroll
  for (int i = 0; i < S::nrw; ++i)
#pragma unroll
    for (int pb = 0; pb < 4; ++pb) acc[i][pb][0] = (f32x4)0.f;
  const int nks0 = t.nks0, p0 = t.src_pitch[0], p1 = t.src_pitch[1];
  const int o0 = t.src_lds[0] + r * p0 + 8 * g, o1 = t.src_lds[1] + r * p1 + 8 * g;
#pragma unroll
  for (int ks = 0; ks < S::ks; ++ks) {
    const bool s1 = ks >= nks0;  // (wave-uniform)
    const int o = s1 ? o1 + (ks - nks0) * 32 : o0 + ks * 32, pit = s1 ? p1 : p0;
    Vec8<f16> bq[4];
#pragma unroll
    for (int pb = 0; pb < 4; ++pb) bq[pb].load(lds + o + pb * 16 * pit);
#pragma unroll
    for (int i = 0; i < S::nrw; ++i)
#pragma unroll
      for (int pb = 0; pb < 4; ++pb) acc[i][pb][0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[ks * S::nrw + i].v, bq[pb].v, acc[i][pb][0], 0, 0, 0);
  }
  // ---- epilogue: lane (r, g) holds 4 consecutive channels of pixel 16 pb + r per row block (ey_conv_pack_weight's row permutation)
#pragma unroll
  for (int i = 0; i < S::nrw; ++i) {
    const int rb = wave + FAST_WAVES * i;
    if (rb >= t.nrb) break;
    const int nb = rb / t.nt, j = rb - nb * t.nt;
    const int ch0 = (nb * 16 + 4 * g) * t.nt + 4 * j;
    BlkEpi e;
    e.bias = t.bias_lds >= 0 ? lbias + t.bias_lds + ch0 : nullptr;
    e.z = nullptr; e.addz_cs = 0; e.Hz = 0; e.Wz = 0; e.zsy = 0.f; e.zsx = 0.f;
    e.act = t.act; e.out_scale = t.out_scale; e.nq = 1;
    e.res = t.res_lds >= 0 ? lds + t.res_lds + ch0 : nullptr;
    e.res_cs = t.res_pitch;
    gf16* yg = t.y_glob ? (gf16*)(reinterpret_cast<f16*>(t.y) + (long)b * t.y_img + ch0) : nullptr;
    // Always through LDS (a slot of its own, aliased over dead tensors, when no later stage reads the output): blk_epilogue's stores
    // are then LDS writes, and the lane copies its own 4 halves out with a GLOBAL store.  Through a generic pointer both would be
    // flat stores, which count as LDS traffic as well: every later LDS wait (bias, residual, the stage barrier) would wait for them.
    f16* yl = lds + t.y_lds + ch0;
    e.y = yl; e.y_cs = t.y_pitch;
#pragma unroll
    for (int pb = 0; pb < 4; ++pb) {
      const int row = pb * 16 + r, m = m0 + row;
      if (m >= M) continue;
      blk_epilogue<1>(e, acc[i][pb], m, 0, 0, row, row);
      if (t.y_glob) *reinterpret_cast<gf16x4*>(yg + (long)m * t.y_cs) = *reinterpret_cast<const f16x4*>(yl + row * t.y_pitch);
    }
  }
}

template <int SI, class Pre, class S0, class... Rest>
__device__ __forceinline__ void fast_run(const FPlan& p, const Vec8<f16> (&wf)[S0::nf], const Pre& pre, f16* lds, const float* lbias, int b, int m0) {
  if constexpr (sizeof...(Rest) > 0) {
    typedef typename FFirst<Rest...>::type S1;
    Vec8<f16> wn[S1::nf];
    fast_wload<S1>(wn, p.st[SI + 1]);  // in flight while this stage multiplies
    if constexpr (SI == 0) pre();
    fast_stage<S0>(p.st[SI], wf, lds, lbias, b, m0, p.M);
    ey_lds_barrier();  // this stage's LDS output is complete, its LDS inputs are free
    fast_run<SI + 1, Pre, Rest...>(p, wn, pre, lds, lbias, b, m0);
  } else {
    if constexpr (SI == 0) pre();
    fast_stage<S0>(p.st[SI], wf, lds, lbias, b, m0, p.M);
  }
}

template <class... S>
__global__ __launch_bounds__(512) void block_chain_kernel(FPlan p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  f16* lds = reinterpret_cast<f16*>(smem);
  float* lbias = reinterpret_cast<float*>(lds + p.bias_base);
  typedef typename FFirst<S...>::type S0;
  const int tid = threadIdx.x, b = blockIdx.y, m0 = blockIdx.x * FAST_PX, M = p.M;
  Vec8<f16> w0[S0::nf];
  fast_wload<S0>(w0, p.st[0]);
  // ---- every global tile and bias of the chain: all requests first, LDS stores behind the next stage's weight requests
  // (branch-free: the plan carries one descriptor per round, an unused round or a missing bias is an empty buffer and reads nothing)
  Vec8<f16> pv[FAST_MAX_SLOTS];
  int pdst[FAST_MAX_SLOTS];
#pragma unroll
  for (int u = 0; u < FAST_MAX_SLOTS; ++u) {
    const FJob& jb = p.slot[u];
    const int v = tid + jb.v0;
    const int px = (int)(((unsigned)v * (unsigned)jb.inv) >> 20), c8 = v - px * jb.cv;  // v / cv, exact for v < 4096 (cv < 256)
    const unsigned goff = (unsigned)(((m0 + px) * jb.cs + c8 * 8) * 2);
    const int ldst = jb.lds + px * jb.pitch + c8 * 8;
    const bool in = v < jb.nv, ok = in & (m0 + px < M);  // (selects, no control flow: a branch here puts a wait for ALL loads in flight between two rounds)
    const __amdgpu_buffer_rsrc_t rs = ey_rsrc(reinterpret_cast<const f16*>(jb.addr) + (long)b * jb.img, (unsigned)jb.bytes);
    BufLoad8<f16>::load(pv[u], rs, ok ? goff : EY_OOB);
    pdst[u] = in ? ldst : -1;
  }
  float bv[FAST_MAX_STAGES];
#pragma unroll
  for (int s = 0; s < FAST_MAX_STAGES; ++s) {
    const FStage& t = p.st[s];  // (beyond nstages: zero-filled, bias_lds = -1)
    const __amdgpu_buffer_rsrc_t rb = ey_rsrc(t.bias, (unsigned)t.bias_bytes);
    bv[s] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rb, tid * 4, 0, 0));
  }
  auto pre = [&]() {
#pragma unroll
    for (int u = 0; u < FAST_MAX_SLOTS; ++u)
      if (pdst[u] >= 0) pv[u].store(lds + pdst[u]);
#pragma unroll
    for (int s = 0; s < FAST_MAX_STAGES; ++s)
      if (p.st[s].bias_lds >= 0 && tid < p.st[s].Cout) lbias[p.st[s].bias_lds + tid] = bv[s];
    ey_lds_barrier();
  };
  fast_run<0, decltype(pre), S...>(p, w0, pre, lds, lbias, b, m0);
}

// the instantiated chains: (k-steps, row blocks per wave) per stage
#define FAST_CHAINS(X)                                \
  X(FS<4, 1>, FS<4, 2>, FS<8, 1>, FS<8, 2>) /* C2PSA tail at c = 128: proj 128->128, ffn 128->256->128, cv2 256->256 */ \
  X(FS<8, 2>, FS<4, 3>)                     /* C2PSA head at c = 128: cv1 256->256, qkv 128->384 */                     \
  X(FS<2, 1>, FS<2, 1>, FS<4, 1>, FS<4, 1>) /* C2PSA tail at c = 64 */                                                  \
  X(FS<4, 1>, FS<2, 2>)                     /* C2PSA head at c = 64 */

// ---------------------------------------------------------------------------------------------------------------- host side
static const int kMT[3] = {1, 2, 4};

extern "C" size_t ey_block_program_bytes(int nstages) { return (size_t)(nstages > 0 ? nstages : 0) * sizeof(ey_block_stage); }
extern "C" size_t ey_block_stage_sizeof(void) { return sizeof(ey_block_stage); }

static int blk_view_ok(int64_t addr, int ext, int cs, int C, const char* what, int si) {
  if (ext >= BLK_MAX_EXT) return ey_set_error(EY_EINVAL, "block stage %d: %s: ext index %d out of range", si, what, ext);
  if (ext < 0 && addr == 0) return ey_set_error(EY_EINVAL, "block stage %d: %s: null pointer", si, what);
  if (addr % 16) return ey_set_error(EY_EINVAL, "block stage %d: %s: not 16-byte aligned", si, what);
  if (cs < C || (cs * 2) % 16 || C % 8) return ey_set_error(EY_EINVAL, "block stage %d: %s: cstride %d / channels %d (multiples of 8, 16-byte pixel stride)", si, what, cs, C);
  return EY_OK;
}

// Validates the stages, fills the derived fields (packing geometry, wave-tile shape) and writes the device image of the program
// into out_host (upload it; ey_block_run takes the device copy).
extern "C" int ey_block_compile(const ey_block_stage* st, int nstages, void* out_host, size_t out_bytes) {
  EY_CHECK(st && out_host && nstages > 0, "block_compile: null / empty program");
  EY_CHECK(out_bytes >= ey_block_program_bytes(nstages), "block_compile: output buffer too small");
  ey_block_stage* o = (ey_block_stage*)out_host;
  for (int i = 0; i < nstages; ++i) {
    ey_block_stage s = st[i];
    EY_CHECK(s.H > 0 && s.W > 0 && s.Ho > 0 && s.Wo > 0 && (long)s.H * s.W <= 4096, "block stage %d: extent %dx%d -> %dx%d (maps up to 4096 pixels)", i, s.H, s.W, s.Ho, s.Wo);
    int rc;
    if ((rc = blk_view_ok(s.src[0], s.src_ext[0], s.src_cs[0], s.src_C[0], "src0", i))) return rc;
    EY_CHECK(s.src_img[0] >= 0 && s.y_img >= 0, "block stage %d: negative image stride", i);
    switch (s.op) {
      case EY_BLK_CONV: {
        EY_CHECK((s.k == 1 || s.k == 3) && (s.stride == 1 || s.stride == 2), "block stage %d: conv k=%d stride=%d", i, s.k, s.stride);
        EY_CHECK(s.Ho == (s.H + 2 * (s.k / 2) - s.k) / s.stride + 1 && s.Wo == (s.W + 2 * (s.k / 2) - s.k) / s.stride + 1, "block stage %d: conv output extent", i);
        EY_CHECK(s.nsrc == 1 || s.nsrc == 2, "block stage %d: nsrc=%d", i, s.nsrc);
        if (s.nsrc == 2 && (rc = blk_view_ok(s.src[1], s.src_ext[1], s.src_cs[1], s.src_C[1], "src1", i))) return rc;
        EY_CHECK(s.w && s.Cout > 0 && s.Cout % 8 == 0, "block stage %d: conv Cout=%d (multiple of 8) / weights", i, s.Cout);
        if ((rc = blk_view_ok(s.y, s.y_ext, s.y_cs, s.Cout, "y", i))) return rc;
        if (s.has_res && (rc = blk_view_ok(s.res, s.res_ext, s.res_cs, s.Cout, "res", i))) return rc;
        if (s.has_addz && (rc = blk_view_ok(s.addz, s.addz_ext, s.addz_cs, s.Cout, "addz", i))) return rc;
        EY_CHECK(!s.has_addz || (s.addz_H > 0 && s.addz_W > 0), "block stage %d: addz extent", i);
        EY_CHECK(!s.bias || ey_aligned(s.bias, 16), "block stage %d: bias alignment", i);
        if (s.ngroup < 1) s.ngroup = 1;
        EY_CHECK(s.ngroup == 1 || s.nsrc == 1, "block stage %d: groups need a single source", i);
        EY_CHECK((s.src_g * 2) % 16 == 0 && (s.y_g * 2) % 16 == 0, "block stage %d: group strides", i);
        int Cin = 0;
        for (int j = 0; j < s.nsrc; ++j) Cin += s.src_C[j];
        s.kpad = ey_conv_kpad(s.k * s.k * Cin, 2);
        s.nt_pack = ey_conv_pack_nt(s.Cout);
        s.zsy = s.has_addz ? (float)s.addz_H / (float)s.Ho : 0.f;
        s.zsx = s.has_addz ? (float)s.addz_W / (float)s.Wo : 0.f;
        if (s.w_gmax < 0) s.w_gmax = 0;
        s.lds = 0;
        {  // pointwise-chain form (block_tile_kernel): the 4 waves of a tile's workgroup split nblk * NT / nti items; widest nti with >= 4 items
          const int NT = s.nt_pack, nblk = (s.Cout + 16 * NT - 1) / (16 * NT);
          s.tile_nti = 0;
          if (s.k == 1 && s.stride == 1 && s.ngroup == 1) {
            const int cand[4] = {5, 4, 2, 1};
            for (int q = 0; q < 4 && !s.tile_nti; ++q)
              if (NT % cand[q] == 0 && (cand[q] != 5 || NT == 5) && (nblk * (NT / cand[q]) >= 4 || cand[q] == 1)) s.tile_nti = cand[q];
          }
        }
        // wave tile (MT pixel tiles x NTI row blocks): operands come fragment-wise through the CU's 64 B/clk vector-memory path, so a
        // round of the 16 waves costs ~(MT + NTI) fragment loads per k-step (the MFMAs hide behind them): fewest rounds x loads wins
        const int M = s.Ho * s.Wo, NT = s.nt_pack, nblk = (s.Cout + 16 * NT - 1) / (16 * NT);
        long best = -1;
        for (int a = 0; a < 3; ++a) {
          for (int nti = 1; nti <= 5; ++nti) {
            const int mt = kMT[a];
            if (NT % nti || nti == 3 || mt * nti > 8 || (nti == 5 && mt > 1)) continue;  // (the instantiated wave tiles: <= 8 accumulator blocks, 128 VGPRs)
            const long items = (long)s.ngroup * ((M + 16 * mt - 1) / (16 * mt)) * nblk * (NT / nti);
            const long rounds = (items + BLK_WAVES - 1) / BLK_WAVES;
            const long cost = rounds * (mt + nti) * 16 + mt * nti;
            if (best < 0 || cost < best) { best = cost; s.mt = mt; s.nti = nti; }
          }
        }
        break;
      }
      case EY_BLK_DW:
        EY_CHECK((s.k == 3 || s.k == 5 || s.k == 7) && s.w && s.Ho == s.H && s.Wo == s.W, "block stage %d: depthwise k=%d", i, s.k);
        if ((rc = blk_view_ok(s.y, s.y_ext, s.y_cs, s.src_C[0], "y", i))) return rc;
        EY_CHECK(ey_aligned(s.w, 16), "block stage %d: depthwise weights alignment", i);
        break;
      case EY_BLK_DWT:
        EY_CHECK(s.H >= 2 && s.W >= 2 && s.Ho == s.H / 2 && s.Wo == s.W / 2, "block stage %d: dwt extent", i);
        if ((rc = blk_view_ok(s.y, s.y_ext, s.y_cs, 4 * s.src_C[0], "y", i))) return rc;
        break;
      case EY_BLK_POOL:
        EY_CHECK(s.Ho == s.H && s.Wo == s.W && (long)s.H * s.W * 16 * 2 <= BLK_LDS_BYTES, "block stage %d: pool map %dx%d does not fit LDS", i, s.H, s.W);
        if ((rc = blk_view_ok(s.y, s.y_ext, s.y_cs, 3 * s.src_C[0], "y", i))) return rc;
        break;
      case EY_BLK_LINATTN:
        EY_CHECK(s.heads > 0 && s.heads % 2 == 0 && s.Cout == 64 * s.heads && s.src_C[0] == 3 * s.Cout, "block stage %d: linear attention needs an even number of 64-channel heads", i);
        EY_CHECK(2 * sizeof(LinAttnLds) <= BLK_LDS_BYTES, "block stage %d: LDS", i);
        if ((rc = blk_view_ok(s.y, s.y_ext, s.y_cs, s.Cout, "y", i))) return rc;
        break;
      default:
        return ey_set_error(EY_EINVAL, "block stage %d: unknown op %d", i, s.op);
    }
    o[i] = s;
  }
  // ---- pointwise-chain lowering (block_tile_kernel): tensors that only the chain touches (absolute refs produced by a stage) live in
  // LDS, one row of C + 8 halves per pixel of the 32-pixel tile; everything else stays in global memory
  {
    struct Own { int64_t addr; int cs, C, lds, lcs; };
    Own own[TILE_MAX_STAGES];
    int nown = 0;
    long top = 0;
    bool ok = nstages <= TILE_MAX_STAGES;
    for (int i = 0; i < nstages && ok; ++i) {
      ey_block_stage& s = o[i];
      if (s.op != EY_BLK_CONV || s.tile_nti == 0) { ok = false; break; }
      auto find = [&](int64_t addr, int ext, int cs, int& lds, int& lcs) {
        lds = -1; lcs = 0;
        if (ext >= 0) return;
        for (int q = 0; q < nown; ++q)
          if (own[q].cs == cs && addr >= own[q].addr && addr < own[q].addr + (int64_t)own[q].C * 2) {
            lds = own[q].lds + (int)((addr - own[q].addr) / 2);
            lcs = own[q].lcs;
          }
      };
      for (int j = 0; j < 2; ++j) {
        s.tile_src_lds[j] = -1; s.tile_src_lcs[j] = 0;
        if (j < s.nsrc) find(s.src[j], s.src_ext[j], s.src_cs[j], s.tile_src_lds[j], s.tile_src_lcs[j]);
      }
      s.tile_res_lds = -1; s.tile_res_lcs = 0;
      if (s.has_res) find(s.res, s.res_ext, s.res_cs, s.tile_res_lds, s.tile_res_lcs);
      s.tile_y_lds = -1; s.tile_y_lcs = 0;
      if (s.y_ext < 0) {  // an intermediate the caller never sees
        int lds, lcs;
        find(s.y, s.y_ext, s.y_cs, lds, lcs);
        if (lds >= 0) { s.tile_y_lds = lds; s.tile_y_lcs = lcs; }  // (written into a slice of an earlier intermediate)
        else {
          Own w; w.addr = s.y; w.cs = s.y_cs; w.C = s.Cout; w.lcs = s.Cout + 8; w.lds = (int)top;
          top += (long)TILE_PX * w.lcs;
          own[nown++] = w;
          s.tile_y_lds = w.lds; s.tile_y_lcs = w.lcs;
        }
      }
    }
    o[0].tile_lds_bytes = (ok && top * 2 <= 56 * 1024) ? (int32_t)(top * 2) : -1;
  }
  return EY_OK;
}

// which executor the last launch on this thread took (EY_BLK_RAN_*): a fallback is visible to tools and tests
static thread_local int g_blk_last_variant = 0;
extern "C" int ey_block_last_variant(void) { return g_blk_last_variant; }

static int block_launch(const void* program_dev, int nstages, int B, const void* const* ext_ptrs_host, int next, long long* tstamps, ey_stream_t stream) {
  EY_CHECK(program_dev && nstages > 0 && B > 0, "block_run: null / empty program");
  EY_CHECK(next >= 0 && next <= BLK_MAX_EXT && (next == 0 || ext_ptrs_host), "block_run: %d external tensors (0..%d)", next, BLK_MAX_EXT);
  BlkExt ext;
  for (int i = 0; i < BLK_MAX_EXT; ++i) {
    ext.p[i] = i < next ? (char*)const_cast<void*>(ext_ptrs_host[i]) : nullptr;
    EY_CHECK(i >= next || (ext.p[i] && ey_aligned(ext.p[i], 16)), "block_run: external tensor %d null / not 16-byte aligned", i);
  }
  static bool attr_done = false;
  if (!attr_done) {
    if (hipFuncSetAttribute((const void*)block_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, BLK_LDS_BYTES) != hipSuccess)
      return ey_set_error(EY_ELAUNCH, "block_run: cannot reserve %d B of LDS", BLK_LDS_BYTES);
    attr_done = true;
  }
  hipLaunchKernelGGL(block_kernel, dim3(B), dim3(BLK_THREADS), BLK_LDS_BYTES, (hipStream_t)stream, (const BlkStage*)program_dev, nstages, ext, tstamps);
  EY_LAUNCH_CHECK("ey_block_run");
  g_blk_last_variant = EY_BLK_RAN_IMAGE;
  return EY_OK;
}

extern "C" int ey_block_run(const void* program_dev, int nstages, int B, const void* const* ext_ptrs_host, int next, ey_stream_t stream) {
  return block_launch(program_dev, nstages, B, ext_ptrs_host, next, nullptr, stream);
}

// Pointwise-chain form: every stage must be tile-executable (ey_block_tileable on the compiled program) and share the map H x W.
extern "C" int ey_block_tileable(const ey_block_stage* compiled_host, int nstages) {
  if (!compiled_host || nstages <= 0 || nstages > TILE_MAX_STAGES || compiled_host[0].tile_lds_bytes < 0) return 0;
  for (int i = 0; i < nstages; ++i) {
    const ey_block_stage& s = compiled_host[i];
    if (s.op != EY_BLK_CONV || s.tile_nti == 0 || s.Ho != compiled_host[0].Ho || s.Wo != compiled_host[0].Wo || s.H != s.Ho || s.W != s.Wo) return 0;
  }
  return 1;
}
extern "C" int ey_block_run_tiles(const void* program_dev, int nstages, int B, int H, int W, int lds_bytes, const void* const* ext_ptrs_host, int next,
                                  ey_stream_t stream) {
  EY_CHECK(program_dev && nstages > 0 && nstages <= TILE_MAX_STAGES && B > 0 && H > 0 && W > 0 && lds_bytes >= 0 && lds_bytes <= 56 * 1024,
           "block_run_tiles: bad program (%d stages, %d B of LDS)", nstages, lds_bytes);
  EY_CHECK(next >= 0 && next <= BLK_MAX_EXT && (next == 0 || ext_ptrs_host), "block_run_tiles: %d external tensors (0..%d)", next, BLK_MAX_EXT);
  BlkExt ext;
  for (int i = 0; i < BLK_MAX_EXT; ++i) {
    ext.p[i] = i < next ? (char*)const_cast<void*>(ext_ptrs_host[i]) : nullptr;
    EY_CHECK(i >= next || (ext.p[i] && ey_aligned(ext.p[i], 16)), "block_run_tiles: external tensor %d null / not 16-byte aligned", i);
  }
  const int mtiles = (H * W + TILE_PX - 1) / TILE_PX;
  EY_CHECK(B <= 65535, "block_run_tiles: batch %d", B);
  const size_t lds = TILE_MAX_STAGES * sizeof(TStage) + (size_t)lds_bytes;
  hipLaunchKernelGGL(block_tile_kernel, dim3((unsigned)mtiles, (unsigned)B), dim3(256), lds, (hipStream_t)stream, (const BlkStage*)program_dev, nstages, ext);
  EY_LAUNCH_CHECK("ey_block_run_tiles");
  g_blk_last_variant = EY_BLK_RAN_TILE;
  return EY_OK;
}
// ---- register-weight chains (block_chain_kernel): plan on the host, where the stage list is known
template <class... S>
static constexpr uint32_t fast_sig() {
  uint32_t sig = 0;
  int sh = 0;
  ((sig |= (uint32_t)S::code << sh, sh += 8), ...);
  return sig;
}
static bool fast_sig_known(uint32_t sig) {
#define EY_X(...) if (sig == fast_sig<__VA_ARGS__>()) return true;
  FAST_CHAINS(EY_X)
#undef EY_X
  return false;
}
static int fast_pitch(int C) {  // LDS pixel pitch (elements): 2 (mod 4) 16-byte units, conflict-free fragment reads (as pwn_launch)
  int units = C >> 3;
  while ((units & 3) != 2) ++units;
  return units * 8;
}

extern "C" size_t ey_block_fast_plan_bytes(void) { return sizeof(FPlan); }

// Eligibility + lowering of a compiled, tileable program for block_chain_kernel.  1: plan_host holds the plan; 0: not eligible (the
// program keeps block_tile_kernel).  Pure host function of the stage list.
extern "C" int ey_block_fast_plan(const ey_block_stage* cs, int nstages, void* plan_host, size_t plan_bytes) {
  if (!cs || !plan_host || plan_bytes < sizeof(FPlan) || nstages > FAST_MAX_STAGES || !ey_block_tileable(cs, nstages)) return 0;
  FPlan p;
  memset(&p, 0, sizeof(p));
  p.nstages = nstages;
  p.M = cs[0].Ho * cs[0].Wo;
  for (int u = 0; u < FAST_MAX_SLOTS; ++u) { p.slot[u].ext = -1; p.slot[u].cv = 1; }  // unused rounds: an empty buffer
  for (int i = 0; i < FAST_MAX_STAGES; ++i) p.st[i].bias_lds = -1;
  // ---- shapes: pointwise, no addz, 32-channel sources, whole packed block tiles, an instantiated (k-steps, row blocks per wave) list
  uint32_t sig = 0;
  for (int i = 0; i < nstages; ++i) {
    const ey_block_stage& s = cs[i];
    if (s.k != 1 || s.stride != 1 || s.ngroup != 1 || s.has_addz || s.Cout > 512 || s.Cout % (16 * s.nt_pack)) return 0;
    int K = 0;
    for (int j = 0; j < s.nsrc; ++j) {
      if (s.src_C[j] % 32) return 0;
      K += s.src_C[j];
    }
    const int ks = K / 32, nrw = (s.Cout / 16 + FAST_WAVES - 1) / FAST_WAVES;
    if (ks > 31 || nrw > 7) return 0;
    sig |= (uint32_t)(ks * 8 + nrw) << (8 * i);
  }
  if (!fast_sig_known(sig)) return 0;  // (the per-wave fragment budget: only the instantiated lists fit the register file by construction)
  p.sig = (int32_t)sig;
  // ---- LDS tensors: overlapping channel ranges of one pixel row (same tensor, pixel stride and image stride) are ONE buffer
  struct Buf { int ext, cs, fw, lr, lds, pitch; int64_t img, lo, hi; uint64_t valid, pre; bool read; };
  struct Ref { int ext, cs, C; int64_t addr, img; };
  Buf buf[16];
  int nbuf = 0;
  auto touch = [&](const Ref& r) -> bool {
    if (nbuf >= 16) return false;
    Buf n;
    memset(&n, 0, sizeof(n));
    n.ext = r.ext; n.cs = r.cs; n.img = r.img; n.lo = r.addr; n.hi = r.addr + 2 * (int64_t)r.C; n.fw = 99; n.lr = -1; n.lds = -1;
    buf[nbuf++] = n;
    for (bool again = true; again;) {  // merge until no two buffers of one tensor overlap
      again = false;
      for (int a = 0; a < nbuf && !again; ++a)
        for (int c = a + 1; c < nbuf && !again; ++c) {
          Buf &u = buf[a], &o = buf[c];
          if (u.ext != o.ext || u.cs != o.cs || u.img != o.img || u.lo >= o.hi || o.lo >= u.hi) continue;
          u.lo = u.lo < o.lo ? u.lo : o.lo;
          u.hi = u.hi > o.hi ? u.hi : o.hi;
          buf[c] = buf[--nbuf];
          again = true;
        }
    }
    return true;
  };
  auto src_ref = [&](const ey_block_stage& s, int j) { Ref r = {s.src_ext[j], s.src_cs[j], s.src_C[j], s.src[j], s.src_img[j]}; return r; };
  auto res_ref = [&](const ey_block_stage& s) { Ref r = {s.res_ext, s.res_cs, s.Cout, s.res, s.res_img}; return r; };
  auto y_ref = [&](const ey_block_stage& s) { Ref r = {s.y_ext, s.y_cs, s.Cout, s.y, s.y_img}; return r; };
  for (int i = 0; i < nstages; ++i) {
    const ey_block_stage& s = cs[i];
    for (int j = 0; j < s.nsrc; ++j) if (!touch(src_ref(s, j))) return 0;
    if (s.has_res && !touch(res_ref(s))) return 0;
    if (!touch(y_ref(s))) return 0;
  }
  auto find = [&](const Ref& r) -> int {
    for (int q = 0; q < nbuf; ++q)
      if (buf[q].ext == r.ext && buf[q].cs == r.cs && buf[q].img == r.img && r.addr >= buf[q].lo && r.addr + 2 * (int64_t)r.C <= buf[q].hi) return q;
    return -1;
  };
  auto mask = [&](const Buf& u, const Ref& r) -> uint64_t {  // the 8-channel units of r inside u
    const int u0 = (int)((r.addr - u.lo) / 16), n = r.C / 8;
    return (n >= 64 ? ~0ull : ((1ull << n) - 1)) << u0;
  };
  for (int q = 0; q < nbuf; ++q)
    if ((buf[q].hi - buf[q].lo) > 2 * (int64_t)buf[q].cs || (buf[q].hi - buf[q].lo) > 64 * 16 || (buf[q].lo % 16)) return 0;  // one pixel row, <= 512 channels
  // ---- walk the stages: what is read before the chain wrote it comes from global memory (preload); lifetimes for the LDS placement
  for (int i = 0; i < nstages; ++i) {
    const ey_block_stage& s = cs[i];
    const Ref yr = y_ref(s);
    const int yb = find(yr);
    if (yb < 0) return 0;
    const uint64_t ym = mask(buf[yb], yr);
    auto rd = [&](const Ref& r, bool is_res) -> bool {
      const int q = find(r);
      if (q < 0) return false;
      Buf& u = buf[q];
      const uint64_t m = mask(u, r);
      if (q == yb && (m & ym) && !(is_res && m == ym)) return false;  // in-place over a source: other waves still read it (a residual of the same range is the lane's own)
      const uint64_t need = m & ~u.valid;
      if (need) { u.pre |= need; u.valid |= need; u.fw = -1; }
      u.read = true;
      if (u.lr < i) u.lr = i;
      return true;
    };
    for (int j = 0; j < s.nsrc; ++j) if (!rd(src_ref(s, j), false)) return 0;
    if (s.has_res && !rd(res_ref(s), true)) return 0;
    Buf& u = buf[yb];
    u.valid |= ym;
    if (u.fw > i) u.fw = i;
    if (u.lr < i) u.lr = i;
  }
  // ---- placement: largest first, first fit among the buffers whose lifetimes overlap (a buffer last read in stage s may be
  // overwritten from the epilogue of stage s + 1 on: a barrier lies between)
  int order[16], nord = 0;
  for (int q = 0; q < nbuf; ++q) {
    Buf& u = buf[q];  // (an output nobody in the chain reads included: its epilogue goes through LDS on the way to global memory)
    u.pitch = fast_pitch((int)((u.hi - u.lo) / 2));
    order[nord++] = q;
  }
  for (int a = 0; a < nord; ++a)
    for (int c = a + 1; c < nord; ++c)
      if (buf[order[c]].pitch > buf[order[a]].pitch) { const int t = order[a]; order[a] = order[c]; order[c] = t; }
  long top = 0;
  for (int a = 0; a < nord; ++a) {
    Buf& u = buf[order[a]];
    const long size = (long)FAST_PX * u.pitch;
    long best = -1;
    for (int c = -1; c < a; ++c) {  // candidate offsets: 0 and the end of every placed buffer
      const long off = c < 0 ? 0 : buf[order[c]].lds + (long)FAST_PX * buf[order[c]].pitch;
      bool ok = true;
      for (int d = 0; d < a && ok; ++d) {
        const Buf& o = buf[order[d]];
        const bool live = !(o.lr < u.fw || u.lr < o.fw);
        if (live && off < o.lds + (long)FAST_PX * o.pitch && o.lds < off + size) ok = false;
      }
      if (ok && (best < 0 || off < best)) best = off;
    }
    u.lds = (int)best;
    if (best + size > top) top = best + size;
  }
  // ---- preload jobs: runs of units read before written
  for (int q = 0; q < nbuf; ++q) {
    const Buf& u = buf[q];
    for (int b0 = 0; b0 < 64;) {
      if (!((u.pre >> b0) & 1)) { ++b0; continue; }
      int b1 = b0;
      while (b1 < 64 && ((u.pre >> b1) & 1)) ++b1;
      if (p.njobs >= FAST_MAX_JOBS || u.lds < 0) return 0;
      FJob jb;
      memset(&jb, 0, sizeof(jb));
      jb.addr = u.lo + 16 * (int64_t)b0; jb.img = u.img; jb.ext = u.ext; jb.cs = u.cs;
      jb.cv = b1 - b0; jb.C = 8 * jb.cv; jb.inv = ((1 << 20) + jb.cv - 1) / jb.cv; jb.nv = FAST_PX * jb.cv;
      jb.lds = u.lds + 8 * b0; jb.pitch = u.pitch;
      jb.bytes = (int32_t)((((long)p.M - 1) * jb.cs + jb.C) * 2);
      if (jb.cv < 2) return 0;
      for (int v0 = 0; v0 < jb.nv; v0 += 512) {
        if (p.nslot >= FAST_MAX_SLOTS) return 0;
        jb.v0 = v0;
        p.slot[p.nslot++] = jb;
      }
      ++p.njobs;
      b0 = b1;
    }
  }
  // ---- stages
  p.bias_base = (int32_t)((top + 7) / 8 * 8);
  int nbias = 0;
  for (int i = 0; i < nstages; ++i) {
    const ey_block_stage& s = cs[i];
    FStage& t = p.st[i];
    t.w = reinterpret_cast<const f16*>(s.w); t.bias = s.bias;
    t.y = s.y; t.y_img = s.y_img; t.y_ext = s.y_ext; t.y_cs = s.y_cs;
    t.y_glob = s.y_ext >= 0;
    const Ref yr = y_ref(s);
    const Buf& yb = buf[find(yr)];
    t.y_lds = -1; t.y_pitch = 0;
    if (yb.lds < 0) return 0;
    t.y_lds = yb.lds + (int)((yr.addr - yb.lo) / 2); t.y_pitch = yb.pitch;
    t.res_lds = -1; t.res_pitch = 0;
    if (s.has_res) {
      const Ref rr = res_ref(s);
      const Buf& rb = buf[find(rr)];
      if (rb.lds < 0) return 0;
      t.res_lds = rb.lds + (int)((rr.addr - rb.lo) / 2); t.res_pitch = rb.pitch;
    }
    for (int j = 0; j < 2; ++j) { t.src_lds[j] = 0; t.src_pitch[j] = 0; }
    for (int j = 0; j < s.nsrc; ++j) {
      const Ref sr = src_ref(s, j);
      const Buf& sb = buf[find(sr)];
      if (sb.lds < 0) return 0;
      t.src_lds[j] = sb.lds + (int)((sr.addr - sb.lo) / 2); t.src_pitch[j] = sb.pitch;
    }
    t.nks0 = s.src_C[0] / 32;
    t.bias_lds = -1;
    if (s.bias) { t.bias_lds = nbias; t.bias_bytes = 4 * s.Cout; nbias += s.Cout; }
    t.kpad = s.kpad; t.nt = s.nt_pack; t.nrb = s.Cout / 16; t.Cout = s.Cout; t.act = s.act; t.out_scale = s.out_scale;
  }
  const long bytes = (long)p.bias_base * 2 + (long)nbias * 4;
  if (bytes > FAST_LDS_MAX) return 0;
  p.lds_bytes = (int32_t)bytes;
  memcpy(plan_host, &p, sizeof(p));
  return 1;
}

template <class... S>
static int chain_launch(const FPlan& p, int B, hipStream_t st) {
  const size_t lds = (size_t)p.lds_bytes;
  if (!ey_lds_reserve<block_chain_kernel<S...>>(lds)) return ey_set_error(EY_ELAUNCH, "block_run_chain: cannot reserve %zu B of LDS", lds);
  hipLaunchKernelGGL((block_chain_kernel<S...>), dim3((unsigned)((p.M + FAST_PX - 1) / FAST_PX), (unsigned)B), dim3(512), lds, st, p);
  return EY_OK;
}

// ey_block_run_tiles with a plan: plan_host = what ey_block_fast_plan filled for this program, or NULL.  With a plan and the tunable
// chain_fast != 0 the program runs on block_chain_kernel, otherwise on block_tile_kernel; ey_block_last_variant tells which.
extern "C" int ey_block_run_chain(const void* program_dev, int nstages, int B, int H, int W, int lds_bytes, const void* plan_host,
                                  const void* const* ext_ptrs_host, int next, ey_stream_t stream) {
  if (!plan_host || tune().chain_fast == 0) return ey_block_run_tiles(program_dev, nstages, B, H, W, lds_bytes, ext_ptrs_host, next, stream);
  FPlan p;
  memcpy(&p, plan_host, sizeof(p));
  EY_CHECK(B > 0 && B <= 65535 && H > 0 && W > 0 && p.nstages == nstages && p.M == H * W && p.lds_bytes > 0 && p.lds_bytes <= FAST_LDS_MAX &&
               p.njobs >= 0 && p.njobs <= FAST_MAX_JOBS && p.nslot >= 0 && p.nslot <= FAST_MAX_SLOTS,
           "block_run_chain: the plan does not belong to this program (%d stages, %dx%d)", nstages, H, W);
  EY_CHECK(next >= 0 && next <= BLK_MAX_EXT && (next == 0 || ext_ptrs_host), "block_run_chain: %d external tensors (0..%d)", next, BLK_MAX_EXT);
  BlkExt ext;
  for (int i = 0; i < BLK_MAX_EXT; ++i) {
    ext.p[i] = i < next ? (char*)const_cast<void*>(ext_ptrs_host[i]) : nullptr;
    EY_CHECK(i >= next || (ext.p[i] && ey_aligned(ext.p[i], 16)), "block_run_chain: external tensor %d null / not 16-byte aligned", i);
  }
  // the kernel takes absolute addresses: (index, byte offset) references are bound to this call's external tensors here
  for (int u = 0; u < FAST_MAX_SLOTS; ++u) {
    EY_CHECK(p.slot[u].ext < next, "block_run_chain: the plan names external tensor %d of %d", p.slot[u].ext, next);
    if (p.slot[u].ext >= 0) p.slot[u].addr += (int64_t)(uintptr_t)ext.p[p.slot[u].ext];
  }
  for (int i = 0; i < FAST_MAX_STAGES; ++i) {
    EY_CHECK(p.st[i].y_ext < next, "block_run_chain: the plan names external tensor %d of %d", p.st[i].y_ext, next);
    if (p.st[i].y_glob && p.st[i].y_ext >= 0) p.st[i].y += (int64_t)(uintptr_t)ext.p[p.st[i].y_ext];
  }
  int rc = EY_EINVAL;
  bool found = false;
#define EY_X(...) if (!found && (uint32_t)p.sig == fast_sig<__VA_ARGS__>()) { found = true; rc = chain_launch<__VA_ARGS__>(p, B, (hipStream_t)stream); }
  FAST_CHAINS(EY_X)
#undef EY_X
  EY_CHECK(found, "block_run_chain: no kernel for chain signature %#x", (unsigned)p.sig);
  if (rc != EY_OK) return rc;
  EY_LAUNCH_CHECK("ey_block_run_chain");
  g_blk_last_variant = EY_BLK_RAN_CHAIN;
  return EY_OK;
}
// developer tool: same launch; workgroup 0 also writes wall_clock64() (100 MHz) at the start and after every stage into tstamps_dev[nstages + 1]
extern "C" int ey_block_run_timed(const void* program_dev, int nstages, int B, const void* const* ext_ptrs_host, int next, long long* tstamps_dev, ey_stream_t stream) {
  EY_CHECK(tstamps_dev, "block_run_timed: null timestamp buffer");
  return block_launch(program_dev, nstages, B, ext_ptrs_host, next, tstamps_dev, stream);
}
