// Instance segmentation (reference ultralytics/utils/ops.py:644-693 process_mask / crop_mask, nn/modules/block.py:112-129 Proto).
//
// ey_process_mask: per kept detection n, mask[n] = (bilinear_up_s(crop(coef_n . proto)) > 0) as uint8.  The eager form writes the
// low-resolution product, the cropped copy and an fp32 full-resolution map before the compare; here a workgroup owns (detection, band of
// 32 output rows), walks the band in 256-column tiles, keeps the low-resolution values a tile needs (+ a one-pixel ring) in LDS as fp32 and
// writes only the result bytes, 16 per store.  Tiles the cropped box cannot reach are stored as zeros without touching proto.  No atomics,
// fixed summation order (k ascending fmaf chain): the output is the same run to run.
//
// ey_process_mask_native (reference utils/ops.py:696-737 process_mask_native / scale_masks): the same product resized to each ORIGINAL image
// at any ratio, cropped after the resize; see the kernel below.
//
// ey_deconv2x2: dense ConvTranspose2d(Cin, Cout, 2, 2) + bias as ONE GEMM [pixels x Cin] . [Cin x 4 Cout] whose epilogue scatters the four
// (di, dj) positions.  A wave owns 64 pixels (4 MFMA tiles) and sweeps the packed weight rows 64 at a time.
#include "common.h"
#include "mask_source.h"

#define PM_TH 32    // output rows per band (work item)
#define PM_TW 256   // output columns per tile
#define PM_MAXNM 64
#define PM_MAXLV 4

struct pm_levels {
  const void* coef[PM_MAXLV];
  int cs[PM_MAXLV], H[PM_MAXLV], W[PM_MAXLV];
  int n;
};

// 16 result bytes at out[0..15] (columns ox .. ox+15 of a row iw wide): one 16-byte store where the row allows it
__device__ __forceinline__ void pm_store16(uint8_t* out, const ey_u32x4& v, int ox, int iw, bool vec) {
  if (vec && ox + 16 <= iw) {
    *reinterpret_cast<ey_u32x4*>(out) = v;
  } else {
    for (int e = 0; e < 16 && ox + e < iw; ++e) out[e] = (uint8_t)((v[e >> 2] >> (8 * (e & 3))) & 0xffu);
  }
}

template <typename T>
__global__ __launch_bounds__(256) void process_mask_kernel(int B, int mh, int mw, int nm, const T* __restrict__ proto, int pcs, bool pvec, pm_levels lv,
                                                           int coef_f32, int nbands, const int* __restrict__ rows, const float* __restrict__ boxes, int s,
                                                           uint8_t* __restrict__ out, bool ovec) {
  // low-resolution tile: rows ry0 .. ry0 + TR - 1, columns cx0 .. cx0 + TC - 1 (largest at s = 1: 34 x 258)
  __shared__ float tile[(PM_TH + 2) * (PM_TW + 2)];
  __shared__ float coef[PM_MAXNM];
  const int tid = threadIdx.x;
  const long item = blockIdx.x;
  const int n = (int)(item / nbands), band = (int)(item % nbands);
  const int ih = mh * s, iw = mw * s;
  const int oy0 = band * PM_TH;
  uint8_t* o = out + (long)n * ih * iw;

  // ---- the detection: image, anchor -> level and pixel of the coefficient maps
  const int img = rows[2 * n], a = rows[2 * n + 1];
  int lvl = -1, pix = 0;
  if (img >= 0 && img < B && a >= 0) {
    int rem = a;
    for (int l = 0; l < lv.n; ++l) {
      const int hw = lv.H[l] * lv.W[l];
      if (rem < hw) { lvl = l; pix = rem; break; }
      rem -= hw;
    }
  }
  const bool valid = lvl >= 0;
  const float inv = 1.f / (float)s;  // (a power of two: exact)
  // crop_mask on the low-resolution grid: r >= x1, r < x2, c >= y1, c < y2 with the box scaled in fp32
  float x1 = 0.f, y1 = 0.f, x2 = 0.f, y2 = 0.f;
  if (valid) {
    x1 = boxes[4 * n] * inv; y1 = boxes[4 * n + 1] * inv; x2 = boxes[4 * n + 2] * inv; y2 = boxes[4 * n + 3] * inv;
    if (tid < nm) {
      const long off = ((long)img * lv.H[lvl] * lv.W[lvl] + pix) * lv.cs[lvl] + tid;
      coef[tid] = coef_f32 ? ((const float*)lv.coef[lvl])[off] : (float)((const f16*)lv.coef[lvl])[off];
    }
  }
  // integer footprint of the crop (only used to skip work; the comparisons above decide every pixel).  NaN corners give an empty one.
  const int fx_lo = (int)ceilf(fminf(fmaxf(x1, 0.f), (float)mw)), fx_hi = (int)ceilf(fminf(fmaxf(x2, 0.f), (float)mw));
  const int fy_lo = (int)ceilf(fminf(fmaxf(y1, 0.f), (float)mh)), fy_hi = (int)ceilf(fminf(fmaxf(y2, 0.f), (float)mh));
  const int TR = PM_TH / s + 2, TC = PM_TW / s + 2;
  const int ry0 = oy0 / s - 1;
  // low-resolution rows this band reads: ry0 .. ry0 + TR - 1
  const bool band_live = valid && fx_lo < fx_hi && fy_lo < fy_hi && ry0 + TR - 1 >= fy_lo && ry0 < fy_hi;

  for (int ox0 = 0; ox0 < iw; ox0 += PM_TW) {
    const int cx0 = ox0 / s - 1;
    const bool live = band_live && cx0 + TC - 1 >= fx_lo && cx0 < fx_hi;  // (workgroup-uniform)
    if (live) {
      __syncthreads();  // coef is written; the previous tile's readers are done
      for (int idx = tid; idx < TR * TC; idx += 256) {
        const int r = ry0 + idx / TC, c = cx0 + idx % TC;
        float v = 0.f;
        if (r >= 0 && r < mh && c >= 0 && c < mw) {
          const float fc = (float)c, fr = (float)r;
          if (fc >= x1 && fc < x2 && fr >= y1 && fr < y2) {
            const T* p = proto + (((long)img * mh + r) * mw + c) * pcs;
            if (pvec) {
              for (int k = 0; k < nm; k += 8) {
                Vec8<T> q;
                q.load(p + k);
#pragma unroll
                for (int e = 0; e < 8; ++e) v = __builtin_fmaf(coef[k + e], q.get(e), v);
              }
            } else {
              for (int k = 0; k < nm; ++k) v = __builtin_fmaf(coef[k], to_f(p[k]), v);
            }
          }
        }
        tile[idx] = v;
      }
      __syncthreads();
    }
    // ---- output: a thread owns 16 consecutive columns of a row; consecutive lanes, consecutive 16-byte groups
    for (int g = tid; g < PM_TH * (PM_TW / 16); g += 256) {
      const int oy = oy0 + g / (PM_TW / 16), ox = ox0 + (g % (PM_TW / 16)) * 16;
      if (oy >= ih || ox >= iw) continue;
      ey_u32x4 bits = (ey_u32x4)0u;
      if (live) {
        if (s == 1) {
          const float* t = &tile[(oy - ry0) * TC + (ox - cx0)];
          for (int e = 0; e < 16 && ox + e < iw; ++e) bits[e >> 2] |= (t[e] > 0.f ? 1u : 0u) << (8 * (e & 3));
        } else {
          // bilinear, align_corners=False: source = (dst + 0.5) / s - 0.5 clamped at 0, upper neighbour clamped to the map
          const float sy = fmaxf(((float)oy + 0.5f) * inv - 0.5f, 0.f);
          const int yl = (int)sy, yh = min(yl + 1, mh - 1);
          const float ly = sy - (float)yl;
          const float* t0 = &tile[(yl - ry0) * TC - cx0];
          const float* t1 = &tile[(yh - ry0) * TC - cx0];
          for (int e = 0; e < 16 && ox + e < iw; ++e) {
            const float sx = fmaxf(((float)(ox + e) + 0.5f) * inv - 0.5f, 0.f);
            const int xl = (int)sx, xh = min(xl + 1, mw - 1);
            const float lx = sx - (float)xl;
            const float top = (1.f - lx) * t0[xl] + lx * t0[xh], bot = (1.f - lx) * t1[xl] + lx * t1[xh];
            const float v = (1.f - ly) * top + ly * bot;
            bits[e >> 2] |= (v > 0.f ? 1u : 0u) << (8 * (e & 3));
          }
        }
      }
      pm_store16(o + (long)oy * iw + ox, bits, ox, iw, ovec);
    }
  }
}

extern "C" int ey_process_mask(int dtype, int B, int mh, int mw, int nm, const void* proto, int proto_cstride, int nlevels, const void* const* coef,
                               int coef_dtype, const int* coef_cstride, const int* H, const int* W, int N, const int* rows, const float* boxes, int s,
                               uint8_t* out, ey_stream_t stream) {
  EY_CHECK(dtype == EY_F16 || dtype == EY_F32, "process_mask: bad dtype");
  EY_CHECK(coef_dtype == EY_F16 || coef_dtype == EY_F32, "process_mask: bad coefficient dtype");
  if (s != 1 && s != 2 && s != 4 && s != 8) return ey_set_error(EY_EUNSUPPORTED, "process_mask: s=%d (1, 2, 4 and 8 are built)", s);
  if (nm < 8 || nm > PM_MAXNM || nm % 8) return ey_set_error(EY_EUNSUPPORTED, "process_mask: nm=%d (multiples of 8 up to %d are built)", nm, PM_MAXNM);
  if (nlevels < 1 || nlevels > PM_MAXLV) return ey_set_error(EY_EUNSUPPORTED, "process_mask: %d coefficient levels (1 to %d are built)", nlevels, PM_MAXLV);
  EY_CHECK(N >= 0 && B > 0 && mh > 0 && mw > 0 && proto_cstride >= nm, "process_mask: B=%d mh=%d mw=%d nm=%d N=%d", B, mh, mw, nm, N);
  if (N == 0) return EY_OK;
  EY_CHECK(proto && coef && coef_cstride && H && W && rows && boxes && out, "process_mask: null pointer");
  pm_levels lv;
  lv.n = nlevels;
  long A = 0;
  for (int l = 0; l < PM_MAXLV; ++l) {
    const bool on = l < nlevels;
    EY_CHECK(!on || (coef[l] && H[l] > 0 && W[l] > 0 && coef_cstride[l] >= nm), "process_mask: level %d is empty", l);
    lv.coef[l] = on ? coef[l] : nullptr;
    lv.cs[l] = on ? coef_cstride[l] : 0;
    lv.H[l] = on ? H[l] : 0;
    lv.W[l] = on ? W[l] : 0;
    if (on) A += (long)H[l] * W[l];
  }
  const long ih = (long)mh * s, iw = (long)mw * s;
  if (A >= (1L << 31) || ih >= (1L << 24) || iw >= (1L << 24)) return ey_set_error(EY_EUNSUPPORTED, "process_mask: map too large");
  const int nbands = ey_cdiv(ih, PM_TH);
  const long items = (long)N * nbands;
  if (items >= (1L << 31)) return ey_set_error(EY_EUNSUPPORTED, "process_mask: %ld work items", items);
  const size_t es = dtype == EY_F16 ? 2 : 4;
  const bool pvec = ey_aligned(proto, 16) && ((size_t)proto_cstride * es) % 16 == 0;
  const bool ovec = ey_aligned(out, 16) && iw % 16 == 0;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == EY_F16)
    hipLaunchKernelGGL((process_mask_kernel<f16>), dim3((unsigned)items), dim3(256), 0, st, B, mh, mw, nm, (const f16*)proto, proto_cstride, pvec, lv,
                       coef_dtype == EY_F32, nbands, rows, boxes, s, out, ovec);
  else
    hipLaunchKernelGGL((process_mask_kernel<float>), dim3((unsigned)items), dim3(256), 0, st, B, mh, mw, nm, (const float*)proto, proto_cstride, pvec, lv,
                       coef_dtype == EY_F32, nbands, rows, boxes, s, out, ovec);
  EY_LAUNCH_CHECK("ey_process_mask");
  return EY_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// ey_process_mask_native (reference utils/ops.py:696-737 process_mask_native + scale_masks, behind retina_masks=True in
// models/yolo/segment/predict.py:48-50): the product, scale_masks' crop, the bilinear resize to the ORIGINAL image (any ratio, up or down),
// crop_mask on the resized map and the compare, for the kept detections of a whole batch whose images may all have different originals.
// A workgroup owns (detection, band of th output rows) and walks the band in tiles of tw columns; th x tw is 32 x 256 and shrinks per
// image with the ratio (pn_plan) so that the low-resolution rows and columns a tile blends fit the LDS tile, which holds them as fp32;
// the per-column source index and weight of a tile sit in LDS too, the per-row ones in registers.  Only the part of a tile the box can
// reach is computed; tiles it cannot reach are stored as zeros without touching proto.  Where the original is smaller than half the
// crop -- four source pixels per result, the rest of the crop unused -- or a tile would not fit, the four products are read from proto
// directly: no ratio is refused.  Result bytes leave in 16-byte stores: the column groups of a row start where its address is a
// multiple of 16, whatever the row length and the output offset, with byte stores at both ends.  No atomics, k-ascending fmaf chains,
// blends with one rounding per operation: the same bytes run to run.
#define PN_MAXB 64                              // images per call (the tables travel as a kernel argument)
#define PN_CAP ((PM_TH + 2) * (PM_TW + 2))      // fp32 entries of the LDS tile

struct pn_tab {
  int B;
  int moff[PN_MAXB + 1];         // rows of image b: moff[b] .. moff[b+1] - 1
  int geo[PN_MAXB][6];           // top, bottom, left, right (scale_masks' crop of the proto grid), H0, W0
  unsigned short th[PN_MAXB], tw[PN_MAXB];  // band rows, tile columns (a multiple of 16)
  unsigned char direct[PN_MAXB];  // 1: no LDS tile, the blend reads proto
  long ooff[PN_MAXB];            // first output byte of image b
  long ioff[PN_MAXB + 1];        // first work item of image b
};

// tile shape of one image: th x tw output pixels blend at most (th - 1) in_h / H0 + 3 by (tw - 1) in_w / W0 + 3 low-resolution ones (the
// kernel measures every tile and reads proto directly where one does not fit after all)
static void pn_plan(int inh, int inw, int H0, int W0, int* th, int* tw, int* direct) {
  const double sy = (double)inh / H0, sx = (double)inw / W0;
  *th = PM_TH;
  *tw = PM_TW;
  *direct = sy > 2.0 || sx > 2.0;
  if (*direct) return;
  while (*th > 1 && (*th - 1) * sy + 3 > PM_TH + 2) *th >>= 1;
  while (*tw > 16 && (*tw - 1) * sx + 3 > PM_TW + 2) *tw >>= 1;
}

template <typename T>
__device__ __forceinline__ float pn_dot(const T* __restrict__ p, const float* coef, int nm, bool pvec) {
  float v = 0.f;
  if (pvec) {
    for (int k = 0; k < nm; k += 8) {
      Vec8<T> q;
      q.load(p + k);
#pragma unroll
      for (int e = 0; e < 8; ++e) v = __builtin_fmaf(coef[k + e], q.get(e), v);
    }
  } else {
    for (int k = 0; k < nm; ++k) v = __builtin_fmaf(coef[k], to_f(p[k]), v);
  }
  return v;
}

template <typename T>
__global__ __launch_bounds__(256) void process_mask_native_kernel(pn_tab tab, int mh, int mw, int nm, const T* __restrict__ proto, int pcs, bool pvec, pm_levels lv,
                                                                  int coef_f32, const int* __restrict__ rows, const float* __restrict__ boxes,
                                                                  uint8_t* __restrict__ out) {
  __shared__ float tile[PN_CAP];
  __shared__ float coef[PM_MAXNM];
  __shared__ int xi0[PM_TW], xi1[PM_TW];  // source columns of the tile's output columns, relative to the LDS tile
  __shared__ float xl1[PM_TW];
  const int tid = threadIdx.x;
  const long item = blockIdx.x;
  int b = 0;
  while (b + 1 < tab.B && item >= tab.ioff[b + 1]) ++b;  // (workgroup-uniform)
  const int* g = tab.geo[b];
  const int top = g[0], left = g[2], inh = g[1] - g[0], inw = g[3] - g[2], H0 = g[4], W0 = g[5];
  const int th = tab.th[b], tw = tab.tw[b];
  const int nbands = (H0 + th - 1) / th;
  const long local = item - tab.ioff[b];
  const int nl = (int)(local / nbands), band = (int)(local % nbands);
  const int n = tab.moff[b] + nl;
  const int oy0 = band * th, oy1 = min(oy0 + th, H0);
  uint8_t* o = out + tab.ooff[b] + (long)nl * H0 * W0;

  // ---- the detection: (image, anchor) -> level and pixel of the coefficient maps.  The image must be the one whose rows these are.
  const int img = rows[2 * n], a = rows[2 * n + 1];
  int lvl = -1, pix = 0;
  if (img == b && a >= 0) {
    int rem = a;
    for (int l = 0; l < lv.n; ++l) {
      const int hw = lv.H[l] * lv.W[l];
      if (rem < hw) { lvl = l; pix = rem; break; }
      rem -= hw;
    }
  }
  const bool valid = lvl >= 0;
  float x1 = 0.f, y1 = 0.f, x2 = 0.f, y2 = 0.f;
  if (valid) {
    x1 = boxes[4 * n]; y1 = boxes[4 * n + 1]; x2 = boxes[4 * n + 2]; y2 = boxes[4 * n + 3];
    if (tid < nm) {
      const long off = ((long)img * lv.H[lvl] * lv.W[lvl] + pix) * lv.cs[lvl] + tid;
      coef[tid] = coef_f32 ? ((const float*)lv.coef[lvl])[off] : (float)((const f16*)lv.coef[lvl])[off];
    }
  }
  // integer footprint of crop_mask (only used to skip work; the fp32 comparisons below decide every pixel).  NaN corners give an empty one.
  const int fx_lo = (int)ceilf(fminf(fmaxf(x1, 0.f), (float)W0)), fx_hi = (int)ceilf(fminf(fmaxf(x2, 0.f), (float)W0));
  const int fy_lo = (int)ceilf(fminf(fmaxf(y1, 0.f), (float)H0)), fy_hi = (int)ceilf(fminf(fmaxf(y2, 0.f), (float)H0));
  const int oya = max(oy0, fy_lo), oyb = min(oy1, fy_hi);  // the band's rows the box reaches
  const bool band_live = valid && fx_lo < fx_hi && oya < oyb;
  const float scy = mp_scale(inh, H0), scx = mp_scale(inw, W0);
  int ra = 0, TR = 0;
  if (band_live) {
    ra = mp_source_scaled(oya, inh, H0, scy).i0;
    TR = mp_source_scaled(oyb - 1, inh, H0, scy).i1 - ra + 1;
  }
  const T* pimg = proto + (((long)b * mh + top) * mw + left) * pcs;  // the crop's first pixel
  const int ng = tw / 16 + 1;  // 16-byte groups of a tile's row, counted from the aligned address at or below its first byte

  for (int ox0 = 0; ox0 < W0; ox0 += tw) {
    const int ox1 = min(ox0 + tw, W0);
    const int oxa = max(ox0, fx_lo), oxb = min(ox1, fx_hi);  // the tile's columns the box reaches
    const bool live = band_live && oxa < oxb;  // (workgroup-uniform, like everything above)
    int ca = 0, TC = 0;
    bool lds = false;
    if (live) {
      ca = mp_source_scaled(oxa, inw, W0, scx).i0;
      TC = mp_source_scaled(oxb - 1, inw, W0, scx).i1 - ca + 1;
      lds = !tab.direct[b] && (long)TR * TC <= PN_CAP;
      __syncthreads();  // coef is written; the previous tile's readers are done
      if (lds) {
        for (int idx = tid; idx < TR * TC; idx += 256) {
          const int r = ra + idx / TC, c = ca + idx % TC;
          tile[idx] = pn_dot(pimg + ((long)r * mw + c) * pcs, coef, nm, pvec);
        }
      }
      for (int k = tid; k < oxb - oxa; k += 256) {
        const mp_src sx = mp_source_scaled(oxa + k, inw, W0, scx);
        xi0[k] = sx.i0 - ca;
        xi1[k] = sx.i1 - ca;
        xl1[k] = sx.l1;
      }
      __syncthreads();
    }
    // ---- output: a thread owns one 16-byte group of a row; consecutive lanes, consecutive groups
    for (int w = tid; w < (oy1 - oy0) * ng; w += 256) {
      const int oy = oy0 + w / ng, gi = w % ng;
      uint8_t* row = o + (long)oy * W0;
      const int gx = ox0 - (int)((uintptr_t)(row + ox0) & 15) + 16 * gi;  // the group's first column: row + gx is a multiple of 16
      const int lo = max(gx, ox0), hi = min(gx + 16, ox1);
      if (lo >= hi) continue;
      ey_u32x4 bits = (ey_u32x4)0u;
      const float fy = (float)oy;
      if (live && fy >= y1 && fy < y2 && lo < oxb && hi > oxa) {
        const mp_src sy = mp_source_scaled(oy, inh, H0, scy);
        const float* t0 = &tile[(sy.i0 - ra) * TC];
        const float* t1 = &tile[(sy.i1 - ra) * TC];
        const T* p0 = pimg + (long)sy.i0 * mw * pcs;
        const T* p1 = pimg + (long)sy.i1 * mw * pcs;
        for (int ox = max(lo, oxa); ox < min(hi, oxb); ++ox) {
          const float fx = (float)ox;
          if (!(fx >= x1 && fx < x2)) continue;
          const int k = ox - oxa, e = ox - gx;
          const int c0 = xi0[k], c1 = xi1[k];
          const float l1 = xl1[k], l0 = __fsub_rn(1.f, l1);
          float va, vb, vc, vd;
          if (lds) {
            va = t0[c0]; vb = t0[c1]; vc = t1[c0]; vd = t1[c1];
          } else {
            va = pn_dot(p0 + (long)(ca + c0) * pcs, coef, nm, pvec);
            vb = pn_dot(p0 + (long)(ca + c1) * pcs, coef, nm, pvec);
            vc = pn_dot(p1 + (long)(ca + c0) * pcs, coef, nm, pvec);
            vd = pn_dot(p1 + (long)(ca + c1) * pcs, coef, nm, pvec);
          }
          const float u0 = __fadd_rn(__fmul_rn(l0, va), __fmul_rn(l1, vb)), u1 = __fadd_rn(__fmul_rn(l0, vc), __fmul_rn(l1, vd));
          const float v = __fadd_rn(__fmul_rn(sy.l0, u0), __fmul_rn(sy.l1, u1));
          bits[e >> 2] |= (v > 0.f ? 1u : 0u) << (8 * (e & 3));
        }
      }
      if (hi - lo == 16) {
        *reinterpret_cast<ey_u32x4*>(row + gx) = bits;
      } else {
        for (int e = lo - gx; e < hi - gx; ++e) row[gx + e] = (uint8_t)((bits[e >> 2] >> (8 * (e & 3))) & 0xffu);
      }
    }
  }
}

extern "C" int ey_process_mask_native(int dtype, int B, int mh, int mw, int nm, const void* proto, int proto_cstride, int nlevels, const void* const* coef,
                                      int coef_dtype, const int* coef_cstride, const int* H, const int* W, int N, const int* rows, const float* boxes,
                                      const int* mask_off, const int* geo, const long* out_off, uint8_t* out, ey_stream_t stream) {
  EY_CHECK(dtype == EY_F16 || dtype == EY_F32, "process_mask_native: bad dtype");
  EY_CHECK(coef_dtype == EY_F16 || coef_dtype == EY_F32, "process_mask_native: bad coefficient dtype");
  if (nm < 8 || nm > PM_MAXNM || nm % 8) return ey_set_error(EY_EUNSUPPORTED, "process_mask_native: nm=%d (multiples of 8 up to %d are built)", nm, PM_MAXNM);
  if (nlevels < 1 || nlevels > PM_MAXLV)
    return ey_set_error(EY_EUNSUPPORTED, "process_mask_native: %d coefficient levels (1 to %d are built)", nlevels, PM_MAXLV);
  if (B > PN_MAXB) return ey_set_error(EY_EUNSUPPORTED, "process_mask_native: B=%d (up to %d images per call are built)", B, PN_MAXB);
  EY_CHECK(N >= 0 && B > 0 && mh > 0 && mw > 0 && proto_cstride >= nm, "process_mask_native: B=%d mh=%d mw=%d nm=%d N=%d", B, mh, mw, nm, N);
  if (N == 0) return EY_OK;
  EY_CHECK(proto && coef && coef_cstride && H && W && rows && boxes && out && mask_off && geo && out_off, "process_mask_native: null pointer");
  // rows grouped by image: image b's are mask_off[b] .. mask_off[b+1] - 1 (a row there that names another image gives a zero mask)
  EY_CHECK(mask_off[0] == 0, "process_mask_native: mask_off[0]=%d must be 0", mask_off[0]);
  for (int b = 0; b < B; ++b) EY_CHECK(mask_off[b + 1] >= mask_off[b], "process_mask_native: rows are not grouped by image: the offsets of image %d decrease", b);
  EY_CHECK(mask_off[B] == N, "process_mask_native: rows are not grouped by image: mask_off[%d]=%d, N=%d", B, mask_off[B], N);
  pn_tab tab = {};
  tab.B = B;
  long items = 0;
  for (int b = 0; b < B; ++b) {
    const int* g = geo + 6 * b;
    EY_CHECK(g[4] >= 1 && g[5] >= 1, "process_mask_native: image %d: target %d x %d", b, g[4], g[5]);
    EY_CHECK(0 <= g[0] && g[0] < g[1] && g[1] <= mh && 0 <= g[2] && g[2] < g[3] && g[3] <= mw,
             "process_mask_native: image %d: empty or misplaced crop, rows %d..%d, columns %d..%d of a %d x %d proto", b, g[0], g[1], g[2], g[3], mh, mw);
    if (g[4] >= (1 << 24) || g[5] >= (1 << 24))
      return ey_set_error(EY_EUNSUPPORTED, "process_mask_native: image %d: target %d x %d (coordinates up to 2^24 are exact in fp32)", b, g[4], g[5]);
    int th, tw, direct;
    pn_plan(g[1] - g[0], g[3] - g[2], g[4], g[5], &th, &tw, &direct);
    for (int k = 0; k < 6; ++k) tab.geo[b][k] = g[k];
    tab.th[b] = (unsigned short)th;
    tab.tw[b] = (unsigned short)tw;
    tab.direct[b] = (unsigned char)direct;
    tab.moff[b + 1] = mask_off[b + 1];
    tab.ioff[b] = items;
    items += (long)(mask_off[b + 1] - mask_off[b]) * ey_cdiv(g[4], th);
    tab.ioff[b + 1] = items;
    EY_CHECK(out_off[b] >= 0 || mask_off[b + 1] == mask_off[b], "process_mask_native: out_off[%d]=%ld", b, out_off[b]);
    tab.ooff[b] = out_off[b];
  }
  pm_levels lv;
  lv.n = nlevels;
  long A = 0;
  for (int l = 0; l < PM_MAXLV; ++l) {
    const bool on = l < nlevels;
    EY_CHECK(!on || (coef[l] && H[l] > 0 && W[l] > 0 && coef_cstride[l] >= nm), "process_mask_native: level %d is empty", l);
    lv.coef[l] = on ? coef[l] : nullptr;
    lv.cs[l] = on ? coef_cstride[l] : 0;
    lv.H[l] = on ? H[l] : 0;
    lv.W[l] = on ? W[l] : 0;
    if (on) A += (long)H[l] * W[l];
  }
  if (A >= (1L << 31) || (long)mh * mw >= (1L << 31)) return ey_set_error(EY_EUNSUPPORTED, "process_mask_native: map too large");
  if (items >= (1L << 31)) return ey_set_error(EY_EUNSUPPORTED, "process_mask_native: %ld work items (up to 2^31 - 1)", items);
  const size_t es = dtype == EY_F16 ? 2 : 4;
  const bool pvec = ey_aligned(proto, 16) && ((size_t)proto_cstride * es) % 16 == 0;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == EY_F16)
    hipLaunchKernelGGL((process_mask_native_kernel<f16>), dim3((unsigned)items), dim3(256), 0, st, tab, mh, mw, nm, (const f16*)proto, proto_cstride, pvec, lv,
                       coef_dtype == EY_F32, rows, boxes, out);
  else
    hipLaunchKernelGGL((process_mask_native_kernel<float>), dim3((unsigned)items), dim3(256), 0, st, tab, mh, mw, nm, (const float*)proto, proto_cstride, pvec, lv,
                       coef_dtype == EY_F32, rows, boxes, out);
  EY_LAUNCH_CHECK("ey_process_mask_native");
  return EY_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// ey_deconv2x2.  Packed weight: [4 Cout rows][Cin] in T.  Row order: rows come in groups of 32 = two MFMA tiles; row i of the first tile
// of group p is GEMM column q = 32p + 8 (i / 4) + (i % 4), row i of the second q + 4: the lane (pixel, kq) of the result then holds the 8
// consecutive columns 32p + 8kq .. + 7 -- one (di, dj) position (q / Cout) and 8 consecutive output channels: one 16-byte (f16) store.
#define DC_MT 4  // 16-pixel tiles per wave
#define DC_NP 2  // 32-row weight groups per sweep

__device__ __forceinline__ f32x4 dc_mma(const Vec8<f16>& a, const Vec8<f16>& b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(a.v, b.v, c, 0, 0, 0);
}
// exact f32: a k-ordered fmaf chain (lane (r, q) holds k = 8q .. 8q+7 of both operands)
__device__ __forceinline__ f32x4 dc_mma(const Vec8<float>& a, const Vec8<float>& b, f32x4 c) {
#pragma unroll
  for (int j = 0; j < 4; ++j) c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.lo[j], b.lo[j], c, 0, 0, 0);
#pragma unroll
  for (int j = 0; j < 4; ++j) c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.hi[j], b.hi[j], c, 0, 0, 0);
  return c;
}

template <typename T>
__global__ __launch_bounds__(256) void deconv2x2_kernel(int npix, int H, int W, int Cin, int Cout, const T* __restrict__ x, int xCs, const T* __restrict__ wp,
                                                        const float* __restrict__ bias, T* __restrict__ y, int yCs) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = lane & 15, kq = lane >> 4;
  const long p0 = ((long)blockIdx.x * 4 + wave) * (16 * DC_MT);
  if (p0 >= npix) return;
  const T* xp[DC_MT];
  long ybase[DC_MT];
  bool ok[DC_MT];
#pragma unroll
  for (int m = 0; m < DC_MT; ++m) {
    long p = p0 + m * 16 + col;
    ok[m] = p < npix;
    if (!ok[m]) p = npix - 1;  // tile tail: a valid address, the result is never stored
    xp[m] = x + p * xCs + kq * 8;
    const int j = (int)(p % W), i = (int)((p / W) % H);
    const long b = p / ((long)W * H);
    ybase[m] = ((b * 2 * H + 2 * i) * (2L * W) + 2 * j) * yCs;
  }
  const int ngroups = (4 * Cout) / 32;
  for (int g0 = 0; g0 < ngroups; g0 += DC_NP) {
    f32x4 acc[DC_MT][2 * DC_NP];
#pragma unroll
    for (int m = 0; m < DC_MT; ++m)
#pragma unroll
      for (int t = 0; t < 2 * DC_NP; ++t) acc[m][t] = (f32x4)0.f;
    for (int k0 = 0; k0 < Cin; k0 += 32) {
      const bool in = k0 + kq * 8 < Cin;  // K tail (Cin % 32 != 0): whole octets, zero in both operands
      Vec8<T> b[DC_MT];
#pragma unroll
      for (int m = 0; m < DC_MT; ++m) {
        if (in) b[m].load(xp[m] + k0); else b[m].zero();
      }
#pragma unroll
      for (int t = 0; t < 2 * DC_NP; ++t) {
        const int row = (g0 + (t >> 1)) * 32 + (t & 1) * 16 + col;
        Vec8<T> a;
        if (in && row < 4 * Cout) a.load(wp + (long)row * Cin + kq * 8 + k0); else a.zero();
#pragma unroll
        for (int m = 0; m < DC_MT; ++m) acc[m][t] = dc_mma(a, b[m], acc[m][t]);
      }
    }
#pragma unroll
    for (int pr = 0; pr < DC_NP; ++pr) {
      const int q = (g0 + pr) * 32 + kq * 8;
      if (q >= 4 * Cout) continue;
      const int d = q / Cout, co = q % Cout;
      const long doff = ((long)(d >> 1) * (2L * W) + (d & 1)) * yCs + co;
      float bv[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) bv[e] = bias[co + e];
#pragma unroll
      for (int m = 0; m < DC_MT; ++m) {
        if (!ok[m]) continue;
        Vec8<T> o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          o.set(e, acc[m][2 * pr][e] + bv[e]);
          o.set(e + 4, acc[m][2 * pr + 1][e] + bv[e + 4]);
        }
        o.store(y + ybase[m] + doff);
      }
    }
  }
}

static inline long dc_row_column(long row) {  // packed row -> GEMM column q = (di * 2 + dj) * Cout + co
  const long p = row / 32, t = (row % 32) / 16, i = row % 16;
  return 32 * p + 8 * (i / 4) + 4 * t + (i % 4);
}

extern "C" size_t ey_deconv2x2_packed_bytes(int dtype, int Cin, int Cout) {
  if (Cin <= 0 || Cout <= 0) return 0;
  return (size_t)4 * Cout * Cin * (dtype == EY_F16 ? 2 : 4);
}

extern "C" int ey_deconv2x2_pack_weight(int dtype, int Cin, int Cout, const float* w_iohw, void* dst, size_t dst_bytes) {
  EY_CHECK(w_iohw && dst, "deconv2x2_pack_weight: null pointer");
  EY_CHECK(dtype == EY_F16 || dtype == EY_F32, "deconv2x2_pack_weight: bad dtype");
  EY_CHECK(Cin > 0 && Cout > 0 && Cin % 8 == 0 && Cout % 8 == 0, "deconv2x2_pack_weight: Cin=%d Cout=%d must be multiples of 8", Cin, Cout);
  EY_CHECK(dst_bytes >= ey_deconv2x2_packed_bytes(dtype, Cin, Cout), "deconv2x2_pack_weight: destination too small");
  for (long row = 0; row < 4L * Cout; ++row) {
    const long q = dc_row_column(row);
    const long d = q / Cout, co = q % Cout;
    for (long ci = 0; ci < Cin; ++ci) {
      const float v = w_iohw[(ci * Cout + co) * 4 + d];  // W[ci][co][di][dj]
      if (dtype == EY_F16) ((f16*)dst)[row * Cin + ci] = (f16)v;
      else ((float*)dst)[row * Cin + ci] = v;
    }
  }
  return EY_OK;
}

extern "C" int ey_deconv2x2(int dtype, int B, int H, int W, int Cin, int Cout, const void* x, int x_cstride, const void* w_packed, const float* bias, void* y,
                            int y_cstride, ey_stream_t stream) {
  EY_CHECK(x && w_packed && bias && y, "deconv2x2: null pointer");
  EY_CHECK(dtype == EY_F16 || dtype == EY_F32, "deconv2x2: bad dtype");
  EY_CHECK(B > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0 && x_cstride >= Cin && y_cstride >= Cout, "deconv2x2: B=%d H=%d W=%d Cin=%d Cout=%d", B, H, W, Cin, Cout);
  if (Cin % 8 || Cout % 8 || Cin > 384 || Cout > 384)
    return ey_set_error(EY_EUNSUPPORTED, "deconv2x2: Cin=%d Cout=%d (multiples of 8 up to 384 are built)", Cin, Cout);
  const size_t es = dtype == EY_F16 ? 2 : 4;
  if (!ey_aligned(x, 16) || !ey_aligned(y, 16) || ((size_t)x_cstride * es) % 16 || ((size_t)y_cstride * es) % 16)
    return ey_set_error(EY_EUNSUPPORTED, "deconv2x2: x and y must be 16-byte aligned channel windows (pixel strides multiples of 16 bytes)");
  EY_CHECK(ey_aligned(w_packed, 16), "deconv2x2: the packed weight must be 16-byte aligned");
  const long npix = (long)B * H * W;
  if (npix * 4 * y_cstride >= (1L << 40) || npix >= (1L << 29)) return ey_set_error(EY_EUNSUPPORTED, "deconv2x2: tensor too large (%ld input pixels)", npix);
  const dim3 grid((unsigned)ey_cdiv(npix, 4 * 16 * DC_MT));
  hipStream_t st = (hipStream_t)stream;
  if (dtype == EY_F16)
    hipLaunchKernelGGL((deconv2x2_kernel<f16>), grid, dim3(256), 0, st, (int)npix, H, W, Cin, Cout, (const f16*)x, x_cstride, (const f16*)w_packed, bias, (f16*)y,
                       y_cstride);
  else
    hipLaunchKernelGGL((deconv2x2_kernel<float>), grid, dim3(256), 0, st, (int)npix, H, W, Cin, Cout, (const float*)x, x_cstride, (const float*)w_packed, bias,
                       (float*)y, y_cstride);
  EY_LAUNCH_CHECK("ey_deconv2x2");
  return EY_OK;
}
