// Per-axis source index and weights of F.interpolate(mode="bilinear", align_corners=False), shared by the FastSAM prompt kernels, ey_scale_masks
// (fastsam.hip) and ey_process_mask_native (segment.hip).  They are torch's CPU operator's (aten/src/ATen/native/UpSample.h
// compute_source_index_and_lambda with float opmath; the source coordinate is ONE fused multiply-add, which is what the operator's compiled
// code evaluates -- the two-rounding form differs from it in individual weights):
//   in == out:  i0 = i1 = y, l0 = 1, l1 = 0
//   otherwise:  r = max(fmaf((float)in / out, y + 0.5f, -0.5f), 0);  i0 = min((int)r, in - 1);  l1 = min(max(r - i0, 0), 1);
//               i1 = i0 + (i0 < in - 1);  l0 = 1 - l1
// Every operation is written out with its rounding, so the result does not depend on the including file's -ffp-contract setting.
#pragma once

struct mp_src {
  int i0, i1;
  float l0, l1;
};

// the scale of an axis: computed once where a thread walks many coordinates of it
__device__ __forceinline__ float mp_scale(int in, int out) { return __fdiv_rn((float)in, (float)out); }

__device__ __forceinline__ mp_src mp_source_scaled(int y, int in, int out, float scale) {
  mp_src s;
  if (in == out) {
    s.i0 = s.i1 = y;
    s.l0 = 1.f;
    s.l1 = 0.f;
    return s;
  }
  float r = __builtin_fmaf(scale, __fadd_rn((float)y, 0.5f), -0.5f);
  r = r < 0.f ? 0.f : r;
  s.i0 = min((int)floorf(r), in - 1);
  s.l1 = fminf(fmaxf(__fsub_rn(r, (float)s.i0), 0.f), 1.f);
  s.i1 = s.i0 + (s.i0 < in - 1 ? 1 : 0);
  s.l0 = __fsub_rn(1.f, s.l1);
  return s;
}

__device__ __forceinline__ mp_src mp_source(int y, int in, int out) { return mp_source_scaled(y, in, out, mp_scale(in, out)); }
