// Matching one image's kept rows against its labels: the true positives of the reference's BaseValidator.match_predictions (engine/validator.py
// :222-262) at up to MAX_T IoU thresholds and the increments of its ConfusionMatrix.process_batch (utils/metrics.py:326-382), as closed forms
// with no sort in them; written once for the device (match.hip: one workgroup per image) and for the host (tests/match_host_main.cpp: one lane).
// Everything here is stated against a tiny lane abstraction `L`, as contours_core.inc.h and track_core.inc.h are:
//   ln.id() / ln.count()   this lane and the number of lanes that work on the same image
//   ln.barrier()           every lane arrives; the writes made before it are visible to every lane after it
//   ln.amin(p, v)          *p = min(*p, v), atomically among the lanes (p: scratch shared by the lanes)
//   ln.amax(p, v)          *p = max(*p, v), likewise, on 64-bit keys
//   ln.gadd(p)             ++*p, atomically among all images (p: the confusion matrix)
//
// True positives (class-aware): q[g,d] = iou[g,d] * (cls[g] == cls[d]); g*(d) = argmax_g q[g,d], b(d) = that value.  At threshold t label g is
//   taken by the LOWEST-index d with g*(d) = g and b(d) >= iouv[t]; tp[d,t] = 1 for exactly those d.  This is the reference's
//   sort-by-IoU / unique-by-detection / unique-by-label: the first unique keeps each detection's best pair, and since np.unique returns its
//   values sorted, the pairs then stand in detection order and the second unique keeps each label's lowest detection.
// Confusion matrix (class-agnostic), among the detections with conf > cm_conf: g*(d) = argmax_g iou[g,d], valid if > cm_iou; label g takes the
//   detection with the HIGHEST IoU among those whose g* is g (the reference sorts by IoU again before its second unique).
// Ties (exact IoU ties are not pinned by the reference, numpy's sort being unstable): among labels the HIGHER label index wins, among
//   detections the LOWER detection index wins.
// No FMA contraction anywhere in this file: the box IoU equals metrics.box_iou / torch's CPU box_iou bit for bit.  DESIGN.md section 7t.
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifndef MTC_HD
#define MTC_HD
#endif

namespace mtc {

enum { MAX_T = 16, FREE = 0x7fffffff };
enum { CG_OUT = -2, CG_NONE = -1 };  // cg[d]: the detection takes no part in the matrix / takes part and has no valid label

typedef unsigned long long u64;

// scratch bytes of one image of up to D rows and G labels (what the kernel carves out of its LDS)
MTC_HD inline size_t scratch_bytes(int D, int G, int T, bool boxes, bool want_tp, bool want_matrix) {
  size_t n = (size_t)G * 4;                                            // lcls
  if (want_matrix) n += (size_t)G * 8 + (size_t)D * 4;                 // cmkey, cg
  if (boxes) n += (size_t)G * 16;                                      // lbox
  if (want_tp) n += (size_t)G * (size_t)T * 4 + (size_t)D * 8;         // taker, dg, db
  return (n + 15) / 16 * 16 + 16;
}

struct Job {
  int D, G, T, nc, stride;  // rows and labels of this image, thresholds, classes, floats per row
  const float* rows;        // [D][stride] x1,y1,x2,y2,conf,cls,...: only columns 0..5 of rows 0..D-1 are read
  const float* xform;       // [5] padx, pady, gain, w0, h0, or null: the rows are in the labels' frame already
  const float* gbox;        // [G][4] xyxy, or null in matrix mode
  const int* gcls;          // [G]
  const float* iou;         // [G][ld] row-major in matrix mode (ld >= D), else null
  int ld;
  const float* iouv;        // [T]
  float cm_conf, cm_iou;
  unsigned char* tp;        // [D][T] or null
  int* matrix;              // [(nc + 1)^2] or null
  // scratch shared by the lanes (LDS on the device); the ones of an absent output or mode may be null
  float* lbox;              // [G][4]
  int* lcls;                // [G] the label's class, -1 where it is outside [0, nc)
  int* taker;               // [G][T] the lowest detection that takes the label at the threshold
  u64* cmkey;               // [G] the best (IoU, detection) of the label, 0 = none
  int* dg;                  // [D] g*(d) of the true positives, -1 = none
  float* db;                // [D] b(d)
  int* cg;                  // [D] g*(d) of the matrix, or CG_OUT / CG_NONE
};

MTC_HD inline unsigned f2ord(float f) {  // order-preserving map of the floats onto the unsigned integers
  union { float f; unsigned u; } v;
  v.f = f;
  return (v.u & 0x80000000u) ? ~v.u : (v.u | 0x80000000u);
}

// ops.scale_boxes + clip_boxes of one coordinate: subtract the pad, IEEE-divide by the gain, clamp to [0, hi]
MTC_HD inline float scale1(float v, float pad, float gain, float hi) {
#pragma clang fp contract(off)
  float r = (v - pad) / gain;
  r = r < 0.f ? 0.f : r;
  return r > hi ? hi : r;
}

// metrics.box_iou(label, detection) of one pair; ad: the detection's area
MTC_HD inline float box_iou1(const float* g, float x1, float y1, float x2, float y2, float ad) {
#pragma clang fp contract(off)
  float w = (g[2] < x2 ? g[2] : x2) - (g[0] > x1 ? g[0] : x1);
  float h = (g[3] < y2 ? g[3] : y2) - (g[1] > y1 ? g[1] : y1);
  w = w > 0.f ? w : 0.f;
  h = h > 0.f ? h : 0.f;
  const float inter = w * h;
  const float ag = (g[2] - g[0]) * (g[3] - g[1]);
  const float sum = ag + ad;
  const float uni = sum - inter;
  return inter / (uni + 1e-7f);
}

template <class L>
MTC_HD void match(L& ln, const Job& J) {
#pragma clang fp contract(off)
  const int lane = ln.id(), nl = ln.count();
  const int D = J.D, G = J.G, T = J.T, nc = J.nc;
  const bool want_tp = J.tp != nullptr, want_cm = J.matrix != nullptr, boxes = J.gbox != nullptr;
  for (int g = lane; g < G; g += nl) {
    const int c = J.gcls[g];
    J.lcls[g] = (c >= 0 && c < nc) ? c : -1;
    if (boxes)
      for (int k = 0; k < 4; ++k) J.lbox[4 * g + k] = J.gbox[4 * (size_t)g + k];
    if (want_cm) J.cmkey[g] = 0;
    if (want_tp)
      for (int t = 0; t < T; ++t) J.taker[g * T + t] = FREE;
  }
  ln.barrier();
  const float ninf = -__builtin_huge_valf();
  for (int d = lane; d < D; d += nl) {
    const float* r = J.rows + (size_t)d * J.stride;
    const float conf = r[4], c = r[5];
    const bool ok = c >= 0.f && c < (float)nc;  // (false for NaN) a row of another class is skipped, never indexed with
    float x1 = 0.f, y1 = 0.f, x2 = 0.f, y2 = 0.f, ad = 0.f;
    if (boxes && ok) {
      x1 = r[0]; y1 = r[1]; x2 = r[2]; y2 = r[3];
      if (J.xform) {
        const float px = J.xform[0], py = J.xform[1], gn = J.xform[2], w0 = J.xform[3], h0 = J.xform[4];
        x1 = scale1(x1, px, gn, w0); y1 = scale1(y1, py, gn, h0); x2 = scale1(x2, px, gn, w0); y2 = scale1(y2, py, gn, h0);
      }
      ad = (x2 - x1) * (y2 - y1);
    }
    const bool part = want_cm && ok && conf > J.cm_conf;
    float bt = ninf, bc = ninf;
    int gt = -1, gc = -1;
    if (ok && (want_tp || part)) {
      for (int g = 0; g < G; ++g) {
        const int cg = J.lcls[g];
        if (cg < 0) continue;
        const float iou = boxes ? box_iou1(J.lbox + 4 * g, x1, y1, x2, y2, ad) : J.iou[(size_t)g * J.ld + d];
        const float q = iou * ((float)cg == c ? 1.f : 0.f);
        if (q >= bt) { bt = q; gt = g; }    // >=: of equal labels the higher index
        if (iou >= bc) { bc = iou; gc = g; }
      }
    }
    if (want_tp) {
      J.dg[d] = gt;
      J.db[d] = bt;
      if (gt >= 0)
        for (int t = 0; t < T; ++t)
          if (bt >= J.iouv[t]) ln.amin(J.taker + gt * T + t, d);  // of equal detections the lower index
    }
    if (want_cm) {
      const bool valid = part && gc >= 0 && bc > J.cm_iou;
      J.cg[d] = !part ? (int)CG_OUT : (valid ? gc : (int)CG_NONE);
      if (valid) ln.amax(J.cmkey + gc, ((u64)f2ord(bc) << 32) | (u64)(0xFFFFFFFFu - (unsigned)d));  // highest IoU, then the lower index
    }
  }
  ln.barrier();
  for (int d = lane; d < D; d += nl) {
    if (want_tp) {
      const int gt = J.dg[d];
      const float bt = J.db[d];
      for (int t = 0; t < T; ++t) J.tp[(size_t)d * T + t] = (gt >= 0 && bt >= J.iouv[t] && J.taker[gt * T + t] == d) ? 1 : 0;
    }
    if (want_cm) {
      const int gc = J.cg[d];
      if (gc == CG_OUT) continue;
      const bool won = gc >= 0 && (unsigned)(J.cmkey[gc] & 0xFFFFFFFFu) == 0xFFFFFFFFu - (unsigned)d;
      if (!won) ln.gadd(J.matrix + (size_t)(int)J.rows[(size_t)d * J.stride + 5] * (nc + 1) + nc);  // predicted, matched by no label
    }
  }
  if (want_cm)
    for (int g = lane; g < G; g += nl) {
      const int cg = J.lcls[g];
      if (cg < 0) continue;
      const u64 key = J.cmkey[g];
      if (key == 0) { ln.gadd(J.matrix + (size_t)nc * (nc + 1) + cg); continue; }  // a label no detection matched
      const unsigned d = 0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFu);
      ln.gadd(J.matrix + (size_t)(int)J.rows[(size_t)d * J.stride + 5] * (nc + 1) + cg);
    }
}

}  // namespace mtc
