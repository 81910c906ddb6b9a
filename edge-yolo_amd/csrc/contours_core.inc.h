// External contours of binary masks: OpenCV's border following (Suzuki & Abe 1985, algorithm 1) for RETR_EXTERNAL / CHAIN_APPROX_SIMPLE,
// written once for the device (contours.hip: one workgroup per mask) and for the host (tests/contours_host_main.cpp: one lane).
// Everything here is stated against a tiny lane abstraction `L`, as track_core.inc.h is:
//   ln.id() / ln.count()    this lane and the number of lanes that walk the same mask
//   ln.barrier()            every lane arrives; the writes made before it are visible to every lane after it
//   ln.imin(v)              the minimum of v over all lanes, the same in every lane (contains a barrier)
// The raster scan for the next border start is spread over the lanes; a border is followed by lane 0 alone, in the sequential order, so
// the result is the sequential algorithm's by construction.  Control flow is uniform: every lane takes every branch that contains a
// barrier together.  Every loop has a bound that is known before it starts.  Definition, phases and the buffer protocol: DESIGN.md 7s.
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifndef CTR_HD
#define CTR_HD
#endif

namespace ctr {

enum { F_OVERFLOW = 1, F_STEPS = 2 };                          // info[I_FLAGS]
enum { I_CONTOURS = 0, I_VERTICES, I_FLAGS, I_PAD, I_N = 4 };  // per-mask int32 info[I_N]
enum { PROBES = 16 };                                          // pixels a lane tests per round of the raster search

// the label plane of one mask: the scan window with a frame of one zero pixel around it, (wh + 2) rows of (ww + 2) labels
CTR_HD inline size_t plane_bytes(int h, int w) { return (((size_t)h + 2) * ((size_t)w + 2) + 15) / 16 * 16; }

struct Job {
  const unsigned char* mask;  // [h][w], read only
  long ld;                    // its row stride
  int x0, y0, ww, wh;         // scan window, inside the mask: columns x0 .. x0+ww-1, rows y0 .. y0+wh-1
  signed char* lbl;           // [(wh + 2) * (ww + 2)] labels: 0, 1, 2 (followed), -2 (followed, the east neighbour seen as 0)
  int ccap, vcap;             // capacity of lens[] (contours) and verts[] (vertices)
  int* lens;                  // [ccap] vertex count of contour k, in the order of discovery
  int* verts;                 // [vcap][2] x, y of all contours' vertices, one contour after the other
  int* info;                  // [I_N]
  int* sh;                    // [1] shared by the lanes
};

// directions counter-clockwise from east: 0=E 1=NE 2=N 3=NW 4=W 5=SW 6=S 7=SE; dx + 1 and dy + 1 as 2-bit fields
CTR_HD inline int delta(int s, int S) {
  s &= 7;
  const int dx = (int)((0x901Au >> (2 * s)) & 3u) - 1, dy = (int)((0xA901u >> (2 * s)) & 3u) - 1;
  return dy * S + dx;
}

struct Out {
  int nc, nv, flags;
};

// follow the border that starts at label-plane index i0 (lane 0 only).  maxsteps bounds the walk: a border enters a pixel from at most
// 8 directions, so more than 8 * (pixels of the plane) steps cannot happen in a correct walk and end it with F_STEPS.
CTR_HD inline void follow(const Job& J, int S, int i0, long maxsteps, Out& o) {
  signed char* lbl = J.lbl;
  int len = 0;
  auto emit = [&](int i) {
    const int y = i / S, x = i - y * S;
    if (o.nv < J.vcap) {
      J.verts[2 * (size_t)o.nv] = x - 1 + J.x0;
      J.verts[2 * (size_t)o.nv + 1] = y - 1 + J.y0;
    } else {
      o.flags |= F_OVERFLOW;
    }
    ++o.nv;
    ++len;
  };
  int s = 4, i1 = i0;
  bool found = false;
  for (int k = 0; k < 8; ++k) {  // clockwise from west
    s = (s - 1) & 7;
    i1 = i0 + delta(s, S);
    if (lbl[i1] != 0) { found = true; break; }
  }
  if (!found || s == 4) {  // (s == 4 cannot hold a non-zero pixel: the west neighbour of a start is 0)
    lbl[i0] = -2;
    emit(i0);
  } else {
    int i3 = i0, prev_s = s ^ 4;
    long step = 0;
    for (; step < maxsteps; ++step) {
      const int s_end = s;
      int i4 = i3;
      bool hit = false;
      for (int k = 0; k < 8; ++k) {  // counter-clockwise from s_end + 1
        ++s;
        i4 = i3 + delta(s, S);
        if (lbl[i4] != 0) { hit = true; break; }
      }
      if (!hit) { o.flags |= F_STEPS; break; }  // (the pixel the walk came from is non-zero: cannot happen)
      s &= 7;
      if ((unsigned)(s - 1) < (unsigned)s_end) lbl[i3] = -2;
      else if (lbl[i3] == 1) lbl[i3] = 2;
      if (s != prev_s) { emit(i3); prev_s = s; }
      if (i4 == i0 && i3 == i1) break;
      i3 = i4;
      s = (s + 4) & 7;
    }
    if (step >= maxsteps) o.flags |= F_STEPS;
  }
  if (o.nc < J.ccap) J.lens[o.nc] = len;
  else o.flags |= F_OVERFLOW;
  ++o.nc;
}

template <class L>
CTR_HD void contours(L& ln, const Job& J) {
  const int lane = ln.id(), nl = ln.count();
  Out o = {0, 0, 0};
  if (J.ww <= 0 || J.wh <= 0) {
    if (lane == 0) { J.info[I_CONTOURS] = 0; J.info[I_VERTICES] = 0; J.info[I_FLAGS] = 0; J.info[I_PAD] = 0; }
    return;
  }
  const int S = J.ww + 2, R = J.wh + 2;
  signed char* lbl = J.lbl;
  for (int r = 0; r < R; ++r) {  // labels = (mask != 0) inside the window, 0 on the frame
    const bool inner = r >= 1 && r <= J.wh;
    for (int c = lane; c < S; c += nl)
      lbl[(long)r * S + c] = (inner && c >= 1 && c <= J.ww && J.mask[(long)(J.y0 + r - 1) * J.ld + (J.x0 + c - 1)] != 0) ? 1 : 0;
  }
  if (lane == 0) J.sh[0] = 0;
  ln.barrier();
  const int begin = S, end = (R - 1) * S;  // the rows of the window, frame columns included (they are 0 and start nothing)
  const long maxsteps = 8L * R * S + 8;
  int pos = begin, row = -1, lx = -1;
  for (int guard = begin; guard <= end; ++guard) {  // bound: pos grows by at least 1 per round
    // the first pixel at or behind pos with label 1 and a 0 to its left: the only kind of pixel at which a border can start
    int found = end;
    for (int base = pos; base < end; base += nl * PROBES) {  // bound: (end - pos) / (nl * PROBES) + 1 rounds
      int best = end;
      for (int k = PROBES - 1; k >= 0; --k) {
        const long i = (long)base + (long)k * nl + lane;
        if (i < end && lbl[i] == 1 && lbl[i - 1] == 0) best = (int)i;
      }
      found = ln.imin(best);
      if (found < end) break;
    }
    if (found >= end) break;
    // lx: the last pixel of this row before `found` at which the scan saw a label other than 0 and 1 (and other than its left neighbour's)
    const int y = found / S;
    if (y != row) { row = y; lx = -1; }
    const int from = pos > y * S ? pos : y * S;
    int last = 0;  // (negated for imin; every index is >= S > 0)
    for (int i = from + lane; i < found; i += nl) {  // bound: one row
      const int p = lbl[i];
      if ((p & -2) != 0 && p != lbl[i - 1]) last = -i;
    }
    last = -ln.imin(last);
    if (last > 0) lx = last;
    if (!(lx >= 0 && lbl[lx] > 0)) {  // not inside a hole of a border followed before
      ln.barrier();                   // (every lane has read lbl[lx] before lane 0 relabels)
      if (lane == 0) {
        follow(J, S, found, maxsteps, o);
        if (o.flags & F_STEPS) J.sh[0] = 1;
      }
      ln.barrier();
      if (J.sh[0]) break;
    }
    if ((lbl[found] & -2) != 0) lx = found;
    pos = found + 1;
  }
  if (lane == 0) { J.info[I_CONTOURS] = o.nc; J.info[I_VERTICES] = o.nv; J.info[I_FLAGS] = o.flags; J.info[I_PAD] = 0; }
}

}  // namespace ctr
