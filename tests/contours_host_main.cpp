// Host build of the contour core (edge-yolo_amd/csrc/contours_core.inc.h) with ONE lane: the same text the HIP kernel runs, as a plain
// program that reads masks from a file and writes their contours, so that it can be compared with the restatement
// (tests/contours_ref.py) and run under AddressSanitizer / UBSan without a GPU.  Every array is an allocation of its own, of exactly the
// size the kernel is promised, so that an index past any of them is reported.
//
//   contours_host_main <case file> <result file>
// case file (little endian): int32 head[8] = n, h, w, contour_cap, vertex_cap, has_windows, 0, 0; uint8 masks[n][h][w];
//   int32 windows[n][4] when has_windows
// result, per mask: int32 info[4], int32 lens[contour_cap], int32 verts[vertex_cap][2] (entries nobody wrote hold -7); then the masks
//   again, as they are after the run
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../edge-yolo_amd/csrc/contours_core.inc.h"

struct HostLanes {
  int id() const { return 0; }
  int count() const { return 1; }
  void barrier() {}
  int imin(int v) { return v; }
};

template <class T>
static bool get(FILE* f, T* p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }
template <class T>
static void put(FILE* f, const T* p, size_t n) { if (n) fwrite(p, sizeof(T), n, f); }

static int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) return 2;
  int head[8];
  if (!get(in, head, 8)) return 3;
  const int n = head[0], h = head[1], w = head[2], ccap = head[3], vcap = head[4];
  if (n < 0 || h < 1 || w < 1 || ccap < 1 || vcap < 1) return 3;
  std::vector<std::vector<unsigned char>> masks(n, std::vector<unsigned char>((size_t)h * w));
  for (auto& m : masks)
    if (!get(in, m.data(), m.size())) return 3;
  std::vector<int> win((size_t)n * 4);
  if (head[5] && !get(in, win.data(), win.size())) return 3;
  HostLanes ln;
  for (int b = 0; b < n; ++b) {
    ctr::Job J;
    J.mask = masks[b].data();
    J.ld = w;
    int x0 = 0, y0 = 0, x1 = w, y1 = h;
    if (head[5]) {
      x0 = clampi(win[4 * b], 0, w); y0 = clampi(win[4 * b + 1], 0, h);
      x1 = clampi(win[4 * b + 2], x0, w); y1 = clampi(win[4 * b + 3], y0, h);
    }
    J.x0 = x0; J.y0 = y0; J.ww = x1 - x0; J.wh = y1 - y0;
    std::vector<signed char> lbl(((size_t)J.wh + 2) * ((size_t)J.ww + 2), 99);  // exactly the window's plane: smaller than the kernel's
    std::vector<int> lens(ccap, -7), verts((size_t)vcap * 2, -7), info(ctr::I_N, -7), sh(1, -7);
    J.lbl = lbl.data(); J.ccap = ccap; J.vcap = vcap; J.lens = lens.data(); J.verts = verts.data(); J.info = info.data(); J.sh = sh.data();
    ctr::contours(ln, J);
    put(out, info.data(), info.size());
    put(out, lens.data(), lens.size());
    put(out, verts.data(), verts.size());
  }
  for (auto& m : masks) put(out, m.data(), m.size());
  fclose(in);
  return fclose(out) == 0 ? 0 : 4;
}
