// Host side of K1 (the kernels are in conv_kernels.inc.h): weight packing, one X_launch per kernel, one dispatch_X per kernel that
// decides whether a shape is X's, the ordered walk over them (conv2d_typed) and the C ABI entry points.
//
// Included by conv_f16.hip and conv_f32.hip (EY_CONV_PART = 16 / 32): the launchers are templates on the element type, the two
// translation units instantiate one type each and compile in parallel; everything extern "C" lives in the f16 part.
#include "conv_kernels.inc.h"
#include <stdlib.h>
#include "tune.h"  // tunables (defaults measured on MI355X; ey_tune_set overrides them for sweeps)

static int conv_nt(int Cout) {  // channels per block tile / 16
  if (Cout <= 16) return 1;
  if (Cout <= 32) return 2;
  if (Cout <= 64) return 4;
  if (Cout <= 80) return 5;
  if (Cout <= 128) return 8;
  if (Cout % 128 == 0) return 8;
  if (Cout % 80 == 0) return 5;
  if (Cout % 64 == 0) return 4;
  return 8;
}
static int conv_cout_pad(int Cout) { int bn = 16 * conv_nt(Cout); return (Cout + bn - 1) / bn * bn; }
static int conv_kpad(int Cin, int k, int es) { return ey_conv_kpad(k * k * Cin, es); }

#if EY_CONV_PART == 16
extern "C" size_t ey_conv_packed_bytes(int dtype, int Cout, int Cin, int k) {
  return (size_t)conv_cout_pad(Cout) * conv_kpad(Cin, k, dtype == EY_F16 ? 2 : 4) * (dtype == EY_F16 ? 2 : 4);
}

extern "C" int ey_conv_pack_weight(int dtype, int Cout, int Cin, int k, const float* w, void* out, size_t out_bytes) {
  EY_CHECK(dtype == EY_F16 || dtype == EY_F32, "pack: bad dtype %d", dtype);
  EY_CHECK(Cout > 0 && Cin > 0 && (k == 1 || k == 3), "pack: Cout=%d Cin=%d k=%d", Cout, Cin, k);
  EY_CHECK(out_bytes >= ey_conv_packed_bytes(dtype, Cout, Cin, k), "pack: output buffer too small");
  const int NT = conv_nt(Cout), BN = 16 * NT, Kp = conv_kpad(Cin, k, dtype == EY_F16 ? 2 : 4), rows = conv_cout_pad(Cout);
  for (int row = 0; row < rows; ++row) {
    // MFMA row rho = 4g+j of n-block nt inside block tile nb  <->  channel nb*BN + g*4NT + 4nt + j
    const int nb = row / BN, within = row % BN, nt = within / 16, rho = within % 16, g = rho / 4, j = rho % 4;
    const int ch = nb * BN + g * 4 * NT + 4 * nt + j;
    for (int kk = 0; kk < Kp; ++kk) {
      float val = 0.f;
      if (ch < Cout && kk < k * k * Cin) {
        const int tap = kk / Cin, c = kk % Cin, ky = tap / k, kx = tap % k;
        val = w[(((long)ch * Cin + c) * k + ky) * k + kx];
      }
      const long o = (long)row * Kp + kk;
      if (dtype == EY_F16) ((f16*)out)[o] = (f16)val;
      else ((float*)out)[o] = val;
    }
  }
  return EY_OK;
}
#endif

// ---- what the launchers share
// Code of the kernel the last ey_conv2d on this thread launched: base + the template arguments (ey_conv_last_variant documents the
// digits).  Every X_launch records it after its launch check passed; ey_conv2d clears it first.  Defined in the f16 translation unit.
enum ConvVariant {
  V_PWN = 3000, V_PW = 4000, V_PWR = 5000, V_TILE = 6000, V_C3R = 7000, V_C3S = 8000, V_C3P = 9000, V_SMALL = 10000, V_HALO = 11000,
  V_WS = 12000, V_IGEMM = 13000
};
#if EY_CONV_PART == 16
thread_local int g_last_variant = 0;
#else
extern thread_local int g_last_variant;
#endif

// Runtime value -> template argument: calls f(std::integral_constant<int, V>()) for the V among Vs... that equals v and returns what
// it returns; 0 ("not this kernel's") when v is none of them.  Only the listed values are instantiated.
template <int... Vs, typename F>
static int conv_pick(int v, F&& f) {
  int r = 0;
  (void)((v == Vs && ((r = f(std::integral_constant<int, Vs>())), true)) || ...);
  return r;
}

// The kernels address a source through a buffer resource with 32-bit byte offsets.  Fills p.srcBytes[s] with the extent of every
// source view (B x H>>up x W>>up pixels at pitch srcCs, srcC channels in the last) and says whether each view and the span of the
// groups, srcG * (ngroup - 1), stay below 2 GiB.
template <typename T>
static bool conv_src_views(ConvP& p, int ngroup) {
  if (p.srcG * (long)sizeof(T) * (ngroup - 1) >= (1L << 31)) return false;
  for (int s = 0; s < p.nsrc; ++s) {
    const long npix = (long)p.B * (p.H >> p.srcUp[s]) * (p.W >> p.srcUp[s]);
    const long bytes = ((npix - 1) * p.srcCs[s] + p.srcC[s]) * (long)sizeof(T);
    if (bytes >= (1L << 31)) return false;
    p.srcBytes[s] = (unsigned)bytes;
  }
  return true;
}
// ... and the packed weights of one set, for the kernels that read them the same way
template <typename T>
static bool conv_weights_fit(const ConvP& p) { return (long)conv_cout_pad(p.Cout) * p.Kpad * (long)sizeof(T) < (1L << 31); }

// total input channels and number of 32-channel K steps over all taps and sources
static void conv_count_k(ConvP& p) {
  p.Ctot = 0; p.nsteps = 0;
  for (int s = 0; s < p.nsrc; ++s) { p.Ctot += p.srcC[s]; p.nsteps += (p.srcC[s] + 31) / 32; }
  p.nsteps *= p.k * p.k;
}

// Flattened output tile of the stride-1 3x3 tile kernels: the (rows x cols) with <= 256 pixels and <= 340 halo pixels that wastes the
// fewest of the 256 pixel slots on this map.  Leaves tr x tc alone when no candidate fits.
static void conv_flat_tile(int Ho, int Wo, int& tr, int& tc) {
  double best = 0.0;
  const int cands[8] = {16, 20, 24, 28, 32, 36, 40, Wo};
  for (int i = 0; i < 8; ++i) {
    const int c = cands[i];
    if (c < 8 || c > 80) continue;
    int rr = 256 / c;
    while (rr > 1 && (rr + 2) * (c + 2) > 340) --rr;
    if (rr < 1 || (rr + 2) * (c + 2) > 340) continue;
    const long cov = (long)((Wo + c - 1) / c) * ((Ho + rr - 1) / rr) * 256;
    const double eff = (double)Wo * Ho / (double)cov;
    if (eff > best + 1e-9) { best = eff; tr = rr; tc = c; }
  }
}

// Widest channel tile NT <= max_nt (in 16-channel blocks) that splits the packing tile ntp into whole blocks and that ok(nt)
// accepts; 0 = none.
template <typename F>
static int conv_widest_nt(int ntp, int max_nt, F ok) {
  static const int cands[5] = {8, 5, 4, 2, 1};
  for (const int nt : cands)
    if (nt <= max_nt && nt <= ntp && ntp % nt == 0 && ok(nt)) return nt;
  return 0;
}

// Every dispatch_X / X_launch below returns 1 = launched, 0 = not this kernel's shape (the next one is tried), < 0 = error (set).

// ---- K-chunked fallback (conv_igemm_kernel): takes every shape
template <typename T, int NT, int MT>
static int igemm_launch(const ConvP& p, int ngroup, hipStream_t st) {
  const long M = (long)p.B * p.Ho * p.Wo;
  const int ntiles = (p.Cout + 16 * NT - 1) / (16 * NT);
  const size_t lds = 2 * (size_t)(16 * NT) * CONV_LS * sizeof(T);  // > 64 KiB for the big-tile / f32 variants
  if (!ey_lds_reserve<conv_igemm_kernel<T, NT, MT>>(lds)) return ey_set_error(EY_ELAUNCH, "conv: cannot reserve LDS for the weight tile");
  const dim3 grid((unsigned)((M + 64 * MT - 1) / (64 * MT)), ntiles, ngroup);
  hipLaunchKernelGGL((conv_igemm_kernel<T, NT, MT>), grid, dim3(256), lds, st, p);
  EY_LAUNCH_CHECK("ey_conv2d");
  g_last_variant = V_IGEMM + NT * 10 + MT;
  return 1;
}

template <typename T>
static int dispatch_igemm(const ConvP& p, int ngroup, hipStream_t st) {
  const long M = (long)p.B * p.Ho * p.Wo;
  const int nt = conv_nt(p.Cout), ntiles = (p.Cout + 16 * nt - 1) / (16 * nt);
  const int mt = (M + 127) / 128 * ntiles * ngroup >= 512 ? 2 : 1;  // 128-pixel block tiles once they still make 512 workgroups
  return conv_pick<1, 2, 4, 5, 8>(nt, [&](auto NT) { return conv_pick<1, 2>(mt, [&](auto MT) { return igemm_launch<T, NT, MT>(p, ngroup, st); }); });
}

// ---- weight-stationary dispatch (conv_ws_kernel)
// widest NT whose weight tile fits `budget` bytes of LDS; the LDS row pitch is Kpad (conv_kpad() already makes it conflict-free for
// the fragment reads)
static int ws_pick_nt(int Cout, int Kpad, int es, size_t budget) {
  return conv_widest_nt(conv_nt(Cout), 8, [&](int nt) { return (size_t)16 * nt * Kpad * es <= budget; });
}

template <typename T, int NT, int MT, int KS>
static int ws_launch(ConvP p, int ngroup, hipStream_t st) {
  const size_t lds = (size_t)16 * NT * p.LSw * sizeof(T);
  if (!ey_lds_reserve<conv_ws_kernel<T, NT, MT, KS>>(lds)) return ey_set_error(EY_ELAUNCH, "conv: cannot reserve LDS for the weight tile");
  const long M = (long)p.B * p.Ho * p.Wo;
  p.ntile = (M + 16 * MT - 1) / (16 * MT);
  const int ntiles_n = (conv_cout_pad(p.Cout)) / (16 * NT);
  // resident workgroups per CU: LDS AND registers decide (a 512-thread workgroup of a 172-VGPR instantiation fits once per
  // CU whatever its LDS footprint); a persistent grid larger than that runs in two rounds and stages every weight tile twice
  const int occ = ey_occupancy<conv_ws_kernel<T, NT, MT, KS>>(512, lds);
  const int wg_per_cu = occ < (int)tune().ws_wg_cu ? occ : (int)tune().ws_wg_cu;
  // persistent grid: one workgroup per resident slot; tiles are dealt round-robin over workgroups first, then waves,
  // so a small layer still spreads over all CUs
  long cap = (long)256 * wg_per_cu / ((long)ntiles_n * ngroup);
  if (cap < 1) cap = 1;
  cap = cap / tune().grid_div > 0 ? cap / tune().grid_div : 1;
  long gx = p.ntile < cap ? p.ntile : cap;
  if (tune().tiles_per_wave > 0) {
    long want = (p.ntile + 8 * tune().tiles_per_wave - 1) / (8 * tune().tiles_per_wave);
    if (want < 1) want = 1;
    if (want < gx) gx = want;
  }
  hipLaunchKernelGGL((conv_ws_kernel<T, NT, MT, KS>), dim3((unsigned)gx, ntiles_n, ngroup), dim3(512), lds, st, p);
  EY_LAUNCH_CHECK("ey_conv2d(ws)");
  g_last_variant = V_WS + NT * 100 + MT * 10 + KS;
  return 1;
}

template <typename T>
static int dispatch_ws(ConvP p, int ngroup, hipStream_t st) {
  int nt = ws_pick_nt(p.Cout, p.Kpad, sizeof(T), (size_t)(tune().ws_lds_kb << 10));
  if (!nt) nt = ws_pick_nt(p.Cout, p.Kpad, sizeof(T), 156 * 1024);
  if (!nt) return 0;
  if (p.k == 3 && nt < tune().ws_k3_minnt && nt < conv_nt(p.Cout)) return 0;
  if (!conv_src_views<T>(p, ngroup)) return 0;  // beyond 32-bit buffer offsets: chunked kernel
  p.NTpack = conv_nt(p.Cout);
  p.LSw = p.Kpad;
  conv_count_k(p);
  if (p.nsrc == 1) { p.srcC[1] = p.srcC[0]; p.srcCs[1] = p.srcCs[0]; p.srcUp[1] = p.srcUp[0]; }  // the kernel reads slot 1 either way
  // enough wave tiles to give every SIMD work: 2 pixel blocks per wave when M is large, else 1 (measured: below this, more
  // (smaller) wave tiles hide latency better)
  const int mt = (long)p.B * p.Ho * p.Wo >= tune().mt2_min_m ? 2 : 1;
  return conv_pick<1, 2, 4, 5, 8>(nt, [&](auto NT) {
    return conv_pick<1, 2>(mt, [&](auto MT) { return conv_pick<1, 3>(p.k, [&](auto KS) { return ws_launch<T, NT, MT, KS>(p, ngroup, st); }); });
  });
}

// ---- 3x3 halo-tile dispatch (conv3_halo_kernel)
template <typename T, int NT, int S>
static int halo_launch(ConvP p, int ngroup, hipStream_t st) {
  constexpr int MT = (S == 1) ? 2 : 1, TR = 8, TC = 16 * MT, HR = (TR - 1) * S + 3, HC = (TC - 1) * S + 3;
  const int C = p.srcC[0];
  const size_t lds = ((size_t)16 * NT * p.LSw + (size_t)HR * HC * (C + 8)) * sizeof(T);
  if (!ey_lds_reserve<conv3_halo_kernel<T, NT, S>>(lds)) return ey_set_error(EY_ELAUNCH, "conv: cannot reserve %zu B of LDS for the halo tile", lds);
  const long ntile = (long)p.B * ((p.Wo + TC - 1) / TC) * ((p.Ho + TR - 1) / TR);
  const int ntn = conv_cout_pad(p.Cout) / (16 * NT);
  const int occ = ey_occupancy<conv3_halo_kernel<T, NT, S>>(512, lds);  // resident workgroups per CU from LDS and registers (see ws_launch)
  const int per_cu = occ < 2 ? occ : 2;
  long gx = (long)256 * per_cu / ((long)ntn * ngroup);
  if (gx < 1) gx = 1;
  if (gx > ntile) gx = ntile;
  hipLaunchKernelGGL((conv3_halo_kernel<T, NT, S>), dim3((unsigned)gx, ntn, ngroup), dim3(512), lds, st, p);
  EY_LAUNCH_CHECK("ey_conv2d(halo)");
  g_last_variant = V_HALO + NT * 10 + S;
  return 1;
}

// widest NT such that weights + halo fit LDS; 0 = does not fit
template <typename T>
static int halo_pick_nt(const ConvP& p, int S) {
  const int MT = (S == 1) ? 2 : 1, TC = 16 * MT, HR = 7 * S + 3, HC = (TC - 1) * S + 3, C = p.srcC[0];
  const size_t halo = (size_t)HR * HC * (C + 8) * sizeof(T);
  return conv_widest_nt(conv_nt(p.Cout), 8, [&](int nt) { return halo + (size_t)16 * nt * p.Kpad * sizeof(T) <= 158 * 1024; });
}

template <typename T>
static int dispatch_halo(ConvP p, int ngroup, hipStream_t st) {
  if (p.k != 3 || p.nsrc != 1 || p.srcUp[0] || p.srcC[0] > 64 || p.srcC[0] < tune().halo_min_c) return 0;  // measured: wins for Cin=64 on large maps
  const int S = p.stride;
  {  // the per-thread register halo holds HV=10 vectors
    const int MT = (S == 1) ? 2 : 1, HR = 7 * S + 3, HC = (16 * MT - 1) * S + 3;
    if ((long)HR * HC * (p.srcC[0] >> 3) > 512L * 10) return 0;
  }
  if (!conv_src_views<T>(p, ngroup)) return 0;
  p.NTpack = conv_nt(p.Cout);
  p.LSw = p.Kpad;
  const int nt = halo_pick_nt<T>(p, S);
  return conv_pick<1, 2, 4, 5, 8>(nt, [&](auto NT) { return conv_pick<1, 2>(S, [&](auto S_) { return halo_launch<T, NT, S_>(p, ngroup, st); }); });
}

// ---- 3x3 tile dispatch (conv3_tile_kernel; f16 throughput mode, the f32 parity mode keeps the exact-f32 kernels)
template <typename T, int NT, int S>
static int tile_launch(ConvP p, int ngroup, hipStream_t st) {
  constexpr int TR = 8, TC = (S == 1) ? 32 : 16, HR = (TR - 1) * S + 3, HC = (TC - 1) * S + 3, LROW = (S == 1) ? HC : 2 * ((HC + 1) / 2);
  const bool wlds = tune().tile_wlds == 1 || (tune().tile_wlds == 2 && S == 1);
  const size_t lds = ((size_t)HR * LROW + (wlds ? 9 * 16 * NT : 0)) * 40 * sizeof(T);
  p.tTR = TR; p.tTC = TC;
  if (S == 1 && tune().tile_flat) conv_flat_tile(p.Ho, p.Wo, p.tTR, p.tTC);
  const long tiles = (long)p.B * ((p.Wo + p.tTC - 1) / p.tTC) * ((p.Ho + p.tTR - 1) / p.tTR);
  const dim3 grid((unsigned)tiles, (unsigned)(conv_cout_pad(p.Cout) / (16 * NT)), (unsigned)ngroup);
  p.xcd = (int)((tune().xcd_map >> 4) & 1) && grid.y == 1 && grid.z == 1;  // (x alone decides the XCD only for a 1-D grid)
  (void)ey_lds_reserve<conv3_tile_kernel<T, NT, S, true>>(100 * 1024);  // up to 46 + 46 KB of dynamic LDS; opted in whatever this call needs
  if (wlds) hipLaunchKernelGGL((conv3_tile_kernel<T, NT, S, true>), grid, dim3(256), lds, st, p);
  else hipLaunchKernelGGL((conv3_tile_kernel<T, NT, S, false>), grid, dim3(256), lds, st, p);
  EY_LAUNCH_CHECK("ey_conv2d(tile)");
  g_last_variant = V_TILE + NT * 10 + S;
  return 1;
}

template <typename T>
static int dispatch_tile(ConvP p, int ngroup, hipStream_t st) {
  if constexpr (sizeof(T) != 2) return 0;
  else {
    if (p.k != 3 || p.nsrc != 1 || p.srcUp[0] || 9L * p.srcC[0] < tune().tile_mink) return 0;
    if (p.stride == 2 && (p.srcC[0] < tune().tile_s2_minc || (long)p.B * p.Ho * p.Wo < tune().tile_s2_minm)) return 0;
    const int ntp = conv_nt(p.Cout);
    int nt = ntp % 4 == 0 ? 4 : ntp == 2 ? 2 : ntp == 1 ? 1 : 0;
    if (!nt) return 0;
    // small maps: too few tiles to fill 256 CUs -> narrower channel tiles (more workgroups) beat the bigger register tile
    if (p.stride == 1 && tune().tile_minwg > 0) {
      const long tiles = (long)p.B * (((long)p.Ho * p.Wo + 239) / 240);
      while (nt > 1 && tiles * (conv_cout_pad(p.Cout) / (16 * nt)) * ngroup < tune().tile_minwg) nt >>= 1;
    }
    if (!conv_src_views<T>(p, ngroup) || !conv_weights_fit<T>(p)) return 0;
    p.NTpack = ntp;
    return conv_pick<1, 2, 4>(nt, [&](auto NT) { return conv_pick<1, 2>(p.stride, [&](auto S) { return tile_launch<T, NT, S>(p, ngroup, st); }); });
  }
}

// ---- register-stationary 3x3 dispatch (conv3r_kernel; f16, Cin == 16)
template <int NT, int S>
static int c3r_launch(const ConvP& p, int ngroup, hipStream_t st) {
  int occ = ey_occupancy<conv3r_kernel<NT, S>>(256, 0);
  if (occ > 4) occ = 4;
  const long ntile = (long)p.B * p.Ho * ((p.Wo + 15) / 16);
  if (ntile >= (1L << 31)) return 0;
  long gx = (long)256 * occ / ngroup / tune().grid_div;
  if (gx > (ntile + 3) / 4) gx = (ntile + 3) / 4;
  if (gx < 1) gx = 1;
  hipLaunchKernelGGL((conv3r_kernel<NT, S>), dim3((unsigned)gx, 1, (unsigned)ngroup), dim3(256), 0, st, p);
  EY_LAUNCH_CHECK("ey_conv2d(c3r)");
  g_last_variant = V_C3R + NT * 10 + S;
  return 1;
}

template <typename T>
static int dispatch_c3r(ConvP p, int ngroup, hipStream_t st) {
  if constexpr (sizeof(T) != 2) return 0;
  else {
    if (!tune().c3r || p.k != 3 || p.nsrc != 1 || p.srcUp[0] || p.srcC[0] != 16 || (p.srcCs[0] * 2) % 8) return 0;
    if (p.stride != 2 && tune().c3r < 2) return 0;  // measured: wins for the stride-2 layer (68 -> 58 us), loses 10 % to the tile kernel at stride 1
    const int ntp = conv_nt(p.Cout);
    if (ntp > 2 || conv_cout_pad(p.Cout) != 16 * ntp) return 0;
    if (!conv_src_views<T>(p, ngroup)) return 0;
    p.NTpack = ntp;
    return conv_pick<1, 2>(ntp, [&](auto NT) { return conv_pick<1, 2>(p.stride, [&](auto S) { return c3r_launch<NT, S>(p, ngroup, st); }); });
  }
}

// ---- persistent 3x3 tile kernel dispatch (conv3p_kernel; f16, Cin = 64, stride 1, Cout a multiple of 64)
template <int NT>
static int c3p_launch(ConvP p, hipStream_t st) {
  p.tTR = 8; p.tTC = 32;
  conv_flat_tile(p.Ho, p.Wo, p.tTR, p.tTC);
  const long tiles = (long)p.B * ((p.Wo + p.tTC - 1) / p.tTC) * ((p.Ho + p.tTR - 1) / p.tTR);
  if (tiles >= (1L << 30)) return 0;
  const int ny = conv_cout_pad(p.Cout) / (16 * NT);
  const size_t lds = ((size_t)9 * 16 * NT + 340) * 80 * 2;
  if (!ey_lds_reserve<conv3p_kernel<NT, true>>(lds) || !ey_lds_reserve<conv3p_kernel<NT, false>>(lds)) return 0;
  long gx = 256 / ny;
  if (gx < 1) gx = 1;
  if (gx > tiles) gx = tiles;
  // the interleaved epilogue: bias + SiLU only, whole 16-byte-aligned channel tiles, output view addressable with 32-bit offsets
  const long ybytes = (((long)p.B * p.Ho * p.Wo - 1) * p.yCs + p.Cout) * 2L;
  const bool fast = tune().c3p_fast && p.bias && p.act == EY_ACT_SILU && p.out_scale == 1.f && !p.res && !p.addz && p.vec_store == 2 && p.Cout % (16 * NT) == 0 &&
                    ybytes < (1L << 31);
  p.srcBytes[1] = fast ? (unsigned)ybytes : 0u;
  const dim3 gg((unsigned)gx, (unsigned)ny, 1);
  if (fast) hipLaunchKernelGGL((conv3p_kernel<NT, true>), gg, dim3(256), lds, st, p);
  else hipLaunchKernelGGL((conv3p_kernel<NT, false>), gg, dim3(256), lds, st, p);
  EY_LAUNCH_CHECK("ey_conv2d(c3p)");
  g_last_variant = V_C3P + NT * 10 + (fast ? 1 : 0);
  return 1;
}

template <typename T>
static int dispatch_c3p(ConvP p, int ngroup, hipStream_t st) {
  if constexpr (sizeof(T) != 2) return 0;
  else {
    if (!tune().c3p || p.k != 3 || p.stride != 1 || p.nsrc != 1 || p.srcUp[0] || ngroup != 1 || p.srcC[0] != 64) return 0;
    const int ntp = conv_nt(p.Cout);
    if (ntp % 4 != 0 || conv_cout_pad(p.Cout) % 64) return 0;
    const long M = (long)p.B * p.Ho * p.Wo;
    if (tune().c3p < 2 && M < tune().c3p_min_m) return 0;
    if (!conv_src_views<T>(p, ngroup) || !conv_weights_fit<T>(p)) return 0;
    p.NTpack = ntp;
    return c3p_launch<4>(p, st);
  }
}

// ---- 3x3 stream kernel dispatch (conv3s_kernel; f16, Cin in {64, 128, 256}, one source, no groups)
template <int NT, int MT, int UPT, int S, int NB>
static int c3s_launch(ConvP p, hipStream_t st) {
  const size_t lds = (size_t)16 * NT * p.LSw * 2;
  if (!ey_lds_reserve<conv3s_kernel<NT, MT, UPT, S, NB>>(lds)) return 0;
  const long M = (long)p.B * p.Ho * p.Wo;
  p.ntile = (M + 16 * MT - 1) / (16 * MT);
  const int ny = conv_cout_pad(p.Cout) / (16 * NT);
  long gx = 256 / ny;  // one workgroup per CU over all channel tiles
  if (gx < 1) gx = 1;
  if (gx * 8 > p.ntile) gx = (p.ntile + 7) / 8;
  p.xcd = (int)((tune().xcd_map >> 3) & 1) && (ny == 1 || gx % 8 == 0);
  hipLaunchKernelGGL((conv3s_kernel<NT, MT, UPT, S, NB>), dim3((unsigned)gx, (unsigned)ny, 1), dim3(512), lds, st, p);
  EY_LAUNCH_CHECK("ey_conv2d(c3s)");
  g_last_variant = V_C3S + NT * 100 + MT * 10 + (NB == 9 ? 5 : 0) + S;
  return 1;
}

template <typename T>
static int dispatch_c3s(ConvP p, int ngroup, hipStream_t st) {
  if constexpr (sizeof(T) != 2) return 0;
  else {
    if (!tune().c3s || p.k != 3 || p.nsrc != 1 || p.srcUp[0] || ngroup != 1) return 0;
    const int Cin = p.srcC[0];
    if (Cin != 64 && Cin != 128 && Cin != 256) return 0;
    const int ntp = conv_nt(p.Cout);
    if (conv_cout_pad(p.Cout) != p.Cout && conv_cout_pad(p.Cout) / 16 != ntp) return 0;
    // widest channel tile whose [16*NT][Kpad] weights fit one CU's LDS
    const int nt = conv_widest_nt(ntp, 4, [&](int n) { return (size_t)16 * n * p.Kpad * 2 <= 156 * 1024; });
    if (!nt) return 0;
    if (!conv_src_views<T>(p, ngroup) || !conv_weights_fit<T>(p)) return 0;
    p.NTpack = ntp;
    p.LSw = p.Kpad;
    const long M = (long)p.B * p.Ho * p.Wo;
    // Measured at batch 32 (tools/c3s_bench.sh, profiles/r03_c3s_vs_tile.txt): the stream kernel wins where the layer is big enough to
    // keep every CU streaming -- the stride-2 down-sampling convs (layer 3: 68 -> 47 us, 5: 56 -> 38, 7: 34 -> 27, 17: 19.5 -> 16) -- and
    // loses to the LDS-halo tile kernel at stride 1 (every input line goes through the vector-memory path 9 times: L2 hits, but at
    // ~30 B/clk per CU that is 13 us for the 80x80 box-tower convs) and on the smallest maps.  c3s = 2 forces it everywhere (tests).
    const long work = M * (conv_cout_pad(p.Cout) / (16 * nt));
    if (tune().c3s < 2 && (p.stride != 2 || work < tune().c3s_min_work)) return 0;
    // wave tile: 4 pixel blocks per wave on the big layers, 2 (more, smaller wave tiles) otherwise
    long cfg = tune().c3s_cfg;  // (developer knob: MT * 10 + ring depth)
    if (!cfg) cfg = (nt == 4 && M >= tune().c3s_mt4_m) ? 43 : 23;
    // (NT, MT) in {(4, 4), (4, 2), (2, 2), (1, 2)}; UPT = Cin / 64; ring depth 3
    const auto go = [&](auto NT, auto MT) {
      return conv_pick<1, 2, 4>(Cin / 64, [&](auto UPT) { return conv_pick<1, 2>(p.stride, [&](auto S) { return c3s_launch<NT, MT, UPT, S, 3>(p, st); }); });
    };
    if (nt == 4 && cfg == 43) return go(std::integral_constant<int, 4>(), std::integral_constant<int, 4>());
    return conv_pick<1, 2, 4>(nt, [&](auto NT) { return go(NT, std::integral_constant<int, 2>()); });
  }
}

// ---- small-M dispatch (conv_small_kernel)
template <typename T, int NT>
static int small_launch(ConvP p, int ngroup, hipStream_t st) {
  constexpr int BATCH = sizeof(T) == 2 ? 8 : 4;
  const long M = (long)p.B * p.Ho * p.Wo;
  p.ntile = (M + 15) / 16;
  p.ntn = conv_cout_pad(p.Cout) / (16 * NT);
  const long waves = p.ntile * p.ntn;
  hipLaunchKernelGGL((conv_small_kernel<T, NT, BATCH>), dim3((unsigned)((waves + 3) / 4), 1, ngroup), dim3(256), 0, st, p);
  EY_LAUNCH_CHECK("ey_conv2d(small)");
  g_last_variant = V_SMALL + NT * 10 + BATCH;
  return 1;
}

static int small_pick_nt(int Cout, int es) {  // <= 5 in f16, <= 2 in f32; NT = 1 always qualifies
  return conv_widest_nt(conv_nt(Cout), es == 2 ? 5 : 2, [](int) { return true; });
}

// The latency-oriented kernel wins (measured) for 1x1 convs on small maps as long as the weights every wave re-reads
// from L2 stay a small total: (#16-pixel tiles) x (weight bytes) <= 48 MB.  Larger weights: weight-stationary kernel.
static bool small_ok(int Cout, int Kpad, int k, long M, int es) {
  if (k != 1 || M >= tune().small_m) return false;
  return ((M + 15) / 16) * (long)conv_cout_pad(Cout) * Kpad * es <= (tune().small_wmb << 20);
}

template <typename T>
static int dispatch_small(ConvP p, int ngroup, hipStream_t st) {
  const long M = (long)p.B * p.Ho * p.Wo;
  if (!small_ok(p.Cout, p.Kpad, p.k, M, sizeof(T))) return 0;
  if (!conv_src_views<T>(p, ngroup)) return 0;
  conv_count_k(p);
  if (p.nsrc == 1) { p.srcC[1] = p.srcC[0]; p.srcCs[1] = p.srcCs[0]; p.srcUp[1] = p.srcUp[0]; p.src[1] = p.src[0]; }  // the kernel reads slot 1 either way
  p.NTpack = conv_nt(p.Cout);
  const int nt = small_pick_nt(p.Cout, sizeof(T));
  const auto go = [&](auto NT) { return small_launch<T, NT>(p, ngroup, st); };
  if constexpr (sizeof(T) == 2) return conv_pick<1, 2, 4, 5>(nt, go);
  else return conv_pick<1, 2>(nt, go);
}

// ---- lean pointwise dispatch (conv_pw_kernel)
static int pw_pick_nt(int Cout, long mtiles, int es) {
  const int ntp = conv_nt(Cout), rows = conv_cout_pad(Cout) / 16;
  const int opts[5] = {8, 5, 4, 2, 1};
  int pick = 0;
  for (int i = 0; i < 5; ++i) {
    const int nt = opts[i];
    if (nt > ntp || ntp % nt || (es == 4 && nt > 4)) continue;
    pick = nt;  // candidates come widest first; keep narrowing until there are enough waves (but stay >= 2 for 16-byte stores)
    if (mtiles * (rows / nt) >= tune().pw_waves || nt <= 2) break;
  }
  return pick;
}

template <typename T, int NT, int TWO, int GEO>
static int pw_launch(const ConvP& p, hipStream_t st) {
  // k-steps in flight per wave: as many as keep the wave at <= ~128 VGPRs (4 waves per SIMD)
  constexpr int BATCH = (sizeof(T) == 2 ? (NT <= 2 ? 8 : NT <= 5 ? 4 : 2) : (NT <= 2 ? 4 : 2));
  const dim3 grid((unsigned)((p.ntile + 3) / 4), (unsigned)(conv_cout_pad(p.Cout) / (16 * NT)), 1);
  hipLaunchKernelGGL((conv_pw_kernel<T, NT, BATCH, TWO != 0, GEO != 0>), grid, dim3(256), 0, st, p);
  EY_LAUNCH_CHECK("ey_conv2d(pw)");
  g_last_variant = V_PW + NT * 10 + (TWO ? 2 : 1);
  return 1;
}

template <typename T>
static int dispatch_pw(ConvP p, int ngroup, hipStream_t st) {
  const long M = (long)p.B * p.Ho * p.Wo;
  if (p.k != 1 || p.stride != 1 || ngroup != 1 || M >= tune().pw_m) return 0;
  if (((M + 15) / 16) * (long)conv_cout_pad(p.Cout) * p.Kpad * (long)sizeof(T) > (tune().pw_wmb << 20)) return 0;  // every wave re-reads its weight rows
  if (!conv_weights_fit<T>(p) || !conv_src_views<T>(p, ngroup)) return 0;
  p.ntile = (M + 15) / 16;
  p.NTpack = conv_nt(p.Cout);
  const int nt = pw_pick_nt(p.Cout, p.ntile, sizeof(T));  // <= 4 in f32
  const bool two = p.nsrc == 2, geo = p.addz != nullptr || p.srcUp[0] || (two && p.srcUp[1]);
  const auto go = [&](auto NT) {
    return conv_pick<0, 1>(two, [&](auto TWO) { return conv_pick<0, 1>(geo, [&](auto GEO) { return pw_launch<T, NT, TWO, GEO>(p, st); }); });
  };
  if constexpr (sizeof(T) == 2) return conv_pick<1, 2, 4, 5, 8>(nt, go);
  else return conv_pick<1, 2, 4>(nt, go);
}

// ---- register-stationary pointwise dispatch (conv_pwr_kernel; f16 -- an f32 fragment is twice the registers; large maps, few channels)
template <typename T, int NT, int KS, int TWO, int GEO>
static int pwr_launch(const ConvP& p, hipStream_t st) {
  // persistent grid = exactly the waves that are resident at once (register-limited), tiles dealt round-robin
  int occ = ey_occupancy<conv_pwr_kernel<T, NT, KS, TWO != 0, GEO != 0>>(256, 0);
  if (occ > 4) occ = 4;
  const unsigned ny = (unsigned)(conv_cout_pad(p.Cout) / (16 * NT));
  long gx = (long)256 * occ / ny / tune().grid_div;
  const long need = (p.ntile + 3) / 4;
  if (gx > need) gx = need;
  if (gx < 1) gx = 1;
  hipLaunchKernelGGL((conv_pwr_kernel<T, NT, KS, TWO != 0, GEO != 0>), dim3((unsigned)gx, ny, 1), dim3(256), 0, st, p);
  EY_LAUNCH_CHECK("ey_conv2d(pwr)");
  g_last_variant = V_PWR + NT * 10 + KS;
  return 1;
}

template <typename T>
static int dispatch_pwr(ConvP p, int ngroup, hipStream_t st) {
  if constexpr (sizeof(T) != 2) return 0;
  else {
    const long M = (long)p.B * p.Ho * p.Wo;
    if (p.k != 1 || p.stride != 1 || ngroup != 1 || M < tune().pwr_m || !p.vec_store || M >= (1L << 27)) return 0;
    const int ntp = conv_nt(p.Cout);
    if (conv_cout_pad(p.Cout) != 16 * ntp) return 0;  // one channel tile covers Cout (Cout <= 128)
    if (p.Cout != 16 * ntp) return 0;  // ... exactly: the epilogue stores whole 4*NT-channel groups with no channel-tail predicate
    const int ks = (p.srcC[0] + 31) / 32 + (p.nsrc == 2 ? (p.srcC[1] + 31) / 32 : 0);
    if (ks * ntp > tune().pwr_frags || ks > 4) return 0;
    if (!conv_src_views<T>(p, ngroup)) return 0;
    p.ntile = (M + 15) / 16;
    p.NTpack = ntp;
    const bool two = p.nsrc == 2, geo = p.addz != nullptr || p.srcUp[0] || (two && p.srcUp[1]);
    return conv_pick<1, 2, 4, 5, 8>(ntp, [&](auto NT) {
      return conv_pick<1, 2, 3, 4>(ks, [&](auto KS) {
        if constexpr (KS == 4 && NT > 4) return 0;  // (no such instantiation: too many fragments for the register file)
        else return conv_pick<0, 1>(two, [&](auto TWO) { return conv_pick<0, 1>(geo, [&](auto GEO) { return pwr_launch<T, NT, KS, TWO, GEO>(p, st); }); });
      });
    });
  }
}

// ---- N-split pointwise kernel (conv_pwn_kernel): f16, small maps, K = 128 ... 512, Cout % 128 == 0
template <int KS, int NTW>
static int pwn_launch(ConvP p, hipStream_t st) {
  int units = KS * 4;
  while ((units & 3) != 2) ++units;  // LDS pixel pitch: 2 (mod 4) 16-byte units (conflict-free fragment reads)
  p.LSw = units * 8;
  const size_t lds = (size_t)64 * p.LSw * 2;
  if (!ey_lds_reserve<conv_pwn_kernel<KS, NTW>>(lds)) return ey_set_error(EY_ELAUNCH, "conv(pwn): cannot reserve %zu B of LDS", lds);
  const long M = (long)p.B * p.Ho * p.Wo;
  hipLaunchKernelGGL((conv_pwn_kernel<KS, NTW>), dim3((unsigned)((M + 63) / 64), (unsigned)(p.Cout / (128 * NTW))), dim3(512), lds, st, p);
  EY_LAUNCH_CHECK("ey_conv2d(pwn)");
  g_last_variant = V_PWN + KS * 10 + NTW;
  return 1;
}

template <typename T>
static int dispatch_pwn(ConvP p, int ngroup, hipStream_t st) {
  if constexpr (sizeof(T) != 2) return 0;
  else {
    const long M = (long)p.B * p.Ho * p.Wo;
    if (!tune().pwn || p.k != 1 || p.stride != 1 || ngroup != 1 || M > tune().pwn_max_m || M < 1024 || p.Cout % 128 || p.res || p.addz || p.out_scale != 1.f ||
        p.vec_store != 2 || (p.bias && !ey_aligned(p.bias, 16)))
      return 0;
    int K = 0;
    for (int s = 0; s < p.nsrc; ++s) {
      if (p.srcC[s] % 32) return 0;
      K += p.srcC[s];
    }
    if (!conv_src_views<T>(p, ngroup)) return 0;
    if (K < 128 || K > 512 || M * p.yCs * 2 >= (1L << 31)) return 0;
    p.NTpack = 8;
    p.Ctot = K;
    long ntw = tune().pwn_ntw;
    if (ntw != 1 && ntw != 2) ntw = (p.Cout % 256 == 0 && (M + 63) / 64 >= 192) ? 2 : 1;  // 256-channel slabs once the pixel tiles alone fill the chip
    if (p.Cout % 256) ntw = 1;
    return conv_pick<4, 6, 8, 12, 16>(K / 32, [&](auto KS) { return conv_pick<1, 2>((int)ntw, [&](auto NTW) { return pwn_launch<KS, NTW>(p, st); }); });
  }
}

// ---- ey_conv2d: the first kernel that takes the shape runs it.  Order matters -- the specialised kernels come before the general
// ones they beat on their shapes: lean pointwise, N-split pointwise, register-stationary pointwise, small-M, then the 3x3 kernels
// (register-stationary, stream, persistent tile, tile, halo tile), then weight-stationary; the K-chunked kernel takes what is left.
// A dispatcher returns 1 = launched, 0 = not mine, < 0 = error; the walk stops at the first non-zero.
template <typename T>
static int conv2d_typed(const ConvP& p, int ngroup, hipStream_t st) {
  static int (*const order[])(ConvP, int, hipStream_t) = {dispatch_pw<T>,  dispatch_pwn<T>, dispatch_pwr<T>,  dispatch_small<T>, dispatch_c3r<T>,
                                                          dispatch_c3s<T>, dispatch_c3p<T>, dispatch_tile<T>, dispatch_halo<T>,  dispatch_ws<T>};
  for (const auto dispatch : order) {
    const int rc = dispatch(p, ngroup, st);
    if (rc != 0) return rc < 0 ? rc : EY_OK;
  }
  const int rc = dispatch_igemm<T>(p, ngroup, st);
  return rc < 0 ? rc : EY_OK;
}

// the f16 and f32 instantiations live in two translation units (conv_f16.hip / conv_f32.hip) so that they compile in parallel
int ey_conv2d_run_f16(const ConvP& p, int ngroup, hipStream_t st);
int ey_conv2d_run_f32(const ConvP& p, int ngroup, hipStream_t st);
#if EY_CONV_PART == 32
int ey_conv2d_run_f32(const ConvP& p, int ngroup, hipStream_t st) { return conv2d_typed<float>(p, ngroup, st); }
#else
int ey_conv2d_run_f16(const ConvP& p, int ngroup, hipStream_t st) { return conv2d_typed<f16>(p, ngroup, st); }

static int conv_desc_to_p(const ey_conv_desc* d, ConvP& p, int& ngroup) {
  EY_CHECK(d, "conv: null desc");
  EY_CHECK(d->dtype == EY_F16 || d->dtype == EY_F32, "conv: bad dtype %d", d->dtype);
  const int es = d->dtype == EY_F16 ? 2 : 4;
  EY_CHECK(d->B > 0 && d->H > 0 && d->W > 0 && d->Cout > 0, "conv: bad extent B=%d H=%d W=%d Cout=%d", d->B, d->H, d->W, d->Cout);
  EY_CHECK((d->k == 1 || d->k == 3) && (d->stride == 1 || d->stride == 2) && d->pad == d->k / 2,
           "conv: k=%d stride=%d pad=%d unsupported by the MFMA kernel (use ey_conv2d_direct)", d->k, d->stride, d->pad);
  EY_CHECK(d->Ho == (d->H + 2 * d->pad - d->k) / d->stride + 1 && d->Wo == (d->W + 2 * d->pad - d->k) / d->stride + 1,
           "conv: Ho/Wo (%d,%d) inconsistent with H/W (%d,%d)", d->Ho, d->Wo, d->H, d->W);
  EY_CHECK(d->nsrc == 1 || d->nsrc == 2, "conv: nsrc=%d", d->nsrc);
  EY_CHECK(d->w && d->y, "conv: null weight/output");
  int Cin = 0;
  for (int s = 0; s < d->nsrc; ++s) {
    EY_CHECK(d->src[s], "conv: null src%d", s);
    EY_CHECK(d->src_C[s] > 0 && d->src_C[s] % 8 == 0, "conv: src%d channels %d not a multiple of 8 (use ey_conv2d_direct)", s, d->src_C[s]);
    EY_CHECK(d->src_cstride[s] >= d->src_C[s] && (d->src_cstride[s] * es) % 16 == 0 && ey_aligned(d->src[s], 16),
             "conv: src%d view (cstride %d) not 16-byte aligned", s, d->src_cstride[s]);
    EY_CHECK(d->src_up[s] == 0 || d->src_up[s] == 1, "conv: src_up must be 0/1");
    EY_CHECK(!d->src_up[s] || (d->H % 2 == 0 && d->W % 2 == 0), "conv: upsampled source needs even H,W");
    Cin += d->src_C[s];
  }
  EY_CHECK(d->y_cstride >= d->Cout, "conv: y_cstride %d < Cout %d", d->y_cstride, d->Cout);
  EY_CHECK(!d->res || d->res_cstride >= d->Cout, "conv: res_cstride");
  EY_CHECK(!d->addz || (d->addz_H > 0 && d->addz_W > 0 && d->addz_cstride >= d->Cout), "conv: addz extent/cstride");
  ngroup = d->ngroup > 0 ? d->ngroup : 1;
  EY_CHECK(ngroup == 1 || d->nsrc == 1, "conv: ngroup>1 needs a single source");
  p.B = d->B; p.H = d->H; p.W = d->W; p.Ho = d->Ho; p.Wo = d->Wo; p.Cout = d->Cout; p.k = d->k; p.stride = d->stride;
  p.pad = d->pad; p.act = d->act; p.nsrc = d->nsrc;
  for (int s = 0; s < 2; ++s) {
    p.src[s] = s < d->nsrc ? d->src[s] : nullptr;
    p.srcC[s] = s < d->nsrc ? d->src_C[s] : 0;
    p.srcCs[s] = s < d->nsrc ? d->src_cstride[s] : 0;
    p.srcUp[s] = s < d->nsrc ? d->src_up[s] : 0;
  }
  p.w = d->w; p.bias = d->bias; p.y = d->y; p.yCs = d->y_cstride; p.res = d->res; p.resCs = d->res_cstride;
  p.out_scale = d->out_scale; p.addz = d->addz; p.addzCs = d->addz_cstride; p.Hz = d->addz_H; p.Wz = d->addz_W;
  p.zsy = d->addz ? (float)d->addz_H / (float)d->Ho : 0.f; p.zsx = d->addz ? (float)d->addz_W / (float)d->Wo : 0.f; p.srcG = d->src_gstride; p.yG = d->y_gstride;
  p.wG = d->w_gstride; p.wGmax = d->w_gmax > 0 ? d->w_gmax : 0;
  p.Kpad = conv_kpad(Cin, d->k, es);
  p.xcd = 0;
  p.nchunks = 0;
  for (int s2 = 0; s2 < d->nsrc; ++s2) p.nchunks += (d->src_C[s2] + CONV_CH - 1) / CONV_CH;
  p.nchunks *= d->k * d->k;
  const int va = 4 * es;  // 4-element vector access alignment
  p.vec_store = d->Cout % 4 == 0 && (d->y_cstride * es) % va == 0 && ey_aligned(d->y, va) && (d->y_gstride * es) % va == 0 &&
                (!d->res || ((d->res_cstride * es) % va == 0 && ey_aligned(d->res, va))) &&
                (!d->addz || ((d->addz_cstride * es) % va == 0 && ey_aligned(d->addz, va))) && (!d->bias || ey_aligned(d->bias, 16));
  if (p.vec_store && (d->y_cstride * es) % 16 == 0 && ey_aligned(d->y, 16) && (d->y_gstride * es) % 16 == 0 &&
      (!d->res || ((d->res_cstride * es) % 16 == 0 && ey_aligned(d->res, 16))))
    p.vec_store = 2;  // 16-byte epilogue accesses allowed
  return EY_OK;
}

extern "C" int ey_conv2d(const ey_conv_desc* d, ey_stream_t stream) {
  ConvP p;
  int ngroup = 1;
  const int rc = conv_desc_to_p(d, p, ngroup);
  if (rc != EY_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  g_last_variant = 0;
  return d->dtype == EY_F16 ? ey_conv2d_run_f16(p, ngroup, st) : ey_conv2d_run_f32(p, ngroup, st);
}

// ---- two chained pointwise convs (conv_pwc_kernel): the second reads exactly what the first writes
extern "C" int ey_conv_pw_pair(const ey_conv_desc* first, const ey_conv_desc* second, ey_stream_t stream) {
  ConvP p, q;
  int g1 = 1, g2 = 1;
  int rc = conv_desc_to_p(first, p, g1);
  if (rc != EY_OK) return rc;
  rc = conv_desc_to_p(second, q, g2);
  if (rc != EY_OK) return rc;
  const long M = (long)p.B * p.Ho * p.Wo;
  const int nt = conv_nt(p.Cout);
  const bool fits = tune().pwc && first->dtype == EY_F16 && second->dtype == EY_F16 && g1 == 1 && g2 == 1 && p.k == 1 && q.k == 1 && p.stride == 1 && q.stride == 1 &&
                    p.nsrc == 1 && q.nsrc == 1 && !p.srcUp[0] && !q.srcUp[0] && (p.Cout == 64 || p.Cout == 128) && q.Cout == p.Cout && q.srcC[0] == p.Cout &&
                    p.srcC[0] % 32 == 0 && p.srcC[0] <= 128 && q.src[0] == p.y && q.srcCs[0] == p.yCs && q.B == p.B && q.H == p.Ho && q.W == p.Wo && !q.res && !q.addz &&
                    q.y != p.y && p.vec_store == 2 && q.vec_store == 2 && M <= tune().pw_m && nt * 16 == p.Cout;
  if (!fits) return ey_set_error(EY_EUNSUPPORTED, "conv_pw_pair: shapes outside the chained kernel (f16, 1x1 -> 1x1, 64 or 128 channels, small maps)");
  for (ConvP* c : {&p, &q}) {
    if (!conv_src_views<f16>(*c, 1)) return ey_set_error(EY_EUNSUPPORTED, "conv_pw_pair: view larger than 2 GiB");
    c->NTpack = nt;
    c->ntile = (M + 15) / 16;
  }
  const dim3 grid((unsigned)((p.ntile + 3) / 4));
  const bool ag = tune().pwc == 2;
  if (nt == 4) {
    if (ag) hipLaunchKernelGGL((conv_pwc_kernel<4, true>), grid, dim3(256), 0, (hipStream_t)stream, p, q);
    else hipLaunchKernelGGL((conv_pwc_kernel<4, false>), grid, dim3(256), 0, (hipStream_t)stream, p, q);
  } else {
    if (ag) hipLaunchKernelGGL((conv_pwc_kernel<8, true>), grid, dim3(256), 0, (hipStream_t)stream, p, q);
    else hipLaunchKernelGGL((conv_pwc_kernel<8, false>), grid, dim3(256), 0, (hipStream_t)stream, p, q);
  }
  EY_LAUNCH_CHECK("ey_conv_pw_pair");
  return EY_OK;
}

// ---- chained pointwise pair (see conv_pw2_kernel)
extern "C" int ey_conv_chain_kperm(int Cmid, int* perm, int perm_len) {
  const int nt1 = conv_nt(Cmid);
  EY_CHECK(Cmid == 16 * nt1 && perm, "chain_kperm: Cmid=%d must be a whole channel tile (16, 32, 64, 80, 128)", Cmid);
  const int ks2 = (4 * nt1 + 7) / 8;
  EY_CHECK(perm_len == 32 * ks2, "chain_kperm: perm_len must be %d", 32 * ks2);
  for (int s2 = 0; s2 < ks2; ++s2)
    for (int g = 0; g < 4; ++g)
      for (int j = 0; j < 8; ++j) {
        const int idx = 8 * s2 + j;
        perm[32 * s2 + 8 * g + j] = idx < 4 * nt1 ? g * 4 * nt1 + idx : -1;  // -1: zero column
      }
  return EY_OK;
}
extern "C" int ey_conv_chain_klen(int Cmid) { const int nt1 = conv_nt(Cmid); return Cmid == 16 * nt1 ? 32 * ((4 * nt1 + 7) / 8) : 0; }

template <int NT1, int KS1, int NT2>
static int pw2_launch(const ConvP& p, const ChainP& q, hipStream_t st) {
  int occ = ey_occupancy<conv_pw2_kernel<NT1, KS1, NT2>>(256, 0);
  if (occ > 4) occ = 4;
  long gx = 256L * occ / tune().grid_div;
  if (gx > (p.ntile + 3) / 4) gx = (p.ntile + 3) / 4;
  if (gx < 1) gx = 1;
  hipLaunchKernelGGL((conv_pw2_kernel<NT1, KS1, NT2>), dim3((unsigned)gx), dim3(256), 0, st, p, q);
  EY_LAUNCH_CHECK("ey_conv_pw_chain");
  return EY_OK;
}

extern "C" int ey_conv_pw_chain(int dtype, int B, int H, int W, int Cin, int Cmid, int Cout, const void* x, int x_cstride, const void* w1_packed, const float* b1,
                                int act1, const void* w2_packed, const float* b2, int act2, void* y, int y_cstride, ey_stream_t stream) {
  EY_CHECK(dtype == EY_F16, "conv_pw_chain: f16 only");
  EY_CHECK(x && w1_packed && w2_packed && y && B > 0 && H > 0 && W > 0, "conv_pw_chain: bad arguments");
  const int nt1 = conv_nt(Cmid), nt2 = conv_nt(Cout), ks1 = (Cin + 31) / 32;
  // two shapes of the Detect class tower (head.py:59,68-70; c3 = max(ch[0], min(nc, 100))): nc = 80 -> 80 -> 80 -> 80, and small class
  // counts (GC10-DET, nc = 10: c3 = 64) -> 64 -> 64 -> nc <= 16
  const bool wide = nt1 == 5 && Cmid == 80 && nt2 == 5 && Cout <= 80 && Cout % 4 == 0 && ks1 == 3 && Cin % 8 == 0;
  const bool narrow = nt1 == 4 && Cmid == 64 && nt2 == 1 && Cout >= 1 && Cout <= 16 && ks1 == 2 && Cin % 8 == 0;
  if (!wide && !narrow)
    return ey_set_error(EY_EUNSUPPORTED, "conv_pw_chain: built for Cin 72..96 -> 80 -> <= 80 and Cin 40..64 -> 64 -> <= 16 (got %d -> %d -> %d)", Cin, Cmid, Cout);
  EY_CHECK(x_cstride >= Cin && (x_cstride * 2) % 16 == 0 && ey_aligned(x, 16) && y_cstride >= Cout && (y_cstride * 2) % 8 == 0 && ey_aligned(y, 8), "conv_pw_chain: view alignment");
  const long M = (long)B * H * W, bytes = ((M - 1) * x_cstride + Cin) * 2L;
  EY_CHECK(bytes < (1L << 31) && M < (1L << 27), "conv_pw_chain: tensor too large");
  ConvP p;
  p.B = B; p.H = H; p.W = W; p.Ho = H; p.Wo = W; p.Cout = Cmid; p.act = act1; p.nsrc = 1;
  p.src[0] = x; p.srcC[0] = Cin; p.srcCs[0] = x_cstride; p.srcBytes[0] = (unsigned)bytes;
  p.w = w1_packed; p.bias = b1; p.Kpad = conv_kpad(Cin, 1, 2); p.ntile = (M + 15) / 16;
  ChainP q;
  q.w2 = w2_packed; q.b2 = b2; q.act2 = act2; q.Cout2 = Cout; q.Kpad2 = conv_kpad(ey_conv_chain_klen(Cmid), 1, 2); q.y2 = y; q.y2Cs = y_cstride;
  return wide ? pw2_launch<5, 3, 5>(p, q, (hipStream_t)stream) : pw2_launch<4, 2, 1>(p, q, (hipStream_t)stream);
}

// A prediction for tools of the general kernel ey_conv2d falls back on for a shape, in a numbering of its own (NOT the codes of
// ey_conv_last_variant): 3000 + NT*10 + BATCH = conv_small_kernel<T,NT,BATCH>, 2000 + NT*10 + MT = conv3_halo_kernel<T,NT,stride>,
// 1000 + NT*10 + MT = conv_ws_kernel<T,NT,MT,k>, NT*10 + MT = conv_igemm_kernel<T,NT,MT>.  It knows nothing of the specialised kernels
// tried first (pw, pwn, pwr, c3r, c3s, c3p, tile) and its ws step assumes the default tunables; ey_conv_last_variant() reports what ran.
extern "C" int ey_conv_variant(int dtype, int Cout, int Cin, int k, int stride, int plain_single_source, long M, int ngroup) {
  const int es = dtype == EY_F16 ? 2 : 4, Kpad = conv_kpad(Cin, k, es);
  if (small_ok(Cout, Kpad, k, M, es)) return 3000 + small_pick_nt(Cout, es) * 10 + (es == 2 ? 8 : 4);
  if (k == 3 && plain_single_source && Cin <= 64 && Cin >= 48) {
    ConvP p;
    p.Cout = Cout; p.srcC[0] = Cin; p.Kpad = Kpad;
    const int MT = stride == 1 ? 2 : 1, HR = 7 * stride + 3, HC = (16 * MT - 1) * stride + 3;
    if ((long)HR * HC * (Cin >> 3) <= 512L * 10) {
      const int nt = es == 2 ? halo_pick_nt<f16>(p, stride) : halo_pick_nt<float>(p, stride);
      if (nt) return 2000 + nt * 10 + MT;
    }
  }
  int nt = ws_pick_nt(Cout, Kpad, es, 76 * 1024);
  if (!nt) nt = ws_pick_nt(Cout, Kpad, es, 156 * 1024);
  if (nt) return 1000 + nt * 10 + (M >= 300000 ? 2 : 1);
  nt = conv_nt(Cout);
  const int ntiles = (Cout + 16 * nt - 1) / (16 * nt);
  return nt * 10 + ((M + 127) / 128 * ntiles * (ngroup > 0 ? ngroup : 1) >= 512 ? 2 : 1);
}
extern "C" int ey_conv_pack_nt(int Cout) { return conv_nt(Cout); }
// kind*1000 + NT*10 + x of the kernel the last ey_conv2d on this thread launched (profiling labels and tests): kind 3 = conv_pwn<KS,NTW>
// (KS*10 + NTW), 4 = conv_pw<T,NT,..> (x = number of sources), 5 = conv_pwr<T,NT,KS>, 6 = conv3_tile<T,NT,S>, 7 = conv3r<NT,S>,
// 8 = conv3s<NT,MT,..> (NT*100 + MT*10 + 5 if the 9-deep ring + S), 9 = conv3p<NT,FAST>, 10 = conv_small<T,NT,BATCH>, 11 = conv3_halo<T,NT,S>,
// 12 = conv_ws<T,NT,MT,KS> (NT*100 + MT*10 + KS), 13 = conv_igemm<T,NT,MT>.
extern "C" int ey_conv_last_variant(void) { return g_last_variant; }
#endif  // EY_CONV_PART
