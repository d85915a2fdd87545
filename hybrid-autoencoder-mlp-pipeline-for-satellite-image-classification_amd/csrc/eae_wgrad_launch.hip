// Host-side dispatch of the generic 3x3 stride-2 weight-gradient kernel.
#include "eae_internal.h"
#include <cstdio>
#include <cstdlib>
#include "eae_wgrad.hip.h"
#include "eae_wgrad_plan.h"

namespace {
template <int CS, int CB, int TW, int TH, int NI, int SM, int BM>
int launch(const WgradArgs& a0, const WgS2Plan& p, float* scratch, float* dw, hipStream_t st, const EaeProfHook* hook) {
  WgradArgs a = a0;
  a.ntiles = p.ntiles;
  a.tiles_per_block = p.tiles_per_block;
  a.part = p.writes_dw ? dw : scratch;
  a.nslices = p.slices;
  constexpr size_t smem = WgGeo<TW, TH, NI>::smem();
  void (*kern)(WgradArgs) = wgrad_s2_kernel<CS, CB, TW, TH, NI, SM, BM>;
  void (*kern_g)(GroupPack<WgradArgs>, int) = wgrad_s2_kernel_g<CS, CB, TW, TH, NI, SM, BM>;
  if constexpr (TW == 16) { if (a.qs) kern = wgrad8_s2_kernel<CS, CB, TW, TH, NI, SM, BM>; }      // fp8 variant (BASELINE config 5)
  EAE_HIP(eae_smem_attr(eae_rec ? reinterpret_cast<const void*>(kern_g) : reinterpret_cast<const void*>(kern), smem));
  if (hook) hook->begin(hook->user, st);
  eae_launch(kern, kern_g, dim3(p.grid), dim3(WG_THREADS), smem, st, a);
  if (hook) hook->end(hook->user, st);
  EAE_LAUNCH_CHECK();
  if (p.writes_dw) return 0;
  launch_reduce_slices(st, scratch, p.slices, (long)((long long)CS * CB * 9 / 4), dw, 1.0f);
  EAE_LAUNCH_CHECK();
  return 0;
}

// EAE_WGRAD_WGS=<n> or <n one-block layers>,<n wider layers>[,<n last layer>], read once per process
struct WgsSetting { int one = 64, wide = 64, last = 64; };
const WgsSetting& wgs_setting() {
  static const WgsSetting s = [] {
    WgsSetting w;
    if (const char* e = getenv("EAE_WGRAD_WGS")) {
      int a = 0, b = 0, c = 0;
      const int n = sscanf(e, "%d,%d,%d", &a, &b, &c);
      if (n >= 1 && a > 0) { w.one = a; w.wide = (n >= 2 && b > 0) ? b : a; w.last = (n >= 3 && c > 0) ? c : w.one; }
    }
    return w;
  }();
  return s;
}

// the plan (eae_wgrad_plan.h) under this process's setting, then the instantiation of the geometry it names
template <int CS, int CB, int SM, int BM>
int geo(const WgradArgs& a, float* scratch, long long sf, float* dw, hipStream_t st, const EaeProfHook* hook) {
  constexpr bool LAST = (CS == 64 && (SM == SRC_BNBWD || SM == SRC_RAWG));      // enc.conv2's: the last weight gradient of the step
  const WgsSetting& w = wgs_setting();
  WgS2Plan p;
  const bool ok = eae_wgrad_s2_plan(p, CS, CB, LAST, a.qs != nullptr, a.B, a.Hs, a.Ws, sf, w.one, w.wide, w.last, eae_geo_mult);
  if (p.refused == WG_NO_GEOMETRY) return eae_set_error(-2, "wgrad: unsupported spatial size");
  if (p.refused == WG_SCRATCH) return eae_set_error(-2, "wgrad: scratch too small");
  if (a.qs) EAE_NO_GROUP("the fp8 weight-gradient kernel");
  if (!ok) return eae_set_error(-2, "wgrad: the fp8 variant needs small maps that are multiples of 8 x 16");
  if (p.tw == 16) return launch<CS, CB, 16, 8, 1, SM, BM>(a, p, scratch, dw, st, hook);
  if (p.tw == 8) return launch<CS, CB, 8, 8, 2, SM, BM>(a, p, scratch, dw, st, hook);
  return launch<CS, CB, 4, 4, 8, SM, BM>(a, p, scratch, dw, st, hook);
}
}  // namespace

int eae_launch_reduce_slices(hipStream_t st, const float* part, int nslices, long n4, float* out, float scale) {
  launch_reduce_slices(st, part, nslices, n4, out, scale);
  EAE_LAUNCH_CHECK();
  return 0;
}

// instantiations used by the path
//   conv2/3/4   : small = dy  (BNBWD), big = input activation (BNRELU): (64,32) (128,64) (256,128)
//   deconv3/2   : small = input activation (BNRELU), big = dOut (BNBWD): (64,32) (128,64)
//   deconv1     : small = dec.fc output (RAW),      big = dOut (BNBWD): (256,128)
int eae_launch_wgrad_s2(hipStream_t st, const WgradArgs& a, int cs, int cb, int smode, int bmode, float* scratch,
                        long long scratch_floats, float* dw, const EaeProfHook* hook) {
#define CASE(S, B_, SM, BM) if (cs == S && cb == B_ && smode == SM && bmode == BM) return geo<S, B_, SM, BM>(a, scratch, scratch_floats, dw, st, hook)
  CASE(64, 32, SRC_BNBWD, SRC_BNRELU);
  CASE(128, 64, SRC_BNBWD, SRC_BNRELU);
  CASE(256, 128, SRC_BNBWD, SRC_BNRELU);
  CASE(64, 32, SRC_BNRELU, SRC_BNBWD);
  CASE(128, 64, SRC_BNRELU, SRC_BNBWD);
  CASE(256, 128, SRC_RAW, SRC_BNBWD);
  CASE(64, 32, SRC_RAW, SRC_RAW);       // plain (tests)
  // the train step: the gradient operand is the dy tensor the layer's backward-data kernel wrote while staging it (SRC_RAWG)
  CASE(64, 32, SRC_RAWG, SRC_BNRELU);
  CASE(128, 64, SRC_RAWG, SRC_BNRELU);
  CASE(256, 128, SRC_RAWG, SRC_BNRELU);
  CASE(64, 32, SRC_BNRELU, SRC_RAWG);
  CASE(128, 64, SRC_BNRELU, SRC_RAWG);
  CASE(256, 128, SRC_RAW, SRC_RAWG);
#undef CASE
  return eae_set_error(-2, "wgrad: no kernel instantiated for this (cs, cb, modes)");
}
