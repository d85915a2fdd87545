// Host-side dispatch of the unified stride-2 conv / transposed-conv implicit-GEMM kernel (eae_igemm.hip.h): every decision is the
// plan's (eae_conv_plan.h); this unit maps a plan to the template instantiation and launches it on the plan's grid.
#include "eae_internal.h"
#include "eae_igemm.hip.h"
#include "eae_igemm2.hip.h"
#include "eae_conv_plan.h"
#include <cstdlib>

static_assert(S2_CONV == KIND_CONV && S2_DECONV == KIND_DECONV && EPI_FWD == 0, "eae_conv_plan.h mirrors these values of eae_args.h");

namespace {

// the plan of a layer as this thread launches it now: EAE_IGEMM2 and EAE_IG_SMALL are read once per process, the group
// multiplier is the thread's (eae_group.h)
void plan_here(S2Plan& p, int kind, int cin, int cout, int epi, bool fp8, int B, int Hin, int Win) {
  static const int igemm2_mode = getenv("EAE_IGEMM2") ? atoi(getenv("EAE_IGEMM2")) : 1;
  static const int ig_small = getenv("EAE_IG_SMALL") ? atoi(getenv("EAE_IG_SMALL")) : -1;
  eae_s2_plan(p, kind, cin, cout, epi, fp8, B, Hin, Win, eae_geo_mult, igemm2_mode, ig_small);      // (no geometry: p.geo says so)
}

// `kern` on the plan's grid -- or, inside a recorded grouped step, its twin `kern_g`
int run(void (*kern)(ConvArgs), void (*kern_g)(GroupPack<ConvArgs>, int), size_t smem, const ConvArgs& a, const S2Plan& p, hipStream_t st) {
  EAE_HIP(eae_smem_attr(eae_rec ? (const void*)kern_g : (const void*)kern, smem));
  ConvArgs b = a;
  b.ntiles = p.ntiles;
  bn_acc_set_limit(b.bacc, p.ntiles);
  eae_launch(kern, kern_g, dim3(p.grid), dim3(p.threads), smem, st, b);
  EAE_LAUNCH_CHECK();
  return 0;
}

template <int KIND, int CIN, int COUT, int BN, int TW, int TH, int NI, int SRC, int EPI>
int launch(const ConvArgs& a, const S2Plan& p, hipStream_t st) {
  return run(igemm_s2_kernel<KIND, CIN, COUT, BN, TW, TH, NI, SRC, EPI>, igemm_s2_kernel_g<KIND, CIN, COUT, BN, TW, TH, NI, SRC, EPI>,
             igemm_smem<KIND, BN, TW, TH, NI>(), a, p, st);
}
// fp8 variant (BASELINE config 5): same geometry, operands converted to fp8 (ConvArgs::qs set by the engine); 16-wide tiles only
template <int KIND, int CIN, int COUT, int BN, int TW, int TH, int NI, int SRC, int EPI>
int launch8(const ConvArgs& a, const S2Plan& p, hipStream_t st) {
  EAE_NO_GROUP("the fp8 implicit-GEMM kernel");
  return run(igemm8_s2_kernel<KIND, CIN, COUT, BN, TW, TH, NI, SRC, EPI>, nullptr, igemm_smem<KIND, BN, TW, TH, NI>(), a, p, st);
}
// wave-specialised kernel (eae_igemm2.hip.h)
template <int KIND, int CIN, int COUT, int BN, int TW, int TH, int NI, int SRC, int EPI, int NBL>
int launch2(const ConvArgs& a, const S2Plan& p, hipStream_t st) {
  return run(igemm2_s2_kernel<KIND, CIN, COUT, BN, TW, TH, NI, SRC, EPI, NBL>, igemm2_s2_kernel_g<KIND, CIN, COUT, BN, TW, TH, NI, SRC, EPI, NBL>,
             igemm2_smem<KIND, BN, TW, TH, NI, NBL>(), a, p, st);
}

// plan -> instantiation.  The `if constexpr` guards keep the set of instantiated kernels to what the plan can ask for: small tiles
// and the wave-specialised kernel from 64 input channels on (conv kind) / from 128 (transposed kind).
template <int CIN, int COUT, int BN, int SRC, int EPI>
int conv_geo(const ConvArgs& a, const S2Plan& p, hipStream_t st) {
  const bool ws = p.kern == S2_WAVE_SPEC;
  switch (p.geo) {
    case S2_GEO_16x8x1:
      return p.kern == S2_FP8 ? launch8<KIND_CONV, CIN, COUT, BN, 16, 8, 1, SRC, EPI>(a, p, st) : launch<KIND_CONV, CIN, COUT, BN, 16, 8, 1, SRC, EPI>(a, p, st);
    case S2_GEO_8x8x2:
      if constexpr (CIN >= 64) { if (ws) return launch2<KIND_CONV, CIN, COUT, BN, 8, 8, 2, SRC, EPI, (CIN == 64) ? COUT / BN : 1>(a, p, st); }
      return launch<KIND_CONV, CIN, COUT, BN, 8, 8, 2, SRC, EPI>(a, p, st);
    case S2_GEO_4x4x8:
      if constexpr (CIN >= 64) { if (ws) return launch2<KIND_CONV, CIN, COUT, BN, 4, 4, 8, SRC, EPI, (CIN == 64) ? COUT / BN : 1>(a, p, st); }
      return launch<KIND_CONV, CIN, COUT, BN, 4, 4, 8, SRC, EPI>(a, p, st);
    case S2_GEO_8x8x1:
      if constexpr (CIN >= 64) return launch<KIND_CONV, CIN, COUT, BN, 8, 8, 1, SRC, EPI>(a, p, st);
      break;
    case S2_GEO_4x4x4:
      if constexpr (CIN >= 64) return launch<KIND_CONV, CIN, COUT, BN, 4, 4, 4, SRC, EPI>(a, p, st);
      break;
  }
  if (a.qs) return eae_set_error(-2, "conv_s2: the fp8 variant needs output maps that are multiples of 8 x 16");
  return eae_set_error(-2, "conv_s2: unsupported spatial size (output must be 4x4, 8x8 or a multiple of 8x16)");
}

template <int CIN, int COUT, int BN, int SRC, int EPI>
int deconv_geo(const ConvArgs& a, const S2Plan& p, hipStream_t st) {
  const bool ws = p.kern == S2_WAVE_SPEC;
  switch (p.geo) {
    case S2_GEO_16x8x1:
      return p.kern == S2_FP8 ? launch8<KIND_DECONV, CIN, COUT, BN, 16, 8, 1, SRC, EPI>(a, p, st) : launch<KIND_DECONV, CIN, COUT, BN, 16, 8, 1, SRC, EPI>(a, p, st);
    case S2_GEO_8x8x1:
      if constexpr (CIN >= 128) { if (ws) return launch2<KIND_DECONV, CIN, COUT, BN, 8, 8, 1, SRC, EPI, 1>(a, p, st); }
      return launch<KIND_DECONV, CIN, COUT, BN, 8, 8, 1, SRC, EPI>(a, p, st);
    case S2_GEO_4x4x4:
      if constexpr (CIN >= 128) { if (ws) return launch2<KIND_DECONV, CIN, COUT, BN, 4, 4, 4, SRC, EPI, 1>(a, p, st); }
      return launch<KIND_DECONV, CIN, COUT, BN, 4, 4, 4, SRC, EPI>(a, p, st);
  }
  if (a.qs) return eae_set_error(-2, "deconv_s2: the fp8 variant needs input maps that are multiples of 8 x 16");
  return eae_set_error(-2, "deconv_s2: unsupported spatial size (input must be 4x4, 8x8 or a multiple of 8x16)");
}

}  // namespace

// conv-kind instantiations used by the path:
//   forward of enc.conv2/3/4      : (32,64) (64,128) (128,256)  SRC_BNRELU / EPI_FWD
//   backward-data of dec.deconv3/2: (32,64) (64,128)            SRC_BNBWD  / EPI_MASK
//   backward-data of dec.deconv1  : (128,256)                   SRC_BNBWD  / EPI_PLAIN
int eae_launch_conv_s2(const ConvArgs& a, int cin, int cout, int src, int epi, hipStream_t st) {
  if (a.B <= 0 || (a.Hin & 1) || (a.Win & 1)) return eae_set_error(-2, "conv_s2: bad shape");
  S2Plan p;
  plan_here(p, KIND_CONV, cin, cout, epi, a.qs != nullptr, a.B, a.Hin, a.Win);      // (no geometry: conv_geo reports it)
#define CASE(CI, CO, S, E) if (cin == CI && cout == CO && src == S && epi == E) return conv_geo<CI, CO, 64, S, E>(a, p, st)
  CASE(32, 64, SRC_BNRELU, EPI_FWD);
  CASE(64, 128, SRC_BNRELU, EPI_FWD);
  CASE(128, 256, SRC_BNRELU, EPI_FWD);
  CASE(32, 64, SRC_BNBWD, EPI_MASK);
  CASE(64, 128, SRC_BNBWD, EPI_MASK);
  CASE(128, 256, SRC_BNBWD, EPI_PLAIN);
  CASE(32, 64, SRC_RAW, EPI_FWD);          // plain conv (tests / generic use)
#undef CASE
  return eae_set_error(-2, "conv_s2: no kernel instantiated for this (cin, cout, src, epilogue)");
}

// deconv-kind instantiations used by the path:
//   forward of dec.deconv1/2/3      : (256,128) SRC_RAW, (128,64) (64,32) SRC_BNRELU / EPI_FWD
//   backward-data of enc.conv4/3/2  : (256,128) (128,64) (64,32)  SRC_BNBWD / EPI_MASK
int eae_launch_deconv_s2(const ConvArgs& a, int cin, int cout, int src, int epi, hipStream_t st) {
  if (a.B <= 0) return eae_set_error(-2, "deconv_s2: bad shape");
  S2Plan p;
  plan_here(p, KIND_DECONV, cin, cout, epi, a.qs != nullptr, a.B, a.Hin, a.Win);    // (no geometry: deconv_geo reports it)
#define CASE(CI, CO, BN_, S, E) if (cin == CI && cout == CO && p.bn == BN_ && src == S && epi == E) return deconv_geo<CI, CO, BN_, S, E>(a, p, st)
  CASE(256, 128, 64, SRC_RAW, EPI_FWD);       CASE(256, 128, 32, SRC_RAW, EPI_FWD);        // (32-channel blocks: the plan's small grids)
  CASE(128, 64, 64, SRC_BNRELU, EPI_FWD);     CASE(128, 64, 32, SRC_BNRELU, EPI_FWD);
  CASE(64, 32, 32, SRC_BNRELU, EPI_FWD);
  CASE(256, 128, 64, SRC_BNBWD, EPI_MASK);    CASE(256, 128, 32, SRC_BNBWD, EPI_MASK);
  CASE(128, 64, 64, SRC_BNBWD, EPI_MASK);     CASE(128, 64, 32, SRC_BNBWD, EPI_MASK);
  CASE(64, 32, 32, SRC_BNBWD, EPI_MASK);
  CASE(64, 32, 32, SRC_RAW, EPI_FWD);          // plain deconv (tests / generic use)
#undef CASE
  return eae_set_error(-2, "deconv_s2: no kernel instantiated for this (cin, cout, src, epilogue)");
}

// number of per-workgroup statistics partials of that launch: the plan's.  -1: no geometry for this map.  (The count depends on
// neither the epilogue nor fp8.)
int eae_conv_s2_ntiles(int kind, int cin, int cout, int B, int Hin, int Win) {
  S2Plan p;
  plan_here(p, kind, cin, cout, EPI_FWD, false, B, Hin, Win);
  return p.ntiles;
}
