// The tile plan of one 3x3 stride-2 conv / transposed-conv launch: which kernel, which tile geometry, how many channel blocks, the
// grid, and the number of per-workgroup statistics partials it writes.  Decided HERE and nowhere else: eae_conv_launch.hip executes
// the plan, eae_conv_s2_ntiles() reports its `ntiles` to whoever sizes or reads the partials.  Plain host code, nothing from HIP.
#pragma once

enum { S2_CONV = 0, S2_DECONV = 1 };                            // = KIND_CONV / KIND_DECONV (eae_args.h)
enum { S2_ONE_ROLE = 0, S2_WAVE_SPEC = 1, S2_FP8 = 2 };         // igemm_s2_kernel, igemm2_s2_kernel, igemm8_s2_kernel
enum { S2_GEO_NONE = -1, S2_GEO_16x8x1, S2_GEO_8x8x2, S2_GEO_8x8x1, S2_GEO_4x4x8, S2_GEO_4x4x4, S2_GEO_COUNT };
// tile width x height in positions (conv: of the output map; transposed: of the input map), images per tile
struct S2Geo { int tw, th, ni; };
constexpr S2Geo S2_GEOS[S2_GEO_COUNT] = {{16, 8, 1}, {8, 8, 2}, {8, 8, 1}, {4, 4, 8}, {4, 4, 4}};

struct S2Plan {
  int kern;          // S2_ONE_ROLE / S2_WAVE_SPEC / S2_FP8
  int geo;           // S2_GEO_*, S2_GEO_NONE: no geometry for this map (then ntiles = -1 and nothing may be launched)
  int bn;            // output channels per channel block
  int nbl;           // channel blocks a workgroup loops over (wave-specialised kernel, two-chunk layers), else 1
  int ntiles;        // tiles = statistics partials per channel ([2][cout][ntiles])
  unsigned grid;     // workgroups (1-D: the kernels map ids to (tile, channel block) XCD-aware)
  unsigned threads;  // per workgroup
};

// Small-tile geometries for the 8x8 / 4x4 maps: 64-position tiles for the conv kind, 32-channel blocks for the transposed kind --
// twice the workgroups, each with half the work.  They pay when the 128-position grid leaves most of the 256 CUs empty (ms per step,
// small vs large: B=64 0.255 vs 0.280, B=128 0.288 vs 0.310, B=256 0.369 vs 0.371) and lose at B=512, so a layer takes them when its
// large-tile grid has fewer than 256 workgroups.  ig_small >= 0 (EAE_IG_SMALL=<mask>) overrides (bit 0: conv kind, bit 1: transposed
// kind).  mult: members of a grouped step (eae_geo_mult) -- K contexts' launches run as one, so the grid that decides is K times the
// member's.
inline bool s2_small(int kind, int B, int Wpos, int cout, int mult, int ig_small) {
  if (ig_small >= 0) return (ig_small & (kind == S2_CONV ? 1 : 2)) != 0;
  B *= mult;
  const int nt = (kind == S2_CONV) ? ((Wpos == 8) ? (B + 1) / 2 : (B + 7) / 8) : ((Wpos == 8) ? B : (B + 3) / 4);
  return nt * (cout / 64) < 256;
}

// Wave-specialised kernel (eae_igemm2.hip.h) for the multi-chunk layers on the small maps.  Inside the training step (rocprofv3,
// B=512, us, igemm2 vs one-role kernel): conv 128->256 forward 16.7 vs 18.3 and deconv 256->128 forward 16.5 vs 18.2 win; conv
// 64->128 forward 18.5 vs 16.8, deconv 128->64 forward 22.6 vs 19.6, and every backward-data use (31.3 vs 26.2, 48.8 vs 33.6: a
// 512-thread workgroup owns the whole CU and collides with the weight-gradient kernels beside it) lose.  So: igemm2_mode
// (EAE_IGEMM2) 1 = the two winning forward layers only, 2 = every layer it is instantiated for (conv from 64 input channels,
// transposed from 128), 0 = one-role kernel everywhere.
inline bool s2_igemm2_on(int kind, int cin, int epi, int igemm2_mode) {
  if (kind == S2_CONV ? cin < 64 : cin < 128) return false;
  const bool wins = (epi == 0 /* EPI_FWD */) && ((kind == S2_CONV && cin == 128) || (kind == S2_DECONV && cin == 256));
  return igemm2_mode >= 2 || (igemm2_mode == 1 && wins);
}

// Fills `p` for a (kind, cin, cout, epilogue) layer on B maps of Hin x Win; false (geo = S2_GEO_NONE, ntiles = -1) when the map
// has no geometry: the position grid must be 4x4, 8x8 or a multiple of 8 rows x 16 columns, and the fp8 variant has 16-wide tiles
// only.  `bn` is set either way.  The geometry, and with it ntiles, depends on neither the epilogue nor fp8.
inline bool eae_s2_plan(S2Plan& p, int kind, int cin, int cout, int epi, bool fp8, int B, int Hin, int Win, int mult,
                        int igemm2_mode, int ig_small) {
  const int Hp = (kind == S2_CONV) ? Hin / 2 : Hin, Wp = (kind == S2_CONV) ? Win / 2 : Win;   // the position grid
  const bool wide = Wp % 16 == 0 && Hp % 8 == 0, narrow = !wide && Hp == Wp && (Wp == 8 || Wp == 4);
  // the conv kind halves its tiles from 64 input channels on; the transposed kind halves its channel blocks from 64 output channels on
  const bool small = narrow && (kind == S2_CONV ? cin >= 64 : cout >= 64) && s2_small(kind, B, Wp, cout, mult, ig_small);
  p.bn = (kind == S2_DECONV && (cout == 32 || small)) ? 32 : 64;
  p.kern = S2_ONE_ROLE; p.nbl = 1; p.threads = 256; p.geo = S2_GEO_NONE; p.ntiles = -1; p.grid = 0;
  if (wide) {
    p.geo = S2_GEO_16x8x1;
    if (fp8) p.kern = S2_FP8;
  } else if (narrow && !fp8) {
    if (kind == S2_CONV) p.geo = (Wp == 8) ? (small ? S2_GEO_8x8x1 : S2_GEO_8x8x2) : (small ? S2_GEO_4x4x4 : S2_GEO_4x4x8);
    else p.geo = (Wp == 8) ? S2_GEO_8x8x1 : S2_GEO_4x4x4;
    // the conv kind's small tiles exist for the one-role kernel only; the transposed kind's 32-channel blocks for both
    if (s2_igemm2_on(kind, cin, epi, igemm2_mode) && !(kind == S2_CONV && small)) {
      p.kern = S2_WAVE_SPEC; p.threads = 512;
      if (kind == S2_CONV && cin == 64) p.nbl = cout / p.bn;     // two chunks: both stay resident, the workgroup loops over the channel blocks
    }
  } else {
    return false;
  }
  const S2Geo g = S2_GEOS[p.geo];
  p.ntiles = (B + g.ni - 1) / g.ni * (Hp / g.th) * (Wp / g.tw);
  p.grid = (unsigned)(p.ntiles * (p.nbl > 1 ? 1 : cout / p.bn));
  return true;
}
