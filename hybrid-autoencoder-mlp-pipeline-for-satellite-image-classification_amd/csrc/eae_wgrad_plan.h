// The slice plan of one weight-gradient launch: tile geometry, tile count, how many workgroups share the tiles, how many tiles each
// takes, the grid and the floats of split-K partials it writes -- for the generic 3x3 stride-2 kernel (eae_wgrad_launch.hip) and for
// the C-band edge kernel (eae_edge_launch.hip) -- and the K range of a latent-projection slice.  Decided HERE and nowhere else: the
// launch units parse their environment switches once per process and hand them in, then execute the plan; eae_ctx.hip sizes the
// buffers from the constants below.  Plain host code, nothing from HIP and nothing read from the environment, so that a sanitised
// CPU program (tests/wgrad_plan_check.cpp) can sweep it: a wrong slice count is a kernel writing partials past its scratch.
#pragma once

// ---- 3x3 stride-2 weight gradient (wgrad_s2_kernel): dw [cs][cb][3][3] in blocks of 64 x 32 x 9
enum { WG_OK = 0, WG_NO_GEOMETRY, WG_SCRATCH, WG_FP8_NARROW };     // WgS2Plan::refused, in the order the checks are made
struct WgS2Plan {
  int tw, th, ni;            // tile width x height in positions of the small map, images per tile
  int ntiles;
  int slices;                // position slices: workgroups per output block, each with a partial of the whole dw
  int tiles_per_block;       // consecutive tiles of a slice; (slices - 1) * tiles_per_block < ntiles <= slices * tiles_per_block
  int nblk;                  // 64 x 32 output blocks
  unsigned grid;             // slices * nblk workgroups
  long long scratch_used;    // floats of partials written at the head of the scratch: slices * cs * cb * 9, 0 when writes_dw
  bool writes_dw;            // one slice: its "partial" is the result (same layout), no reduction launch
  int refused;               // WG_*: why the function returned false
};

// Fills `p` for a (cs, cb) layer on B small maps of Hs x Ws; false (p.refused says why) for a map with no geometry -- the map must
// be 4x4, 8x8 or a multiple of 8 rows x 16 columns --, for a scratch that cannot hold even one slice when more than one is needed,
// and for the fp8 variant (built for the 16 x 8 tiles only) on a narrow map.
//
// 12-wave workgroups (4 consumer + 8 producer waves), one per CU.  Every workgroup writes a partial of its 64 x 32 x 9 block, so
// their number also sets the split-K traffic and the work of the reduction behind the kernel.  Inside the train step these
// kernels run beside the backward-data chain, and what counts is how many CUs they take from it: 64 workgroups measured best for
// every layer (ms per step at B=512 / B=64: 32: 0.599 / 0.241, 48: 0.540, 64: 0.500-0.512 / 0.244, 80: 0.515, 128: 0.509-0.527 /
// 0.271, 256: 0.542).  wgs_one / wgs_wide: the budget of the one-block layer (64 x 32) and of the wider ones; wgs_last: of the
// last weight gradient of the step (`last`: enc.conv2's, which runs in the tail, beside conv2's backward-data and conv1's weight
// gradient only).  EAE_WGRAD_WGS=<one>[,<wide>[,<last>]] sets them.  mult: members of a grouped step (eae_geo_mult) -- the grid
// sizes are per launch, so a member takes its share of the budget, but no fewer than 8 workgroups.
inline bool eae_wgrad_s2_plan(WgS2Plan& p, int cs, int cb, bool last, bool fp8, int B, int Hs, int Ws, long long scratch_floats,
                              int wgs_one, int wgs_wide, int wgs_last, int mult) {
  p = WgS2Plan();
  p.nblk = (cs / 64) * (cb / 32);
  if (Ws % 16 == 0 && Hs % 8 == 0) { p.tw = 16; p.th = 8; p.ni = 1; }
  else if (Ws == 8 && Hs == 8) { p.tw = 8; p.th = 8; p.ni = 2; }
  else if (Ws == 4 && Hs == 4) { p.tw = 4; p.th = 4; p.ni = 8; }
  else { p.refused = WG_NO_GEOMETRY; return false; }
  p.ntiles = (B + p.ni - 1) / p.ni * (Hs / p.th) * (Ws / p.tw);
  const long long sz = (long long)cs * cb * 9;
  int wgs = last ? wgs_last : (p.nblk == 1 ? wgs_one : wgs_wide);
  if (mult > 1) wgs = wgs / mult > 8 ? wgs / mult : 8;
  int slices = wgs / p.nblk;
  if (slices < 1) slices = 1;
  if (slices > p.ntiles) slices = p.ntiles;
  while ((long long)slices * sz > scratch_floats && slices > 1) slices >>= 1;
  if ((long long)slices * sz > scratch_floats) { p.refused = WG_SCRATCH; return false; }
  p.tiles_per_block = (p.ntiles + slices - 1) / slices;
  p.slices = (p.ntiles + p.tiles_per_block - 1) / p.tiles_per_block;      // the slices that are left with a tile
  p.writes_dw = p.slices == 1;
  p.scratch_used = p.writes_dw ? 0 : p.slices * sz;
  p.grid = (unsigned)(p.slices * p.nblk);
  if (fp8 && p.tw != 16) { p.refused = WG_FP8_NARROW; return false; }
  return true;
}

// ---- C-band edge weight gradient (edge_wgrad_kernel): dw [32][C][3][3], one partial of 288 * C floats per workgroup
constexpr int EDGE_TILE_ROWS = 8, EDGE_TILE_COLS = 64;     // image pixels under one tile of 4 x 32 positions (E_TH, E_TW: eae_edge.hip.h)
// conv1's weight gradient has a scratch of its own (it runs on the caller's stream while the side streams still use theirs)
constexpr int EAE_EDGE_WGRAD_SCRATCH_SLICES = 2048;
inline long long eae_edge_wgrad_slice_floats(int C) { return 32LL * 9 * C; }

struct EdgeWgPlan {
  int ntiles;
  int blocks;                // workgroups = partials
  int tiles_per_block;       // (blocks - 1) * tiles_per_block < ntiles <= blocks * tiles_per_block
  long long scratch_used;    // blocks * 288 * C floats at the head of the scratch
};

// Fills `p` for C bands on B images of H x W (multiples of 8 x 64); false when the scratch cannot hold one partial.
//
// Workgroups: each writes a partial, so their number also sets the reduction behind the kernel.  Round 4 re-sweep at B=512 (ms per
// step, main / side cap): 1024 / 1024 0.4875-0.4891, 512 / 1024 0.4832, 512 / 512 0.4821, 512 / 256 0.4794-0.4795, 768 / 256 0.4788,
// 512 / 128 0.4836, 640 / 192 0.4887, 256 main 0.4930.  cap_main (512, EAE_EDGE_WGRAD_BLOCKS): the fp32 image as source; cap_side
// (256, EAE_EDGE_WGRAD_SIDE_BLOCKS; `side_source`): the NHWC source -- a launch beside the backward-data chain (deconv4's weight
// gradient, side stream) takes fewer CUs from it with fewer blocks.  mult: members of a grouped step -- the caps are per launch,
// so a member takes its share, but no fewer than 32 workgroups.
inline bool eae_edge_wgrad_plan(EdgeWgPlan& p, bool side_source, int C, int B, int H, int W, long long scratch_floats, int cap_main,
                                int cap_side, int mult) {
  p = EdgeWgPlan();
  const long long slice = eae_edge_wgrad_slice_floats(C);
  p.ntiles = B * (H / EDGE_TILE_ROWS) * (W / EDGE_TILE_COLS);
  int lim = side_source ? cap_side : cap_main;
  if (mult > 1) lim = lim / mult > 32 ? lim / mult : 32;
  int nblocks = p.ntiles < lim ? p.ntiles : lim;
  while (nblocks * slice > scratch_floats && nblocks > 1) nblocks /= 2;
  p.tiles_per_block = (p.ntiles + nblocks - 1) / nblocks;
  p.blocks = (p.ntiles + p.tiles_per_block - 1) / p.tiles_per_block;      // the workgroups that are left with a tile
  p.scratch_used = p.blocks * slice;
  return p.scratch_used <= scratch_floats;
}

// ---- split-K of the latent projections: K range per slice.  EAE_FC_KLEN_MIN (32 slices) at the reference's 64x64 inputs; wider
// inputs keep the number of slices at `slices_setting` (EAE_FC_SLICES, default 64): K / 128 = 512 slices at 256x256 wrote and re-read
// 67 MB of partials per projection (ms per config-5 step with 512 / 128 / 64 / 32 / 16 slices: 2.066 / 2.050 / 2.040 / 2.058 / 2.107,
// with the prefetching K loop of fc_nt_kernel).  The partials buffer is sized for the most slices there can be, K / EAE_FC_KLEN_MIN.
constexpr int EAE_FC_KLEN_MIN = 128;
inline int eae_fc_klen(long long K, int slices_setting) {
  long long klen = EAE_FC_KLEN_MIN;
  while (K / klen > slices_setting && K % (klen * 2) == 0) klen *= 2;
  return (int)klen;
}
