// Stand-alone sweep of csrc/eae_wgrad_plan.h (compiled under the address and undefined-behaviour sanitisers and run by
// test_wgrad_plan.py).  Prints one line per case -- the plan's arguments, a colon, what the plan decided -- which the test compares
// with the Python restatements (conv_ref.expected_wgrad_launch, edge_ref.expected_edge_wgrad_launch); checks on every case, and on
// extreme arguments that are not printed, that every tile is covered once and that the partials fit the scratch.  Returns the number
// of violations.
#include "eae_wgrad_plan.h"
#include <cstdio>
#include <initializer_list>

static long long cases = 0, bad = 0;
static void fail(const char* what, const char* rule) { std::printf("VIOLATION %s: %s\n", what, rule); ++bad; }
#define REQUIRE(what, cond) do { if (!(cond)) fail(what, #cond); } while (0)

static const long long SIDE_SCRATCH = 6LL * 1024 * 1024;      // eae_ctx::wscratch_floats, the engine's scratch of every side stream

// (cs, cb, small mode, big mode): the 13 instantiations of eae_launch_wgrad_s2; modes 2 and 4 carry the gradient (SRC_BNBWD, SRC_RAWG)
static const int INST[13][4] = {{64, 32, 2, 1}, {128, 64, 2, 1}, {256, 128, 2, 1}, {64, 32, 1, 2}, {128, 64, 1, 2}, {256, 128, 0, 2},
                                {64, 32, 0, 0}, {64, 32, 4, 1}, {128, 64, 4, 1}, {256, 128, 4, 1}, {64, 32, 1, 4}, {128, 64, 1, 4},
                                {256, 128, 0, 4}};
// small maps (rows, columns); the last two have no geometry
static const int MAPS[11][2] = {{4, 4}, {8, 8}, {16, 16}, {8, 16}, {16, 32}, {8, 32}, {24, 16}, {32, 32}, {64, 64}, {16, 8}, {6, 6}};
static const int BANDS[7] = {1, 3, 5, 8, 9, 13, 16};
static const int IMAGES[7][2] = {{8, 64}, {16, 64}, {24, 64}, {64, 64}, {16, 128}, {24, 192}, {256, 256}};
static const int MULTS[4] = {1, 2, 8, 64};

static void s2(const int* in, int hs, int ws, int B, long long scratch, int one, int wide, int last_wgs, int mult, bool fp8, bool print) {
  const int cs = in[0], cb = in[1];
  const bool last = cs == 64 && (in[2] == 2 || in[2] == 4);
  WgS2Plan p;
  const bool ok = eae_wgrad_s2_plan(p, cs, cb, last, fp8, B, hs, ws, scratch, one, wide, last_wgs, mult);
  ++cases;
  if (print)
    std::printf("s2 %d %d %d %d %d %d %d %lld %d %d %d %d %d : %d %d %d %d %d %d %d %d %u %lld %d\n", cs, cb, in[2], in[3], hs, ws, B, scratch,
                one, wide, last_wgs, mult, (int)fp8, p.refused, p.tw, p.th, p.ni, p.ntiles, p.slices, p.tiles_per_block, p.nblk, p.grid,
                p.scratch_used, (int)p.writes_dw);
  REQUIRE("s2", ok == (p.refused == WG_OK));
  if (p.refused == WG_NO_GEOMETRY || p.refused == WG_SCRATCH) return;
  // (the fp8 refusal comes last: the plan of the bf16 kernel on the same map is complete)
  const long long sz = (long long)cs * cb * 9;
  REQUIRE("s2", p.slices >= 1 && p.tiles_per_block >= 1 && p.nblk == (cs / 64) * (cb / 32));
  REQUIRE("s2", p.ntiles == (B + p.ni - 1) / p.ni * (hs / p.th) * (ws / p.tw));
  REQUIRE("s2", (long long)(p.slices - 1) * p.tiles_per_block < p.ntiles && p.ntiles <= (long long)p.slices * p.tiles_per_block);
  REQUIRE("s2", p.slices * sz <= scratch);
  REQUIRE("s2", (long long)p.grid == (long long)p.slices * p.nblk);
  REQUIRE("s2", p.writes_dw == (p.slices == 1) && p.scratch_used == (p.writes_dw ? 0 : p.slices * sz));
}

static void edge(int kind, int C, int H, int W, int B, long long scratch, int cap_main, int cap_side, int mult, const char* print) {
  EdgeWgPlan p;
  const bool ok = eae_edge_wgrad_plan(p, kind == 1, C, B, H, W, scratch, cap_main, cap_side, mult);
  ++cases;
  if (print)
    std::printf("%s %d %d %d %d %d %lld %d %d %d : %d %d %d %d %lld\n", print, kind, C, H, W, B, scratch, cap_main, cap_side, mult, (int)ok,
                p.ntiles, p.blocks, p.tiles_per_block, p.scratch_used);
  REQUIRE("edge", p.ntiles == B * (H / 8) * (W / 64) && p.blocks >= 1 && p.tiles_per_block >= 1);
  REQUIRE("edge", (long long)(p.blocks - 1) * p.tiles_per_block < p.ntiles && p.ntiles <= (long long)p.blocks * p.tiles_per_block);
  REQUIRE("edge", p.scratch_used == p.blocks * 288LL * C && ok == (p.scratch_used <= scratch));
}

int main() {
  const int wgs[4][3] = {{64, 64, 64}, {16, 16, 16}, {256, 256, 256}, {48, 96, 24}};      // the last: each budget reaches its layers
  const int caps[2][2] = {{512, 256}, {64, 32}};
  // Every row x map x batch 1..600: under the default settings on the four scratch sizes and as the fp8 variant; under every other
  // (budget, members) pair on the default scratch (the maps without geometry are refused before a setting is looked at).
  for (const auto& in : INST) for (int mi = 0; mi < 11; ++mi) {
    const int* m = MAPS[mi];
    const long long sz = (long long)in[0] * in[1] * 9, scr[4] = {SIDE_SCRATCH, 3 * sz, sz, sz - 1};
    for (long long sf : scr) for (int B = 1; B <= 600; ++B) s2(in, m[0], m[1], B, sf, 64, 64, 64, 1, false, true);
    for (int B = 1; B <= 600; ++B) s2(in, m[0], m[1], B, SIDE_SCRATCH, 64, 64, 64, 1, true, true);
    for (int wi = 0; wi < 4 && mi < 9; ++wi) for (int mult : MULTS) {
      if ((wi == 0 && mult == 1) || (wi == 3 && mult > 1)) continue;      // the default pair ran above; the mixed triple runs alone
      for (int B = 1; B <= 600; ++B) s2(in, m[0], m[1], B, SIDE_SCRATCH, wgs[wi][0], wgs[wi][1], wgs[wi][2], mult, false, true);
    }
  }
  for (int kind = 0; kind < 2; ++kind) for (int C : BANDS) for (const auto& im : IMAGES) {
    const long long sl = eae_edge_wgrad_slice_floats(C);
    const long long scr[4] = {kind == 1 ? SIDE_SCRATCH : EAE_EDGE_WGRAD_SCRATCH_SLICES * sl, 3 * sl, sl, sl - 1};
    for (long long sf : scr) for (int B = 1; B <= 600; ++B) edge(kind, C, im[0], im[1], B, sf, 512, 256, 1, "edge");
    for (const auto& cp : caps) for (int mult : MULTS) {
      if (cp[0] == 512 && mult == 1) continue;
      for (int B = 1; B <= 600; ++B) edge(kind, C, im[0], im[1], B, scr[0], cp[0], cp[1], mult, "edge");
    }
  }
  // the multi-tile rows of the GPU tests (edge_ref.EDGE_WGRAD_MULTI_TILE) with the scratch those tests give them
  const long long rows[5][6] = {{0, 3, 8, 64, 520, 2 << 20}, {1, 3, 8, 64, 520, 2 << 20}, {0, 5, 16, 64, 5, 4 * 288 * 5}, {1, 8, 16, 64, 5, 4 * 288 * 8},
                                {0, 16, 24, 64, 3, 2 * 288 * 16}};
  for (const auto& r : rows) edge((int)r[0], (int)r[1], (int)r[2], (int)r[3], (int)r[4], r[5], 512, 256, 1, "edge_row");
  for (int setting : {1, 16, 64, 512, 1 << 20}) for (int pn = 1; pn <= 1024; ++pn) {
    const long long K = 256LL * pn;
    const int klen = eae_fc_klen(K, setting);
    ++cases;
    std::printf("fc %lld %d : %d\n", K, setting, klen);
    REQUIRE("fc", klen >= EAE_FC_KLEN_MIN && K % klen == 0 && K / klen <= K / EAE_FC_KLEN_MIN);
  }
  // extreme arguments: only the invariants and a clean sanitiser run are asked of them
  const long long big_scr[4] = {0, 1, 1LL << 40, SIDE_SCRATCH};
  for (const auto& in : INST) for (const auto& m : MAPS) for (int B : {1, 599, 1 << 20}) for (long long sf : big_scr)
    for (int w : {1, 64, 1 << 20}) for (int mult : {1, 64}) for (int fp8 = 0; fp8 < 2; ++fp8) s2(in, m[0], m[1], B, sf, w, w, w, mult, fp8 != 0, false);
  for (int kind = 0; kind < 2; ++kind) for (int C : BANDS) for (const auto& im : IMAGES) for (int B : {1, 599, 1 << 20}) for (long long sf : big_scr)
    for (int cap : {1, 512, 1 << 20}) for (int mult : {1, 64}) edge(kind, C, im[0], im[1], B, sf, cap, cap, mult, nullptr);
  std::printf("%lld cases, %lld violations\n", cases, bad);
  return bad ? 1 : 0;
}
