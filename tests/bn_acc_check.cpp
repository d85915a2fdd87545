// Stand-alone sweep of csrc/eae_bn_acc.h, the fixed-point arithmetic of the folded BatchNorm finalize (compiled under the address
// and undefined-behaviour sanitisers, without fused multiply-adds, and run by test_bn_acc_reference.py).  One line per case: the
// case, a colon, the two accumulator words as the atomics leave them (sums modulo 2^64), the flag, and the finished values as fp32
// bit patterns.  The test compares every line with tests/bn_acc_ref.py.  The program itself checks that no total of contributions
// that passed the limit leaves the signed 64-bit range, on every case and on the worst case of every launch size.  Returns the
// number of violations.
#include "eae_bn_acc.h"
#include <cstdint>
#include <cstdio>
#include <cstring>

static long long cases = 0, bad = 0;
static void fail(const char* what, const char* rule) { std::printf("VIOLATION %s: %s\n", what, rule); ++bad; }
#define REQUIRE(what, cond) do { if (!(cond)) fail(what, #cond); } while (0)

static const int COUNTS[7] = {1, 2, 3, 16, 1000, 4096, 32768};     // workgroups per channel (3 and 1000: limits that are no powers of two)
static const int WORLDS[3] = {1, 2, 8};
static const int E_LO = -60, E_HI = 70;

static uint32_t bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

// contribution i of accumulator `which` in sign mode g (0: all positive, 1: all negative, 2: mixed), launch (ni, wi): 2^e * [1, 2)
static uint32_t hash(uint32_t seed, uint32_t i) {
  uint32_t h = (i * 2654435761u) ^ (seed * 40503u + 0x9e3779b9u);
  h ^= h >> 15; h *= 2246822519u; h ^= h >> 13;
  return h;
}
static float contribution(uint32_t seed, uint32_t i, int e, int g) {
  const uint32_t h = hash(seed, i);
  const float m = 1.0f + (float)(h >> 9) * 1.1920928955078125e-07f;      // 23 random mantissa bits
  const bool neg = g == 1 || (g == 2 && ((h >> 8) & 1u));
  return ldexpf(neg ? -m : m, e);
}

static void one_case(int s, int e, int g, int ni, int wi) {
  const float scale = s ? BN_ACC_SCALE_BWD : BN_ACC_SCALE_FWD;
  const int n = COUNTS[ni], w = WORLDS[wi];
  const long long N = (long long)n * w;
  const float lim = bn_acc_limit(n, w);
  unsigned long long word[2] = {0, 0};
  __int128 exact[2] = {0, 0};
  bool flag = false;
  for (int which = 0; which < 2; ++which) {
    const uint32_t seed = (uint32_t)(((g * 7 + ni) * 3 + wi) * 2 + which);
    for (long long i = 0; i < N; ++i) {
      const float sv = contribution(seed, (uint32_t)i, e, g) * scale;
      if (bn_acc_fits(sv, lim)) { const unsigned long long q = bn_acc_fixed(sv); word[which] += q; exact[which] += (long long)q; }
      else flag = true;
    }
    // what passed the limit cannot wrap: the signed read of the word is the exact sum
    REQUIRE("total", exact[which] == (__int128)(long long)word[which]);
  }
  ++cases;
  const float count = (float)(N * 128);
  std::printf("%d %d %d %d %d : %08x %llu %llu %d", s, e, g, n, w, bits(lim), word[0], word[1], (int)flag);
  if (s == 0) {
    const BnAccFwd o = bn_acc_fwd_finish((long long)word[0], (long long)word[1], flag, 1.0f / scale, count, 1e-5f, 1.25f, -0.5f);
    float rm = 0.25f, rv = 1.5f;
    bn_acc_running(o, count, 0.1f, rm, rv);
    std::printf(" %08x %08x %08x %08x %08x %08x\n", bits(o.s), bits(o.t), bits(o.mean), bits(o.invstd), bits(rm), bits(rv));
  } else {
    const BnAccBwd o = bn_acc_bwd_finish((long long)word[0], (long long)word[1], flag, 1.0f / scale, count, 1.25f, 0.375f, 0.8125f);
    std::printf(" %08x %08x %08x %08x %08x\n", bits(o.A), bits(o.Bc), bits(o.Cc), bits(o.dgamma), bits(o.dbeta));
  }
}

// the largest contribution that passes, N times over with one sign: the worst a launch of that size can do
static void worst(long long n, int w, bool print) {
  const float lim = bn_acc_limit(n, w);
  const float top = nextafterf(lim, 0.f);
  ++cases;
  REQUIRE("worst", bn_acc_fits(top, lim) && !bn_acc_fits(lim, lim) && bn_acc_fits(-top, lim) && !bn_acc_fits(-lim, lim));
  REQUIRE("worst", !bn_acc_fits(__builtin_nanf(""), lim) && !bn_acc_fits(__builtin_inff(), lim) && !bn_acc_fits(-__builtin_inff(), lim));
  const long long q = (long long)bn_acc_fixed(top), qn = (long long)bn_acc_fixed(-top);
  const __int128 total = (__int128)q * n * w, two63 = (__int128)1 << 63;
  REQUIRE("worst", qn == -q && total < two63 && -total > -two63);
  if (print) std::printf("worst %lld %d : %08x %lld\n", n, w, bits(lim), q);
}

int main() {
  for (int s = 0; s < 2; ++s)
    for (int e = E_LO; e <= E_HI; ++e)
      for (int g = 0; g < 3; ++g)
        for (int ni = 0; ni < 7; ++ni)
          for (int wi = 0; wi < 3; ++wi) {
            if (g == 2 && COUNTS[ni] > 1000) continue;      // mixed signs: the small launches (the sums cancel, nothing new at size)
            one_case(s, e, g, ni, wi);
          }
  for (int ni = 0; ni < 7; ++ni)
    for (int wi = 0; wi < 3; ++wi) worst(COUNTS[ni], WORLDS[wi], true);
  // every launch size up to 2^16 workgroups per channel and worlds up to 64, powers of two or not; then sizes no engine reaches
  for (long long n = 1; n <= 65536; n += (n < 4200 ? 1 : 97))
    for (int w = 1; w <= 64; w = w * 2 + (w == 4)) worst(n, w, false);       // 1, 2, 4, 9, 18, 36
  for (int sh = 17; sh <= 36; ++sh) { worst(1LL << sh, 1, false); worst((1LL << sh) - 1, 3, false); }
  std::printf("%lld cases, %lld violations\n", cases, bad);
  return bad ? 1 : 0;
}
