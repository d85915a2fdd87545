// Co-registration of two scenes (include/eae.h, "co-registration"): the correlation sums of a grid of tie-point
// tiles, and the resampling of a planar [C][H][W] scene of uint8 / uint16 / float32 through a 2 x 3 affine map.
//   match:    one workgroup a tile at a time (grid-stride over the tiles).  It stages the template of A ([T][TW] words, TW = T rounded
//             up to 4) and the search window of B ([T + 2R][BW] words) in LDS once: a thread takes consecutive pixels of one row
//             (coalesced), decides the pixel's validity over all bands of its scene and converts the matched band to the 16-bit
//             feature; a word is feature | valid << 16, an invalid or padding word 0.  A work item is (row slice s, dy, g): it owns the
//             four adjacent offsets dx = 4 g .. 4 g + 3 of one dy and walks the template rows of its slice four columns at a time: one
//             128-bit read of A (the same address in every lane of a (dy, g) round: a broadcast) and two of B give 4 x 4 pairs, so a
//             window word is read from LDS once per four offsets instead of once per offset.  Lane q = dy G + g of a round reads B at
//             word (dy + i) BW + 4 g + j; BW is chosen = 4 G (mod 64), which puts lane q on words 4 q .. 4 q + 3 (mod 64): the sixteen
//             lanes of every ds_read_b128 group fall on 64 different banks.  With both words' features zeroed where the pixel is
//             invalid, the six sums need no branch: n += va & vb, sum a += vb ? a : 0 (32-bit: at most 4096 x 65535 < 2^28), and the
//             three second-order sums are one 32 x 32 + 64-bit multiply-add each (products below 2^32, sums below 2^44).  When a tile
//             has fewer than 129 (dy, g) pairs the template rows are cut into S slices so that the workgroup stays busy, and the
//             slices meet in a 64-bit LDS table (integer adds: any order gives the same words); otherwise an item writes its four
//             offsets straight to the output.  Integers only: the table does not depend on the launch geometry.
//   resample: a workgroup is 64 x 4 destination pixels, a thread one pixel with all its bands: coordinates, weights and the validity
//             of the taps are computed once.  Every operation is one correctly rounded float64 product or sum that nothing may contract,
//             in the order the header states, so that the NumPy restatement reproduces every bit.
#include "eae_internal.h"
#include "eae_common.hip.h"

namespace {

typedef unsigned long long u64;
typedef __attribute__((address_space(3))) u64 lds_u64;

constexpr int RG_MAX_C = 16;
constexpr int MT_NT = 256;                  // threads of a matching workgroup
constexpr int MT_GRID = 1024;               // most workgroups of a matching launch: more tiles go round the grid-stride loop
constexpr int MT_MIN_T = 4, MT_MAX_T = 64, MT_MAX_R = 16, MT_MAX_TILES = 1 << 20;
constexpr int MT_K = 4;                     // adjacent dx of a work item: one 128-bit LDS read

__device__ __forceinline__ void wg_barrier() {          // (builtins: see eae_slic.hip)
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}
__device__ __forceinline__ void lds_add64(u64* p, u64 v) {
  __hip_atomic_fetch_add((lds_u64*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

struct RegScene {
  const void* data; const unsigned char* mask; int C, H, W, mode, rule; float nd;
};

template <typename T> __device__ __forceinline__ bool nd_match(T v, int mode, T ref, float fref) {
  if (mode == EAE_NODATA_NONE) return false;
  if constexpr (sizeof(T) == 4) return mode == EAE_NODATA_NAN ? v != v : v == fref;
  else return v == ref;
}

// Whether pixel (y, x) of the scene is valid, as eae_change_moments decides it: inside the raster, its mask byte clear, its nodata rule
// silent over all C bands and, for float32, every band finite.  An integer scene without nodata reads no band.
template <typename T> __device__ __forceinline__ bool pixel_valid(const RegScene& s, long long y, long long x) {
  if (y < 0 || y >= s.H || x < 0 || x >= s.W) return false;
  const long long plane = (long long)s.H * s.W, px = y * s.W + x;
  if (s.mask && s.mask[px]) return false;
  if (sizeof(T) < 4 && s.mode == EAE_NODATA_NONE) return true;
  const T* p = (const T*)s.data + px;
  const T ref = (T)(sizeof(T) < 4 ? s.nd : 0.f);
  bool all = true, any = false, fin = true;
  for (int c = 0; c < s.C; ++c) {
    const T v = p[(long long)c * plane];
    const bool m = nd_match<T>(v, s.mode, ref, s.nd);
    all = all && m;
    any = any || m;
    if constexpr (sizeof(T) == 4) fin = fin && __builtin_fabsf(v) < __builtin_inff();        // false for NaN
  }
  return fin && !(s.rule == EAE_INVALID_ANY ? any : all);
}

// eae_slic_step's feature: rint(65535 * min(max(v / d, 0), 1)) in double, half to even, NaN -> 0
template <typename T> __device__ __forceinline__ unsigned feature(T v, double d) {
  const double p = (double)v / d;
  const double c = p > 0.0 ? (p < 1.0 ? p : 1.0) : 0.0;
  return (unsigned)(int)__builtin_rint(c * 65535.0);
}

// the LDS word of pixel (y, x): feature | 1 << 16, or 0 for an invalid pixel
template <typename T> __device__ __forceinline__ unsigned stage_word(const RegScene& s, int band, double d, long long y, long long x) {
  if (!pixel_valid<T>(s, y, x)) return 0u;
  const T v = ((const T*)s.data)[((long long)band * s.H + y) * s.W + x];
  return feature<T>(v, d) | 0x10000u;
}

// The geometry of a (T, R): a function of the two alone.
struct MatchPlan { int TW, ND, G, BW, S; size_t lds; };
MatchPlan match_plan(int T, int R) {
  MatchPlan p;
  p.TW = (T + 3) / 4 * 4;
  p.ND = 2 * R + 1;
  p.G = (p.ND + MT_K - 1) / MT_K;
  p.BW = MT_K * p.G + p.TW;                                  // the last item's second read ends at word 4 (G - 1) + TW - 4 + 7
  while (p.BW % 64 != (MT_K * p.G) % 64) p.BW += 4;
  const int pairs = p.ND * p.G;
  p.S = MT_NT / pairs < 1 ? 1 : MT_NT / pairs > T ? T : MT_NT / pairs;
  p.lds = ((size_t)T * p.TW + (size_t)(T + 2 * R) * p.BW) * 4 + (p.S > 1 ? (size_t)p.ND * p.ND * 6 * 8 : 0);
  return p;
}

struct MatchArgs {
  RegScene a, b; int band_a, band_b; const float* div_a; const float* div_b;
  int T, R, n_tiles; const int* oa; const int* ob; long long* sums; int TW, ND, G, BW, S;
};

template <typename TA, typename TB>
__global__ EAE_NO_PK __launch_bounds__(MT_NT) void match_tiles_kernel(MatchArgs m) {
  extern __shared__ __attribute__((aligned(16))) unsigned mt_lds[];
  const int tid = threadIdx.x, T = m.T, R = m.R, TW = m.TW, BW = m.BW, ND = m.ND, G = m.G, S = m.S;
  const int BH = T + 2 * R, NO = ND * ND;
  unsigned* At = mt_lds;                                     // [T][TW]
  unsigned* Bt = mt_lds + T * TW;                            // [BH][BW]; T * TW and BW are multiples of 4: 16-byte rows
  u64* tab = (u64*)(Bt + BH * BW);                           // [NO][6], only when S > 1
  const double da = (double)m.div_a[m.band_a], db = (double)m.div_b[m.band_b];
  const int pairs = ND * G, items = pairs * S;

  for (int tile = blockIdx.x; tile < m.n_tiles; tile += gridDim.x) {
    const long long ay = m.oa[2 * tile], ax = m.oa[2 * tile + 1];
    const long long by = (long long)m.ob[2 * tile] - R, bx = (long long)m.ob[2 * tile + 1] - R;
    for (int idx = tid; idx < T * TW; idx += MT_NT) {
      const int i = idx / TW, j = idx - i * TW;
      At[idx] = j < T ? stage_word<TA>(m.a, m.band_a, da, ay + i, ax + j) : 0u;
    }
    for (int idx = tid; idx < BH * BW; idx += MT_NT) {
      const int i = idx / BW, j = idx - i * BW;
      Bt[idx] = j < BH ? stage_word<TB>(m.b, m.band_b, db, by + i, bx + j) : 0u;
    }
    if (S > 1)
      for (int idx = tid; idx < NO * 6; idx += MT_NT) tab[idx] = 0ull;
    wg_barrier();

    long long* out = m.sums + (long long)tile * NO * 6;      // tile < n_tiles: inside the table
    for (int it = tid; it < items; it += MT_NT) {
      const int s = it / pairs, q = it - s * pairs, dy = q / G, g = q - dy * G;
      const int i0 = s * T / S, i1 = (s + 1) * T / S;
      unsigned n[MT_K], sa[MT_K], sb[MT_K];
      u64 saa[MT_K], sbb[MT_K], sab[MT_K];
#pragma unroll
      for (int k = 0; k < MT_K; ++k) { n[k] = sa[k] = sb[k] = 0u; saa[k] = sbb[k] = sab[k] = 0ull; }
      for (int i = i0; i < i1; ++i) {
        const uint4* arow = reinterpret_cast<const uint4*>(At + i * TW);
        const uint4* brow = reinterpret_cast<const uint4*>(Bt + (dy + i) * BW + MT_K * g);
        for (int jb = 0; jb < TW / 4; ++jb) {
          const uint4 av = arow[jb], b0 = brow[jb], b1 = brow[jb + 1];
          const unsigned aw[4] = {av.x, av.y, av.z, av.w};
          const unsigned bw[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const unsigned ua = aw[e] & 0xffffu, va = aw[e] >> 16;
#pragma unroll
            for (int k = 0; k < MT_K; ++k) {
              const unsigned ub = bw[e + k] & 0xffffu, vb = bw[e + k] >> 16;
              const unsigned am = vb ? ua : 0u, bm = va ? ub : 0u;         // ua is 0 where va is: am, bm are 0 unless both are valid
              n[k] += va & vb;
              sa[k] += am;
              sb[k] += bm;
              saa[k] += (u64)am * am;
              sbb[k] += (u64)bm * bm;
              sab[k] += (u64)ua * ub;
            }
          }
        }
      }
#pragma unroll
      for (int k = 0; k < MT_K; ++k) {
        const int dx = MT_K * g + k;
        if (dx >= ND) continue;
        const int o = (dy * ND + dx) * 6;                    // o + 5 < NO * 6
        const u64 v[6] = {n[k], sa[k], sb[k], saa[k], sbb[k], sab[k]};
        if (S > 1) {
#pragma unroll
          for (int e = 0; e < 6; ++e) lds_add64(tab + o + e, v[e]);
        } else {
#pragma unroll
          for (int e = 0; e < 6; ++e) out[o + e] = (long long)v[e];
        }
      }
    }
    wg_barrier();                                            // the items are done with the tiles; the table is complete
    if (S > 1) {
      for (int idx = tid; idx < NO * 6; idx += MT_NT) out[idx] = (long long)tab[idx];
      wg_barrier();                                          // the table is free for the next tile
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------
// resampling
// ---------------------------------------------------------------------------------------------------------------
// One correctly rounded float64 product or sum that no later pass may fuse: this toolchain's __dmul_rn and __dadd_rn are the plain
// operators compiled with contraction allowed, and a product inlined from there still merges with a following sum.
__device__ __forceinline__ double rn_mul(double x, double y) {
#pragma clang fp contract(off)
  return x * y;
}
__device__ __forceinline__ double rn_add(double x, double y) {
#pragma clang fp contract(off)
  return x + y;
}

struct ResampleArgs {
  RegScene s; void* dst; unsigned char* out_valid; double m[6]; double fill; int Hd, Wd; unsigned bx;
};

// The taps of one axis at source coordinate s (finite): their number is NT = 1, 2 or 4; base receives the first tap's coordinate (an
// integer held in a double), w the weights in the header's order of operations.
template <int METHOD> __device__ __forceinline__ void axis_taps(double s, double* base, double* w) {
#pragma clang fp contract(off)
  if constexpr (METHOD == EAE_RESAMPLE_NEAREST) {
    *base = __builtin_floor(rn_add(s, 0.5));
    w[0] = 1.0;
  } else {
    const double f = __builtin_floor(s), t = rn_add(s, -f);
    if constexpr (METHOD == EAE_RESAMPLE_BILINEAR) {
      *base = f;
      w[0] = rn_add(1.0, -t);
      w[1] = t;
    } else {                                                 // Catmull-Rom, a = -0.5, Horner
      *base = rn_add(f, -1.0);
      w[0] = rn_mul(rn_add(rn_mul(rn_add(rn_mul(-0.5, t), 1.0), t), -0.5), t);
      w[1] = rn_add(rn_mul(rn_mul(rn_add(rn_mul(1.5, t), -2.5), t), t), 1.0);
      w[2] = rn_mul(rn_add(rn_mul(rn_add(rn_mul(-1.5, t), 2.0), t), 0.5), t);
      w[3] = rn_mul(rn_mul(rn_add(rn_mul(0.5, t), -0.5), t), t);
    }
  }
}

template <typename T> __device__ __forceinline__ T resample_cast(double v) {
  if constexpr (sizeof(T) == 4) return (float)v;
  else {
    const double hi = sizeof(T) == 1 ? 255.0 : 65535.0, r = __builtin_rint(v);
    return (T)(int)(r < 0.0 ? 0.0 : r > hi ? hi : r);
  }
}

template <typename T, int METHOD>
__global__ EAE_NO_PK __launch_bounds__(256) void scene_resample_kernel(ResampleArgs a) {
#pragma clang fp contract(off)
  constexpr int NT = METHOD == EAE_RESAMPLE_NEAREST ? 1 : METHOD == EAE_RESAMPLE_BILINEAR ? 2 : 4;
  const int tid = threadIdx.x;
  const long long x = (long long)(blockIdx.x % a.bx) * 64 + (tid & 63), y = (long long)(blockIdx.x / a.bx) * 4 + (tid >> 6);
  if (x >= a.Wd || y >= a.Hd) return;
  const double xd = (double)x, yd = (double)y;
  const double sx = rn_add(rn_add(rn_mul(a.m[0], xd), rn_mul(a.m[1], yd)), a.m[2]);
  const double sy = rn_add(rn_add(rn_mul(a.m[3], xd), rn_mul(a.m[4], yd)), a.m[5]);
  bool ok = __builtin_fabs(sx) < __builtin_inf() && __builtin_fabs(sy) < __builtin_inf();
  double wx[NT], wy[NT], bxs = 0.0, bys = 0.0;
  int xi[NT], yi[NT];                                        // the taps' source columns and rows; -1: outside the raster
  if (ok) {
    axis_taps<METHOD>(sx, &bxs, wx);
    axis_taps<METHOD>(sy, &bys, wy);
#pragma unroll
    for (int k = 0; k < NT; ++k) {
      const double cx = bxs + (double)k, cy = bys + (double)k;           // exact below 2^53; beyond it far outside either way
      xi[k] = cx >= 0.0 && cx <= (double)(a.s.W - 1) ? (int)cx : -1;
      yi[k] = cy >= 0.0 && cy <= (double)(a.s.H - 1) ? (int)cy : -1;
    }
    // every tap whose two axis weights are both non-zero must be a valid source pixel
#pragma unroll
    for (int r = 0; r < NT; ++r)
#pragma unroll
      for (int c = 0; c < NT; ++c)
        if (ok && wy[r] != 0.0 && wx[c] != 0.0) ok = yi[r] >= 0 && xi[c] >= 0 && pixel_valid<T>(a.s, yi[r], xi[c]);
  }
  const long long pd = (long long)a.Hd * a.Wd, ps = (long long)a.s.H * a.s.W, at = y * a.Wd + x;
  T* dst = (T*)a.dst + at;
  if (a.out_valid) a.out_valid[at] = ok ? 1 : 0;
  if (!ok) {
    const T f = resample_cast<T>(a.fill);
    for (int c = 0; c < a.s.C; ++c) dst[(long long)c * pd] = f;
    return;
  }
  for (int b = 0; b < a.s.C; ++b) {
    const T* src = (const T*)a.s.data + (long long)b * ps;
    double acc = 0.0;
    bool first = true;
#pragma unroll
    for (int r = 0; r < NT; ++r)
#pragma unroll
      for (int c = 0; c < NT; ++c)
        if (wy[r] != 0.0 && wx[c] != 0.0) {                  // rows ascending, then columns; the first term starts the sum
          const double term = rn_mul(rn_mul(wy[r], wx[c]), (double)src[(long long)yi[r] * a.s.W + xi[c]]);
          acc = first ? term : rn_add(acc, term);
          first = false;
        }
    dst[(long long)b * pd] = resample_cast<T>(acc);
  }
}

int reg_fail(const char* who, const char* what) {
  static thread_local char msg[200];
  snprintf(msg, sizeof msg, "%s: %s", who, what);
  return eae_set_error(EAE_ERR_ARG, msg);
}

int elem_bytes(int dtype) { return dtype == EAE_SCENE_U8 ? 1 : dtype == EAE_SCENE_U16 ? 2 : dtype == EAE_SCENE_F32 ? 4 : 0; }

// the checks of one scene that the two calls share
int scene_check(const char* who, const void* p, int dtype, int C, int H, int W, int mode, float nd, int rule) {
  if (!p) return reg_fail(who, "NULL scene");
  const int eb = elem_bytes(dtype);
  if (!eb) return reg_fail(who, "unknown dtype");
  if (reinterpret_cast<uintptr_t>(p) % (unsigned)eb) return reg_fail(who, "a scene pointer is not aligned to its element size");
  if (C < 1 || C > RG_MAX_C) return reg_fail(who, "the number of bands must be in 1..16");
  if (H < 1 || W < 1) return reg_fail(who, "empty raster");
  if ((long long)H * W >= (1LL << 31)) return reg_fail(who, "H * W must be below 2^31");
  if (mode != EAE_NODATA_NONE && mode != EAE_NODATA_VALUE && mode != EAE_NODATA_NAN) return reg_fail(who, "unknown nodata mode");
  if (rule != EAE_INVALID_ALL && rule != EAE_INVALID_ANY) return reg_fail(who, "unknown nodata rule");
  if (dtype != EAE_SCENE_F32 && mode == EAE_NODATA_NAN) return reg_fail(who, "a NaN nodata needs an fp32 scene");
  if (dtype != EAE_SCENE_F32 && mode == EAE_NODATA_VALUE) {
    const float hi = dtype == EAE_SCENE_U8 ? 255.f : 65535.f;
    if (!(nd >= 0.f && nd <= hi) || nd != (float)(int)nd) return reg_fail(who, "nodata must be an integer in the scene dtype's range");
  }
  return 0;
}

// f(T{}) for the element type
template <typename F> void for_dtype(int dtype, F&& f) {
  if (dtype == EAE_SCENE_U8) f((unsigned char)0);
  else if (dtype == EAE_SCENE_U16) f((unsigned short)0);
  else f(0.f);
}

}  // namespace

extern "C" int eae_match_tiles(void* stream, const void* a, int dtype_a, int Ca, int Ha, int Wa, int band_a, const float* div_a,
                               int nodata_mode_a, float nodata_a, int rule_a, const unsigned char* mask_a, const void* b, int dtype_b,
                               int Cb, int Hb, int Wb, int band_b, const float* div_b, int nodata_mode_b, float nodata_b, int rule_b,
                               const unsigned char* mask_b, int tile, int radius, int n_tiles, const int* origins_a,
                               const int* origins_b, long long* sums) {
  const char* who = "match_tiles";
  if (const int rc = scene_check(who, a, dtype_a, Ca, Ha, Wa, nodata_mode_a, nodata_a, rule_a)) return rc;
  if (const int rc = scene_check(who, b, dtype_b, Cb, Hb, Wb, nodata_mode_b, nodata_b, rule_b)) return rc;
  if (!div_a || !div_b) return reg_fail(who, "NULL divisor");
  if (band_a < 0 || band_a >= Ca || band_b < 0 || band_b >= Cb) return reg_fail(who, "a band index lies outside its scene");
  if (tile < MT_MIN_T || tile > MT_MAX_T) return reg_fail(who, "tile must be in 4..64");
  if (radius < 0 || radius > MT_MAX_R) return reg_fail(who, "radius must be in 0..16");
  if (n_tiles < 1 || n_tiles > MT_MAX_TILES) return reg_fail(who, "n_tiles must be in 1..2^20");
  if (!origins_a || !origins_b || !sums) return reg_fail(who, "NULL origin table or sums");
  EAE_NO_GROUP("match_tiles_kernel");
  const MatchPlan p = match_plan(tile, radius);
  MatchArgs m;
  m.a = {a, mask_a, Ca, Ha, Wa, nodata_mode_a, rule_a, nodata_a};
  m.b = {b, mask_b, Cb, Hb, Wb, nodata_mode_b, rule_b, nodata_b};
  m.band_a = band_a; m.band_b = band_b; m.div_a = div_a; m.div_b = div_b;
  m.T = tile; m.R = radius; m.n_tiles = n_tiles; m.oa = origins_a; m.ob = origins_b; m.sums = sums;
  m.TW = p.TW; m.ND = p.ND; m.G = p.G; m.BW = p.BW; m.S = p.S;
  const dim3 grid((unsigned)(n_tiles < MT_GRID ? n_tiles : MT_GRID));
  int rc = 0;
  for_dtype(dtype_a, [&](auto ta) {
    for_dtype(dtype_b, [&](auto tb) {
      auto k = match_tiles_kernel<decltype(ta), decltype(tb)>;
      if (p.lds > 48 * 1024) {                               // at most 66 KiB (T = 64, R = 10)
        const hipError_t e = eae_smem_attr(reinterpret_cast<const void*>(k), p.lds);
        if (e != hipSuccess) { rc = eae_set_error(-3, hipGetErrorString(e)); return; }
      }
      hipLaunchKernelGGL(k, grid, dim3(MT_NT), p.lds, (hipStream_t)stream, m);
    });
  });
  if (rc) return rc;
  EAE_LAUNCH_CHECK();
  return 0;
}

extern "C" int eae_scene_resample(void* stream, const void* src, int dtype, int C, int Hs, int Ws, int nodata_mode, float nodata,
                                  int rule, const unsigned char* mask_src, const double* matrix, int method, double fill, void* dst,
                                  int Hd, int Wd, unsigned char* out_valid) {
  const char* who = "scene_resample";
  if (const int rc = scene_check(who, src, dtype, C, Hs, Ws, nodata_mode, nodata, rule)) return rc;
  if (!matrix || !dst) return reg_fail(who, "NULL matrix or dst");
  if (reinterpret_cast<uintptr_t>(dst) % (unsigned)elem_bytes(dtype)) return reg_fail(who, "dst is not aligned to its element size");
  if (method != EAE_RESAMPLE_NEAREST && method != EAE_RESAMPLE_BILINEAR && method != EAE_RESAMPLE_CUBIC)
    return reg_fail(who, "unknown method");
  if (Hd < 1 || Wd < 1) return reg_fail(who, "empty destination raster");
  if ((long long)Hd * Wd >= (1LL << 31)) return reg_fail(who, "Hd * Wd must be below 2^31");
  ResampleArgs r;
  for (int i = 0; i < 6; ++i) {
    if (!(__builtin_fabs(matrix[i]) < __builtin_inf())) return reg_fail(who, "a matrix entry is not finite");
    r.m[i] = matrix[i];
  }
  if (dtype != EAE_SCENE_F32 && !(fill >= 0.0 && fill <= (dtype == EAE_SCENE_U8 ? 255.0 : 65535.0)))
    return reg_fail(who, "fill lies outside the scene dtype's range");
  EAE_NO_GROUP("scene_resample_kernel");
  r.s = {src, mask_src, C, Hs, Ws, nodata_mode, rule, nodata};
  r.dst = dst; r.out_valid = out_valid; r.fill = fill; r.Hd = Hd; r.Wd = Wd;
  r.bx = (unsigned)((Wd + 63) / 64);
  const long long blocks = (long long)r.bx * ((Hd + 3) / 4);            // below 2^31 / 4 + 2^29
  const dim3 grid((unsigned)blocks);
  for_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    if (method == EAE_RESAMPLE_NEAREST) hipLaunchKernelGGL((scene_resample_kernel<T, EAE_RESAMPLE_NEAREST>), grid, dim3(256), 0, (hipStream_t)stream, r);
    else if (method == EAE_RESAMPLE_BILINEAR) hipLaunchKernelGGL((scene_resample_kernel<T, EAE_RESAMPLE_BILINEAR>), grid, dim3(256), 0, (hipStream_t)stream, r);
    else hipLaunchKernelGGL((scene_resample_kernel<T, EAE_RESAMPLE_CUBIC>), grid, dim3(256), 0, (hipStream_t)stream, r);
  });
  EAE_LAUNCH_CHECK();
  return 0;
}
