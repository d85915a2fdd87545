// Change detection between two scenes (include/eae.h, "change detection"): the two passes of an IR-MAD iteration
// over a pair of planar [C][H][W] scenes of uint8 / uint16 / float32, read in place.  The pixel vector is v = [x_0 .. x_{C-1}, y_0 ..
// y_{C-1}], x_c = a_c / div_a[c], y_c = b_c / div_b[c], each one fp32 division.
//   moments:  N = sum w, s = sum w (v - p), S = sum w (v - p)(v - p)^T over the valid pixels.  The raster is cut into G chunks of CH
//             pixels, both functions of (C, H, W) alone; one wave takes one chunk at a time.  It stages 128 pixels in LDS (a lane reads
//             consecutive pixels of one plane: coalesced; validity is decided per pixel while its bands pass through the lane), then
//             feeds them to v_mfma_f32_32x32x2_f32 with A = w d and B = d.  2 C is padded to D = 2, 4, 8, 16 or 32 and the 32 x 32 tile
//             holds R = 32 / D independent pixel streams on its diagonal D x D blocks, so an instruction takes 2 R pixels (the blocks off
//             the diagonal mix two streams and are never read).  s, N and the count accumulate in the lane beside the MFMA.  Every
//             chunk stores its whole partial (tile, s, N, count: CH_PART words); the finalize kernel adds the partials in float64,
//             chunks ascending and streams ascending inside a chunk, and writes S[i][j] and S[j][i] from one register.  No float
//             atomics; every partial word that is read has been written.
//   variates: M_i = sum_j T[j][i] (v_j - mean_j), one fma chain in ascending j per pixel and i; Z = sum_i M_i^2, one fma chain in
//             ascending i; prob = Q(dof / 2, Z / 2) in closed form.  One pixel a thread; T and the mean come from LDS (uniform reads).
//             A pixel's results depend on its own values and the model alone.
#include "eae_internal.h"
#include "eae_common.hip.h"
#include "eae_latent.hip.h"

namespace {

constexpr int CH_MAX_C = 16;
constexpr int CH_TP = 128;                  // pixels a wave stages at a time: two per lane
constexpr int CH_MIN_CHUNK = 256;           // pixels of the smallest chunk; every chunk size is a multiple of it (and so of CH_TP)
constexpr int CH_MAX_CHUNKS = 4096;
constexpr int CH_PART = 1024 + 3 * 64;      // words of a chunk's partial: the tile register-major, then s, N and the count per lane
constexpr int CH_GRID = 2048;               // most waves of the moments launch (one wave a workgroup)

struct ChangePair {
  const void* a; const void* b; const float* div_a; const float* div_b;
  int mode_a; float nd_a; int rule_a; int mode_b; float nd_b; int rule_b;
  const unsigned char* mask; int C; long long P;          // P = H * W: pixels of a plane
};

__device__ __forceinline__ void wg_barrier() {          // (builtins: see eae_slic.hip)
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

template <typename T> __device__ __forceinline__ bool nd_match(T v, int mode, T ref, float fref) {
  if (mode == EAE_NODATA_NONE) return false;
  if constexpr (sizeof(T) == 4) return mode == EAE_NODATA_NAN ? v != v : v == fref;
  else return v == ref;
}

// One scene's bands of pixel px through the lane: f(c, x_c) for every band, x_c = v / div[c] (one fp32 division; none for a divisor of
// 1, which gives the same bits).  Returns whether the scene leaves the pixel valid: its nodata rule does not fire and, for float32,
// every band is finite.
template <typename T, typename F>
__device__ __forceinline__ bool scene_bands(const T* __restrict__ src, long long plane, long long px, int C, const float* __restrict__ div,
                                            int mode, float nd, int rule, F&& f) {
  bool all = true, any = false, fin = true;
  const T ref = (T)(sizeof(T) < 4 ? nd : 0.f);
#pragma unroll 4
  for (int c = 0; c < C; ++c) {
    const T v = src[(long long)c * plane + px];
    const bool m = nd_match<T>(v, mode, ref, nd);
    all = all && m;
    any = any || m;
    const float x = (float)v, d = div[c];
    if constexpr (sizeof(T) == 4) fin = fin && __builtin_fabsf(x) < __builtin_inff();       // false for NaN
    f(c, d == 1.f ? x : x / d);
  }
  return fin && !(rule == EAE_INVALID_ANY ? any : all);
}

// ---------------------------------------------------------------------------------------------------------------
// moments, first kernel.  One wave a workgroup; wave g0 takes the chunks g0, g0 + gridDim.x, ..  LDS: rows 0 .. 2 C - 1 hold d = v - p
// of the staged pixels, row 2 C the weight (-1 for a pixel that takes no part, whose d are zeros), each row CH_TP + 2 R words: lane
// (r, h) of MFMA step t reads slot 2 R t + 2 q + h of row i (r = q D + i), word i (CH_TP + 2 R) + slot: 64 different banks.
// ---------------------------------------------------------------------------------------------------------------
struct MomentsArgs { ChangePair s; const float* weights; const float* pivot; float* part; int G, chunk, D; };

template <typename TA, typename TB>
__global__ EAE_NO_PK __launch_bounds__(64) void change_moments_kernel(MomentsArgs a) {
  extern __shared__ float ch_lds[];
  const int lane = threadIdx.x, r = lane & 31, h = lane >> 5;
  const int C = a.s.C, n2 = 2 * C, D = a.D, R = 32 / D, LS = CH_TP + 2 * R;
  const int q = r / D, i = r % D;
  const bool live = i < n2;
  const long long P = a.s.P;
  const TA* pa = (const TA*)a.s.a;
  const TB* pb = (const TB*)a.s.b;
  float* wrow = ch_lds + n2 * LS;
  const float* drow = ch_lds + (live ? i : 0) * LS;
  const int steps = CH_TP / (2 * R);

  for (int g = blockIdx.x; g < a.G; g += gridDim.x) {
    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
    float sa = 0.f, sw = 0.f;
    int cnt = 0;
    const long long p0 = (long long)g * a.chunk, p1 = p0 + a.chunk < P ? p0 + a.chunk : P;
    for (long long t0 = p0; t0 < p1; t0 += CH_TP) {
#pragma unroll
      for (int u = 0; u < CH_TP / 64; ++u) {
        const int slot = u * 64 + lane;
        const long long px = t0 + slot;
        bool ok = px < p1;
        float w = 1.f;
        if (ok) {
          float* col = ch_lds + slot;
          const bool va = scene_bands<TA>(pa, P, px, C, a.s.div_a, a.s.mode_a, a.s.nd_a, a.s.rule_a,
                                          [&](int c, float x) { col[c * LS] = x - a.pivot[c]; });
          const bool vb = scene_bands<TB>(pb, P, px, C, a.s.div_b, a.s.mode_b, a.s.nd_b, a.s.rule_b,
                                          [&](int c, float x) { col[(C + c) * LS] = x - a.pivot[C + c]; });
          if (a.weights) w = a.weights[px];
          ok = va && vb && w >= 0.f && w < __builtin_inff() && !(a.s.mask && a.s.mask[px]);
        }
        if (!ok)
          for (int c = 0; c < n2; ++c) ch_lds[c * LS + slot] = 0.f;
        wrow[slot] = ok ? w : -1.f;
      }
      wg_barrier();
      for (int t = 0; t < steps; ++t) {
        const int slot = 2 * R * t + 2 * q + h;
        const float wv = wrow[slot];
        const bool valid = wv >= 0.f;
        const float w = valid ? wv : 0.f;
        const float d = live ? drow[slot] : 0.f;
        const float av = w * d;
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, d, acc, 0, 0, 0);
        sa += av;
        sw += w;
        cnt += valid;
      }
      wg_barrier();                                        // the tile is free for the next 128 pixels
    }
    float* out = a.part + (size_t)g * CH_PART + lane;      // chunk g < G: inside the workspace
#pragma unroll
    for (int e = 0; e < 16; ++e) out[e * 64] = acc[e];
    out[1024] = sa;
    out[1088] = sw;
    reinterpret_cast<int*>(out)[1152] = cnt;
  }
}

// moments, second kernel: workgroup e owns one output: S[i][j] (i <= j, row-major over the upper triangle), then s[i], N, the count.
// Thread t adds the chunks [t L, (t + 1) L), L = ceil(G / 256), in ascending order and, inside a chunk, the streams q in ascending
// order (for s and N: lane half 0, then 1), all in float64; thread 0 then adds the 256 sums in ascending t.  The order is a function
// of G and D alone.
struct FinalArgs { const float* part; int G, C, D; double* mom; long long* count; };

__global__ EAE_NO_PK __launch_bounds__(256) void change_finalize_kernel(FinalArgs a) {
  __shared__ double red[256];
  const int tid = threadIdx.x, n2 = 2 * a.C, D = a.D, R = 32 / D, tri = n2 * (n2 + 1) / 2;
  int e = blockIdx.x, kind = 0, i = 0, j = 0;
  if (e < tri) {
    while (e >= n2 - i) { e -= n2 - i; ++i; }
    j = i + e;
  } else if (e < tri + n2) { kind = 1; i = e - tri; }
  else kind = e == tri + n2 ? 2 : 3;
  const int L = (a.G + 255) / 256, g0 = tid * L, g1 = g0 + L < a.G ? g0 + L : a.G;
  double s = 0.0;
  for (int g = g0; g < g1; ++g) {
    const float* p = a.part + (size_t)g * CH_PART;
    for (int q = 0; q < R; ++q) {
      if (kind == 0) {
        const int row = q * D + i, col = q * D + j;        // element (row, col) of the tile: register (row & 3) + 4 (row >> 3), half (row >> 2) & 1
        s += (double)p[((row & 3) + 4 * (row >> 3)) * 64 + ((row >> 2) & 1) * 32 + col];
      } else if (kind == 1) {
        s += (double)p[1024 + q * D + i];
        s += (double)p[1024 + 32 + q * D + i];
      } else if (kind == 2) {
        s += (double)p[1088 + q * D];
        s += (double)p[1088 + 32 + q * D];
      } else {                                             // a chunk counts fewer than 2^31 pixels: exact in a double
        const int* c = reinterpret_cast<const int*>(p);
        s += (double)(c[1152 + q * D] + c[1152 + 32 + q * D]);
      }
    }
  }
  red[tid] = s;
  wg_barrier();
  if (tid) return;
  double t = 0.0;
  for (int k = 0; k < 256; ++k) t += red[k];
  if (kind == 0) {
    a.mom[1 + n2 + i * n2 + j] = t;
    a.mom[1 + n2 + j * n2 + i] = t;
  } else if (kind == 1) a.mom[1 + i] = t;
  else if (kind == 2) a.mom[0] = t;
  else *a.count = (long long)t;
}

// The geometry, a function of (C, H, W) alone: chunks of a multiple of 256 pixels, at most 4096 of them; D = 2 C rounded up to a power
// of two.
struct MomentsPlan { int G, chunk, D; };
MomentsPlan change_plan(int C, long long P) {
  MomentsPlan p;
  const long long per = (P + CH_MAX_CHUNKS - 1) / CH_MAX_CHUNKS;
  long long chunk = (per + CH_MIN_CHUNK - 1) / CH_MIN_CHUNK * CH_MIN_CHUNK;
  if (chunk < CH_MIN_CHUNK) chunk = CH_MIN_CHUNK;
  p.chunk = (int)chunk;
  p.G = (int)((P + chunk - 1) / chunk);
  p.D = 2;
  while (p.D < 2 * C) p.D *= 2;
  return p;
}

// ---------------------------------------------------------------------------------------------------------------
// Q(dof / 2, z / 2), the chi-square survival function for integer dof 1..16, h = z / 2:
//   dof = 2 m:     e^-h sum_{j < m} h^j / j!
//   dof = 2 m + 1: erfc(sqrt h) + e^-h sum_{j = 1..m} h^(j - 1/2) / Gamma(j + 1/2)
// every term from its predecessor (t_j = t_{j-1} h / j, or h / (j - 1/2)); e^-h is applied as two factors e^(-h / 2), so that the
// product passes no subnormal while the result is a normal number.  Above h = 128 the value is below 2^-126 for every dof: 0.
// z = NaN gives NaN.
// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float chi2_q(int dof, float z) {
  const float h = 0.5f * z;
  if (!(h <= 128.f)) return h != h ? h : 0.f;
  if (!(h > 0.f)) return 1.f;
  const float e2 = expf(-0.5f * h);
  const int m = dof >> 1;
  if (dof & 1) {
    const float rt = sqrtf(h);
    float t = rt * 1.1283791671f, s = 0.f;                 // 1 / Gamma(3/2) = 2 / sqrt(pi)
    for (int j = 1; j <= m; ++j) {
      if (j > 1) t *= h / ((float)j - 0.5f);
      s += t;
    }
    return erfcf(rt) + (s * e2) * e2;
  }
  float t = 1.f, s = 1.f;
  for (int j = 1; j < m; ++j) {
    t *= h / (float)j;
    s += t;
  }
  return (s * e2) * e2;
}

struct VariatesArgs { ChangePair s; const float* mean; const float* T; int dof; float* chi2; float* prob; float* var; };

template <typename TA, typename TB>
__global__ EAE_NO_PK __launch_bounds__(256) void change_variates_kernel(VariatesArgs a) {
  __shared__ __attribute__((aligned(16))) float Ts[2 * CH_MAX_C][CH_MAX_C];     // T, zero beyond column C - 1
  __shared__ float ms[2 * CH_MAX_C];
  const int tid = threadIdx.x, C = a.s.C, n2 = 2 * C;
  for (int idx = tid; idx < 2 * CH_MAX_C * CH_MAX_C; idx += 256) {
    const int j = idx / CH_MAX_C, i = idx % CH_MAX_C;
    Ts[j][i] = j < n2 && i < C ? a.T[j * C + i] : 0.f;
  }
  if (tid < 2 * CH_MAX_C) ms[tid] = tid < n2 ? a.mean[tid] : 0.f;
  wg_barrier();
  const long long P = a.s.P, px = (long long)blockIdx.x * 256 + tid;
  if (px >= P) return;
  float M[CH_MAX_C];
#pragma unroll
  for (int i = 0; i < CH_MAX_C; ++i) M[i] = 0.f;
  // j ascending: the bands of A, then those of B; a column beyond C - 1 multiplies by zero and stays zero
  const bool va = scene_bands<TA>((const TA*)a.s.a, P, px, C, a.s.div_a, a.s.mode_a, a.s.nd_a, a.s.rule_a, [&](int c, float x) {
    const float d = x - ms[c];
#pragma unroll
    for (int i = 0; i < CH_MAX_C; ++i) M[i] = __builtin_fmaf(Ts[c][i], d, M[i]);
  });
  const bool vb = scene_bands<TB>((const TB*)a.s.b, P, px, C, a.s.div_b, a.s.mode_b, a.s.nd_b, a.s.rule_b, [&](int c, float x) {
    const float d = x - ms[C + c];
#pragma unroll
    for (int i = 0; i < CH_MAX_C; ++i) M[i] = __builtin_fmaf(Ts[C + c][i], d, M[i]);
  });
  const bool ok = va && vb && !(a.s.mask && a.s.mask[px]);
  const float nan = __builtin_nanf("");
  float z = 0.f;
#pragma unroll
  for (int i = 0; i < CH_MAX_C; ++i) z = __builtin_fmaf(M[i], M[i], z);          // (+ 0 beyond C - 1: exact)
  if (a.chi2) a.chi2[px] = ok ? z : nan;
  if (a.prob) a.prob[px] = ok ? chi2_q(a.dof, z) : 0.f;
  if (a.var) {
#pragma unroll
    for (int i = 0; i < CH_MAX_C; ++i)
      if (i < C) a.var[(long long)i * P + px] = ok ? M[i] : nan;
  }
}

int change_fail(const char* who, const char* what) {
  static thread_local char msg[200];
  snprintf(msg, sizeof msg, "%s: %s", who, what);
  return eae_set_error(EAE_ERR_ARG, msg);
}

int elem_bytes(int dtype) { return dtype == EAE_SCENE_U8 ? 1 : dtype == EAE_SCENE_U16 ? 2 : dtype == EAE_SCENE_F32 ? 4 : 0; }

int nodata_check(const char* who, int dtype, int mode, float nd, int rule) {
  if (mode != EAE_NODATA_NONE && mode != EAE_NODATA_VALUE && mode != EAE_NODATA_NAN) return change_fail(who, "unknown nodata mode");
  if (rule != EAE_INVALID_ALL && rule != EAE_INVALID_ANY) return change_fail(who, "unknown nodata rule");
  if (dtype != EAE_SCENE_F32 && mode == EAE_NODATA_NAN) return change_fail(who, "a NaN nodata needs an fp32 scene");
  if (dtype != EAE_SCENE_F32 && mode == EAE_NODATA_VALUE) {
    const float hi = dtype == EAE_SCENE_U8 ? 255.f : 65535.f;
    if (!(nd >= 0.f && nd <= hi) || nd != (float)(int)nd) return change_fail(who, "nodata must be an integer in the scene dtype's range");
  }
  return 0;
}

// every check the two calls share; fills the pair
int pair_check(const char* who, const void* a, const void* b, int dtype_a, int dtype_b, int C, int H, int W, const float* div_a,
               const float* div_b, int mode_a, float nd_a, int rule_a, int mode_b, float nd_b, int rule_b, const unsigned char* mask,
               ChangePair* out) {
  if (!a || !b || !div_a || !div_b) return change_fail(who, "NULL scene or divisor");
  const int ea = elem_bytes(dtype_a), eb = elem_bytes(dtype_b);
  if (!ea || !eb) return change_fail(who, "unknown dtype");
  if (reinterpret_cast<uintptr_t>(a) % (unsigned)ea || reinterpret_cast<uintptr_t>(b) % (unsigned)eb)
    return change_fail(who, "a scene pointer is not aligned to its element size");
  if (C < 1 || C > CH_MAX_C) return change_fail(who, "the number of bands must be in 1..16");
  if (H < 1 || W < 1) return change_fail(who, "empty raster");
  if ((long long)H * W >= (1LL << 31)) return change_fail(who, "H * W must be below 2^31");
  if (const int rc = nodata_check(who, dtype_a, mode_a, nd_a, rule_a)) return rc;
  if (const int rc = nodata_check(who, dtype_b, mode_b, nd_b, rule_b)) return rc;
  *out = {a, b, div_a, div_b, mode_a, nd_a, rule_a, mode_b, nd_b, rule_b, mask, C, (long long)H * W};
  return 0;
}

// f(TA{}, TB{}) for the pair of element types
template <typename F> void for_dtypes(int dtype_a, int dtype_b, F&& f) {
  auto second = [&](auto ta) {
    if (dtype_b == EAE_SCENE_U8) f(ta, (unsigned char)0);
    else if (dtype_b == EAE_SCENE_U16) f(ta, (unsigned short)0);
    else f(ta, 0.f);
  };
  if (dtype_a == EAE_SCENE_U8) second((unsigned char)0);
  else if (dtype_a == EAE_SCENE_U16) second((unsigned short)0);
  else second(0.f);
}

}  // namespace

extern "C" long long eae_change_moments_workspace_bytes(int C, int H, int W) {
  const char* who = "change_moments_workspace_bytes";
  if (C < 1 || C > CH_MAX_C) return change_fail(who, "the number of bands must be in 1..16");
  if (H < 1 || W < 1) return change_fail(who, "empty raster");
  if ((long long)H * W >= (1LL << 31)) return change_fail(who, "H * W must be below 2^31");
  return (long long)change_plan(C, (long long)H * W).G * CH_PART * 4;
}

extern "C" int eae_change_moments(void* stream, const void* a, const void* b, int dtype_a, int dtype_b, int C, int H, int W,
                                  const float* div_a, const float* div_b, int nodata_mode_a, float nodata_a, int rule_a,
                                  int nodata_mode_b, float nodata_b, int rule_b, const unsigned char* mask, const float* weights,
                                  const float* pivot, double* out_moments, long long* out_count, void* workspace,
                                  long long workspace_bytes) {
  const char* who = "change_moments";
  MomentsArgs m;
  if (const int rc = pair_check(who, a, b, dtype_a, dtype_b, C, H, W, div_a, div_b, nodata_mode_a, nodata_a, rule_a, nodata_mode_b,
                                nodata_b, rule_b, mask, &m.s)) return rc;
  if (!pivot || !out_moments || !out_count) return change_fail(who, "NULL pivot, out_moments or out_count");
  const MomentsPlan p = change_plan(C, m.s.P);
  if (!workspace || workspace_bytes < (long long)p.G * CH_PART * 4)
    return change_fail(who, "the workspace is NULL or smaller than eae_change_moments_workspace_bytes");
  EAE_NO_GROUP("change_moments_kernel");
  const hipStream_t st = (hipStream_t)stream;
  m.weights = weights; m.pivot = pivot; m.part = (float*)workspace; m.G = p.G; m.chunk = p.chunk; m.D = p.D;
  const size_t lds = (size_t)(2 * C + 1) * (CH_TP + 2 * (32 / p.D)) * sizeof(float);        // at most 33 x 130 words
  const dim3 grid((unsigned)(p.G < CH_GRID ? p.G : CH_GRID));
  for_dtypes(dtype_a, dtype_b, [&](auto ta, auto tb) {
    hipLaunchKernelGGL((change_moments_kernel<decltype(ta), decltype(tb)>), grid, dim3(64), lds, st, m);
  });
  EAE_LAUNCH_CHECK();
  const FinalArgs f = {(const float*)workspace, p.G, C, p.D, out_moments, out_count};
  hipLaunchKernelGGL(change_finalize_kernel, dim3((unsigned)(C * (2 * C + 1) + 2 * C + 2)), dim3(256), 0, st, f);
  EAE_LAUNCH_CHECK();
  return 0;
}

extern "C" int eae_change_variates(void* stream, const void* a, const void* b, int dtype_a, int dtype_b, int C, int H, int W,
                                   const float* div_a, const float* div_b, int nodata_mode_a, float nodata_a, int rule_a,
                                   int nodata_mode_b, float nodata_b, int rule_b, const unsigned char* mask, const float* mean,
                                   const float* T, int dof, float* out_chi2, float* out_prob, float* out_variates) {
  const char* who = "change_variates";
  VariatesArgs v;
  if (const int rc = pair_check(who, a, b, dtype_a, dtype_b, C, H, W, div_a, div_b, nodata_mode_a, nodata_a, rule_a, nodata_mode_b,
                                nodata_b, rule_b, mask, &v.s)) return rc;
  if (!mean || !T) return change_fail(who, "NULL mean or T");
  if (dof < 1 || dof > 16) return change_fail(who, "dof must be in 1..16");
  if (!out_chi2 && !out_prob && !out_variates) return 0;
  EAE_NO_GROUP("change_variates_kernel");
  v.mean = mean; v.T = T; v.dof = dof; v.chi2 = out_chi2; v.prob = out_prob; v.var = out_variates;
  const dim3 grid((unsigned)((v.s.P + 255) / 256));
  for_dtypes(dtype_a, dtype_b, [&](auto ta, auto tb) {
    hipLaunchKernelGGL((change_variates_kernel<decltype(ta), decltype(tb)>), grid, dim3(256), 0, (hipStream_t)stream, v);
  });
  EAE_LAUNCH_CHECK();
  return 0;
}
