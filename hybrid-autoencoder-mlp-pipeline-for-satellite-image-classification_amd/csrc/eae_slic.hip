// Superpixels (include/eae.h, "superpixels"): SLIC over a [C][H][W] scene, integers only.
//   step:    one pass that fuses assignment and accumulation.  A workgroup takes one tile of SL_TH x SL_TW pixels; wave w takes the rows
//            4 w .. 4 w + 3 of the tile and a lane one column, so a wave's load is 64 consecutive elements of one row of one band at
//            whatever alignment the row starts, and its label store 256 consecutive bytes.  The pixels of a tile can only choose among the
//            clusters of the cells the tile overlaps plus one ring: their centres are staged in LDS ([rows][C + 3] int32) beside a table
//            of 32-bit accumulators of the same shape.  A value is quantised with one multiplication by 1 / divisor and a division only
//            where that could round differently (slic_q).  A pixel compares its (at most) nine candidates band by band (one quantised value
//            in registers at a time, nine 64-bit colour sums), takes the smallest D, the lowest id on a tie, and adds itself to the
//            winner's row: count, y and x relative to the tile's origin, and, in a second pass over the bands (the tile is in L1 by
//            then), its quantised values; the four pixels of a lane are summed in registers first where they chose the same cluster.
//            1024 pixels x 65535 < 2^26: the 32-bit counters cannot overflow.  The table goes to `sums` once per tile with 64-bit integer
//            atomics, the coordinate sums corrected by count x origin, rows without a pixel skipped.
//   centres: the rounded means (2 sum + n) / (2 n), one thread per entry.
// Integers only: integer addition is associative, so sums, centres and labels do not depend on the launch geometry or on the order in
// which the adds arrive.  `centres` is written by one launch and read by the next, behind a kernel boundary: plain loads.  No workgroup
// waits for another one.
#include "eae_internal.h"
#include "eae_common.hip.h"

namespace {

constexpr int SL_NT = 256;                 // threads per workgroup: 4 waves
constexpr int SL_TH = 16, SL_TW = 64;      // the tile: 4 rows per wave, one column per lane
constexpr int SL_ROWS = SL_TH / 4;         // rows of a wave
constexpr int SL_MAX_C = 16;
constexpr int SL_MIN_STEP = 2, SL_MAX_STEP = 256;
constexpr long long SL_MAX_WEIGHT = 1LL << 40;

typedef unsigned long long u64;
typedef __attribute__((address_space(3))) unsigned lds_u32;
typedef __attribute__((address_space(3))) int lds_i32;
// builtins, not atomicAdd() / __syncthreads(): the library functions lack the kernel's EAE_NO_PK target attribute and would stay calls
__device__ __forceinline__ void lds_add(lds_u32* p, unsigned v) { __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void glb_add(u64* p, u64 v) { __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void wg_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// u = rint(65535 * min(max(v / d, 0), 1)) in double, round-half-even; NaN -> 0 (the first comparison is false: zonal_q's order).  The
// division of two doubles is correctly rounded, so this is the NumPy expression of the header bit for bit.
template <typename T> __device__ __forceinline__ unsigned slic_q_exact(T v, double d) {
  const double p = (double)v / d;
  const double c = p > 0.0 ? (p < 1.0 ? p : 1.0) : 0.0;
  return (unsigned)(int)__builtin_rint(c * 65535.0);
}
// The same integer without a division per element: rd = 1 / d (correctly rounded, once per band and workgroup) makes v * rd equal to
// v / d to within 2 ulp, with the same sign, zeros, infinities and NaNs (d and rd are never subnormal doubles: d comes from a float),
// so 65535 times the clamped value lies within 1e-10 of the exact product.  The two round to different integers only where the
// product is that close to a half-integer; within 1e-6 of one the division is made.  Next to the clamps both forms give 0 or 65535.
template <typename T> __device__ __forceinline__ unsigned slic_q(T v, double d, double rd) {
  const double p = (double)v * rd;
  const double c = p > 0.0 ? (p < 1.0 ? p : 1.0) : 0.0;
  const double t = c * 65535.0, r = __builtin_rint(t);
  if (__builtin_fabs(__builtin_fabs(t - r) - 0.5) < 1e-6) return slic_q_exact(v, d);
  return (unsigned)(int)r;
}

// a * b for a < 2^24 and b < 2^56 whose product fits 64 bits: one 32 x 32 -> 64 multiply-add and one 24-bit multiply (the masks tell
// the compiler the operand widths; a generic 64 x 64 product is three quarter-rate multiplies)
__device__ __forceinline__ u64 mul_24x56(unsigned a, u64 b) {
  return (u64)a * (unsigned)b + ((u64)((a & 0xffffffu) * ((unsigned)(b >> 32) & 0xffffffu)) << 32);
}

// the cells a span of `t` pixels that starts at a multiple of t can overlap, plus one ring, clipped to the grid of n cells
__host__ __device__ inline int slic_span(int t, int step, int n) {
  const int c = (t % step == 0 ? t / step : (t - 1) / step + 2) + 2;
  return c < n ? c : n;
}

template <typename T>
__global__ EAE_NO_PK __launch_bounds__(SL_NT) void slic_step_kernel(const T* __restrict__ data, int C, int H, int W,
                                                                    const float* __restrict__ divisor,
                                                                    const unsigned char* __restrict__ mask, int S, u64 M,
                                                                    const int* __restrict__ centres, int n_h, int n_w, int tilesX,
                                                                    u64* sums, int* labels) {
  extern __shared__ int slic_lds[];                          // centres [nr][RW], then the accumulators [nr][RW]
  __shared__ double rdiv[SL_MAX_C];                          // 1 / divisor
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int RW = C + 3;
  const int ty0 = (int)(blockIdx.x / (unsigned)tilesX) * SL_TH, tx0 = (int)(blockIdx.x % (unsigned)tilesX) * SL_TW;
  const int ty1 = ty0 + SL_TH < H ? ty0 + SL_TH : H, tx1 = tx0 + SL_TW < W ? tx0 + SL_TW : W;       // the tile's end, clipped
  // the cells of the tile and their ring, clipped to the grid: rows of the two tables
  const int ci0 = ty0 / S > 0 ? ty0 / S - 1 : 0, ci1 = (ty1 - 1) / S + 1 < n_h - 1 ? (ty1 - 1) / S + 1 : n_h - 1;
  const int cj0 = tx0 / S > 0 ? tx0 / S - 1 : 0, cj1 = (tx1 - 1) / S + 1 < n_w - 1 ? (tx1 - 1) / S + 1 : n_w - 1;
  const int ncj = cj1 - cj0 + 1, nr = (ci1 - ci0 + 1) * ncj;
  lds_i32* cen = (lds_i32*)slic_lds;
  lds_u32* acc = (lds_u32*)(slic_lds + nr * RW);
  for (int i = tid; i < nr * RW; i += SL_NT) {
    const int row = i / RW, e = i - row * RW;
    const long long k = (long long)(ci0 + row / ncj) * n_w + cj0 + row % ncj;
    cen[i] = centres ? centres[k * RW + e] : 0;
    acc[i] = 0u;
  }
  if (tid < C) rdiv[tid] = 1.0 / (double)divisor[tid];
  wg_barrier();
  const long long plane = (long long)H * W;
  const unsigned S2 = (unsigned)(S * S);
  const int x = tx0 + lane;
  const int hj = x / S;                                      // the home cell's column (x < W where it is used)
  int lab[SL_ROWS];                                          // the table row each of the lane's pixels chose; -1: none
#pragma unroll
  for (int r = 0; r < SL_ROWS; ++r) {
    const int y = ty0 + wave * SL_ROWS + r;
    lab[r] = -1;
    const bool in = y < H && x < W;
    const long long px = (long long)y * W + x;
    if (in && !(mask && mask[px])) {
      const int hi = y / S;
      if (!centres) {
        lab[r] = (hi - ci0) * ncj + (hj - cj0);              // iteration 0: the home cluster
      } else {
        int trow[9];                                         // the candidates' table rows in ascending cluster id; -1: none
        u64 dc[9];
#pragma unroll
        for (int q = 0; q < 9; ++q) {
          const int i = hi + q / 3 - 1, j = hj + q % 3 - 1;
          const bool ok = i >= 0 && i < n_h && j >= 0 && j < n_w;
          const int t = ok ? (i - ci0) * ncj + (j - cj0) : 0;
          trow[q] = ok && cen[t * RW] > 0 ? t : -1;
          dc[q] = 0;
        }
        for (int c = 0; c < C; ++c) {
          const unsigned u = slic_q(data[c * plane + px], (double)divisor[c], rdiv[c]);
#pragma unroll
          for (int q = 0; q < 9; ++q) {
            const int mu = cen[(trow[q] < 0 ? 0 : trow[q]) * RW + 3 + c];
            const unsigned d = (unsigned)((int)u > mu ? (int)u - mu : mu - (int)u) & 0xffffu;      // <= 65535: a 24-bit multiply
            dc[q] += d * d;
          }
        }
        u64 best = ~0ull;
#pragma unroll
        for (int q = 0; q < 9; ++q) {
          if (trow[q] < 0) continue;
          const int cy = cen[trow[q] * RW + 1], cx = cen[trow[q] * RW + 2];
          // |y - cy|, |x - cx| < 3 S <= 768 (a cluster only holds pixels of the cells around its own): 24-bit multiplies
          const unsigned ay = (unsigned)(y > cy ? y - cy : cy - y) & 0xffffu, ax = (unsigned)(x > cx ? x - cx : cx - x) & 0xffffu;
          // below 2^63: S^2 * colour <= 2^16 * 16 * 2^32, and the second term is at most 18 * 2^16 * 2^40
          const u64 D = mul_24x56(S2, dc[q]) + mul_24x56(ay * ay + ax * ax, M);
          if (D < best) { best = D; lab[r] = trow[q]; }      // strict: the lowest cluster id keeps a tie
        }
      }
    }
    if (labels && in) {
      // the wave's 64 labels of this row: 256 consecutive bytes through a buffer window of the row's part of the tile
      OutRsrc o;
      o.init(labels + (long long)__builtin_amdgcn_readfirstlane(y) * W + tx0, (long)(tx1 - tx0) * 4);
      const int t = lab[r];
      const int k = t < 0 ? -1 : (ci0 + t / ncj) * n_w + cj0 + t % ncj;
      o.st4<EAE_WT_SLIC>((uint32_t)lane * 4u, (uint32_t)k);
    }
  }
  // the lane's pixels into the table: count, y and x relative to the tile's origin; consecutive rows of one cluster are summed first
  {
    int open = -1;
    unsigned n = 0, sy = 0;
#pragma unroll
    for (int r = 0; r <= SL_ROWS; ++r) {
      const int t = r < SL_ROWS ? lab[r] : -1;
      if (t != open || r == SL_ROWS) {
        if (open >= 0) {
          lds_add(acc + open * RW, n);
          lds_add(acc + open * RW + 1, sy);
          lds_add(acc + open * RW + 2, n * (unsigned)lane);
        }
        open = t; n = 0; sy = 0;
      }
      ++n;
      sy += (unsigned)(wave * SL_ROWS + r);
    }
  }
  // the quantised values, band by band (the tile's elements are read a second time: they are in L1)
  for (int c = 0; c < C; ++c) {
    const double d = (double)divisor[c], rd = rdiv[c];
    int open = -1;
    unsigned su = 0;
#pragma unroll
    for (int r = 0; r <= SL_ROWS; ++r) {
      const int t = r < SL_ROWS ? lab[r] : -1;
      if (t != open || r == SL_ROWS) {
        if (open >= 0 && su) lds_add(acc + open * RW + 3 + c, su);
        open = t; su = 0;
      }
      if (t >= 0) su += slic_q(data[c * plane + (long long)(ty0 + wave * SL_ROWS + r) * W + x], d, rd);
    }
  }
  wg_barrier();
  // the table to global memory: consecutive threads take consecutive counters of a row; a row without a pixel is skipped
  for (int i = tid; i < nr * RW; i += SL_NT) {
    const int row = i / RW, e = i - row * RW;
    const u64 n = acc[row * RW];
    if (!n) continue;
    u64 v = acc[i];
    if (e == 1) v += n * (u64)ty0;
    if (e == 2) v += n * (u64)tx0;
    if (!v) continue;
    const long long k = (long long)(ci0 + row / ncj) * n_w + cj0 + row % ncj;
    glb_add(sums + k * RW + e, v);
  }
}

// centres[k][0] = count, centres[k][e] = (2 sums[k][e] + n) / (2 n), all zeros for an empty cluster
__global__ __launch_bounds__(SL_NT) void slic_centres_kernel(const long long* __restrict__ sums, long long n_entries, int RW,
                                                             int* __restrict__ centres) {
  const long long i = (long long)blockIdx.x * SL_NT + threadIdx.x;
  if (i >= n_entries) return;
  const long long k = i / RW;
  const int e = (int)(i - k * RW);
  const long long n = sums[k * RW];
  centres[i] = e == 0 ? (int)n : n > 0 ? (int)((2 * sums[i] + n) / (2 * n)) : 0;
}

int slic_fail(const char* who, const char* what) {
  static thread_local char msg[200];
  snprintf(msg, sizeof msg, "%s: %s", who, what);
  return eae_set_error(EAE_ERR_ARG, msg);
}

}  // namespace

extern "C" int eae_slic_step(void* stream, const void* data, int dtype, int C, int H, int W, const float* divisor,
                             const unsigned char* mask, int step, long long spatial_weight, const int* centres_in, long long* sums_out,
                             int* labels_out) {
  const char* who = "slic_step";
  if (!data || !divisor || !sums_out) return slic_fail(who, "NULL data, divisor or sums_out");
  if (dtype != EAE_SCENE_U8 && dtype != EAE_SCENE_U16 && dtype != EAE_SCENE_F32) return slic_fail(who, "unknown dtype");
  const int eb = dtype == EAE_SCENE_U8 ? 1 : dtype == EAE_SCENE_U16 ? 2 : 4;
  if (reinterpret_cast<uintptr_t>(data) % (unsigned)eb) return slic_fail(who, "the data pointer is not aligned to its element size");
  if (C < 1 || C > SL_MAX_C) return slic_fail(who, "the number of bands must be in 1..16");
  if (H < 1 || W < 1) return slic_fail(who, "empty raster");
  if ((long long)H * W >= (1LL << 31)) return slic_fail(who, "H * W must be below 2^31");
  if (step < SL_MIN_STEP || step > SL_MAX_STEP) return slic_fail(who, "the step must be in 2..256");
  if (spatial_weight < 0 || spatial_weight > SL_MAX_WEIGHT) return slic_fail(who, "the spatial weight must be in 0..2^40");
  const int n_h = (H + step - 1) / step, n_w = (W + step - 1) / step, RW = C + 3;
  const long long n_cl = (long long)n_h * n_w;
  if (n_cl > 0x7fffffffLL / RW) return slic_fail(who, "the grid is too large: n_h * n_w * (C + 3) must not exceed 2^31 - 1");
  EAE_NO_GROUP("slic_step_kernel");
  const hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(sums_out, 0, (size_t)n_cl * RW * sizeof(long long), st) != hipSuccess)
    return eae_set_error(EAE_ERR_HIP, "slic_step: clearing sums_out failed");
  const int tilesX = (W + SL_TW - 1) / SL_TW, tilesY = (H + SL_TH - 1) / SL_TH;
  // both tables, sized for the tile that overlaps the most cells (step 2, 16 bands: 340 rows, 51680 bytes)
  const size_t lds = (size_t)slic_span(SL_TH, step, n_h) * slic_span(SL_TW, step, n_w) * RW * 2 * sizeof(int);
  const dim3 grid((unsigned)((long long)tilesX * tilesY)), block(SL_NT);
  const u64 M = (u64)spatial_weight;
  if (dtype == EAE_SCENE_U8)
    hipLaunchKernelGGL(slic_step_kernel<unsigned char>, grid, block, lds, st, (const unsigned char*)data, C, H, W, divisor, mask, step, M,
                       centres_in, n_h, n_w, tilesX, (u64*)sums_out, labels_out);
  else if (dtype == EAE_SCENE_U16)
    hipLaunchKernelGGL(slic_step_kernel<unsigned short>, grid, block, lds, st, (const unsigned short*)data, C, H, W, divisor, mask, step,
                       M, centres_in, n_h, n_w, tilesX, (u64*)sums_out, labels_out);
  else
    hipLaunchKernelGGL(slic_step_kernel<float>, grid, block, lds, st, (const float*)data, C, H, W, divisor, mask, step, M, centres_in, n_h,
                       n_w, tilesX, (u64*)sums_out, labels_out);
  EAE_LAUNCH_CHECK();
  return 0;
}

extern "C" int eae_slic_centres(void* stream, const long long* sums, long long n_clusters, int C, int* centres) {
  const char* who = "slic_centres";
  if (!sums || !centres) return slic_fail(who, "NULL sums or centres");
  if (C < 1 || C > SL_MAX_C) return slic_fail(who, "the number of bands must be in 1..16");
  if (n_clusters < 1 || n_clusters > 0x7fffffffLL / (C + 3))
    return slic_fail(who, "n_clusters must be >= 1 and n_clusters * (C + 3) <= 2^31 - 1");
  EAE_NO_GROUP("slic_centres_kernel");
  const long long n = n_clusters * (C + 3);
  hipLaunchKernelGGL(slic_centres_kernel, dim3((unsigned)((n + SL_NT - 1) / SL_NT)), dim3(SL_NT), 0, (hipStream_t)stream, sums, n, C + 3,
                     centres);
  EAE_LAUNCH_CHECK();
  return 0;
}
