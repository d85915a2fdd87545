// What the four units over fp32 latent rows share (eae_cluster.hip: k-means, eae_knn.hip: nearest neighbours, eae_validity.hip:
// class-distance sums, eae_gauss.hip: the Gaussian classifier): all work on the f32-input MFMA (v_mfma_f32_32x32x2_f32), take rows
// [rows][L] within the same limits and launch by the host-side idiom at the end of this file.  The search and the class-distance
// kernel also share eae_latent_tile.hip.h: the first its whole tile body, the second the staging helpers under a tile loop and a row
// loader of its own (DESIGN.md section 31 says why).
#pragma once
#include <type_traits>
#include "eae_internal.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));   // one 32x32 fp32 accumulator tile, 16 registers a lane

constexpr int LATENT_MAXL = 256;                             // widest latent row a unit takes
constexpr int LATENT_MAXK = 256;                             // most centroids or classes

// row of a 32x32 accumulator tile that register `reg` of a lane in half `h` holds (the column is lane & 31)
__device__ __forceinline__ int acc_row(int reg, int h) { return (reg & 3) + 8 * (reg >> 2) + 4 * h; }

// ||row||^2 as one sequential fma chain in ascending l: a function of the row alone, the same in every workgroup and launch geometry
__device__ __forceinline__ float row_sq_chain(const float* p, int L) {
  float s = 0.f;
  for (int l = 0; l < L; ++l) s = __builtin_fmaf(p[l], p[l], s);
  return s;
}

// `row_sq_chain`, NaN unless finite (a row with a NaN or an Inf, or whose squared norm overflows)
__device__ __forceinline__ float row_norm2(const float* p, int L) {
  const float s = row_sq_chain(p, L);
  return s - s == 0.f ? s : __builtin_nanf("");
}

// a [rows][L] operand a unit takes: rows in 1..2^31-1 (a row index fits an int), width in 1..LATENT_MAXL
inline bool latent_dims_ok(long long rows, int L) { return rows >= 1 && rows < 0x80000000LL && L >= 1 && L <= LATENT_MAXL; }
// ... and K centroids or classes over them
inline bool latent_dims_ok(long long N, int L, int K) { return latent_dims_ok(N, L) && K >= 1 && K <= LATENT_MAXK; }

// 16-byte loads of rows [..][L] at p: L % 4 == 0 and an aligned base
inline int latent_vec16(const float* p, int L) { return (L & 3) == 0 && ((uintptr_t)p & 15) == 0; }

// the 32-wide MFMA tiles a kernel is instantiated with to cover n <= 256 centroids or columns: 1, 2, 4 or 8
inline int latent_tiles32(int n) { return n <= 32 ? 1 : n <= 64 ? 2 : n <= 128 ? 4 : 8; }

// f(integral_constant<tiles>) for a count `latent_tiles32` returns: the launch of the instance compiled for it (always inlined: the
// library gains no symbol named after the caller's lambda)
template <class F> __forceinline__ int latent_for_tiles(int tiles, F f) {
  switch (tiles) {
    case 1: return f(std::integral_constant<int, 1>());
    case 2: return f(std::integral_constant<int, 2>());
    case 4: return f(std::integral_constant<int, 4>());
    default: return f(std::integral_constant<int, 8>());
  }
}

// grid of a kernel whose workgroups stride over the tiles of `rows` rows of N: two workgroups on each of 256 CUs at the most
inline unsigned latent_row_tile_grid(long long N, int rows) {
  const long long ntiles = (N + rows - 1) / rows;
  return (unsigned)(ntiles < 512 ? ntiles : 512);
}

// the workspace an entry point was handed against the `need` of its sizing call (0: none is used): 0, or the argument error `msg`
inline int latent_workspace_check(const void* workspace, long long bytes, long long need, const char* msg) {
  return need > 0 && (!workspace || bytes < need) ? eae_set_error(EAE_ERR_ARG, msg) : 0;
}
