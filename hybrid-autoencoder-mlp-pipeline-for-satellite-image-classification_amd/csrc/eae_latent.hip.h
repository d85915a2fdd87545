// What the three units over fp32 latent rows share (eae_cluster.hip: k-means, eae_knn.hip: nearest neighbours, eae_validity.hip:
// class-distance sums): all score row pairs on the f32-input MFMA (v_mfma_f32_32x32x2_f32) as fma(-2, dot, ||row||^2) and take rows
// [rows][L] within the same limits.  eae_knn.hip's distance-tile body is eae_latent_tile.hip.h;
// eae_validity.hip still holds its own copy of that body (DESIGN.md section 31 says why).
#pragma once
#include <hip/hip_runtime.h>

typedef float f32x16 __attribute__((ext_vector_type(16)));   // one 32x32 fp32 accumulator tile, 16 registers a lane

constexpr int LATENT_MAXL = 256;                             // widest latent row a unit takes

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
