// The distance-tile body of eae_knn.hip's search kernel.  eae_validity.hip's class-distance kernel takes the
// constants, the barrier and the staging helpers from here (lds_col, store_rows, stage_scalar, chain64) and keeps a tile loop and a
// row loader of its own until its speed on pair_tile is shown equal (section 31).  A
// workgroup of 4 waves holds 128 queries (wave w owns 32 w .. 32 w + 31 of them) and takes the dot products of one 64-row bank tile
// with them on v_mfma_f32_32x32x2_f32, the BANK rows as the A operand: D[m][n] = b_m . q_n, so a lane owns one query (its column of
// D) and 16 rows of each 32-row half (acc_row).  Both operands pass through LDS, 64 columns a pass; the norms ||b||^2 and ||q||^2 are
// continued from the staged columns.  eae_cluster.hip's assign kernel has another LDS layout and does not use this.
#pragma once
#include "eae_latent.hip.h"

constexpr int LT_NT = 256;          // threads per workgroup: 4 waves
constexpr int LT_QT = 128;          // queries per workgroup tile, 32 per wave
constexpr int LT_BT = 64;           // bank rows per LDS tile: two 32-row MFMA tiles
constexpr int LT_LC = 64;           // columns staged per pass
constexpr int LT_LDS = LT_LC + 4;   // LDS row stride in floats (see lds_col)
constexpr int LT_FLOATS = (LT_QT + LT_BT) * LT_LDS + LT_BT + LT_QT;   // the tile's LDS (TileLds); a kernel's own arrays follow

// __syncthreads() out of builtins: the header's function is not inlined into a kernel that carries a target attribute (EAE_NO_PK), and
// a call inside the tile loop costs the kernel its register allocation
__device__ __forceinline__ void lt_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

struct TileLds {
  float *qs, *bs, *bn, *qn;
  __device__ __forceinline__ explicit TileLds(float* base)
      : qs(base),                    // [128][68]
        bs(qs + LT_QT * LT_LDS),     // [64][68]
        bn(bs + LT_BT * LT_LDS),     // [64]   ||b||^2 of the tile's rows (pair_tile's MASK_BN: NaN for a row that cannot be used)
        qn(bn + LT_BT) {}            // [128]  ||q||^2 of a finite query; the kernel presets it to NaN
};

struct TileSrc {
  const float* q; const float* bank; long long Nq; int L;
  int qvec, bvec;                   // 16-byte loads of q / bank: L % 4 == 0 and an aligned base
};
inline TileSrc tile_src(const float* q, long long Nq, const float* bank, int L) {
  return {q, bank, Nq, L, latent_vec16(q, L), latent_vec16(bank, L)};
}

// A staged row holds 64 columns de-interleaved: the 32 even columns, then the 32 odd ones (then 4 floats of padding).  Lane (r, h) of
// an MFMA step takes column 2 j + h, so a lane's operands of four consecutive steps are one 16-byte LDS read; at a row stride of 68
// floats the 16 lanes a ds_read_b128 serves together (16 different rows) cover the 64 banks once.
__device__ __forceinline__ int lds_col(int col) { return (col & 1) * 32 + (col >> 1); }

// rows [row0, row0 + 16 N) x columns [l0, l0 + 64) of src [..][L] into registers with 16-byte loads (L % 4 == 0 and an aligned
// base), zero from row `nrows` on and beyond L: no row at or past nrows is read.  row0 is uniform over the workgroup, so the 64-bit
// product row0 * L is taken once, off the vector unit; a row adds a 32-bit row * L (row < 128, L <= 256).  `first` is only an
// address: it is formed whatever row0 is and dereferenced under the row guard alone.
template <int N>
__device__ __forceinline__ void load_rows(float4 (&v)[N], const float* src, long long row0, long long nrows, int L, int l0, int lw, int tid) {
  const float* first = src + (size_t)row0 * L + l0;
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const int e = tid + LT_NT * i, row = e >> 4, col = (e & 15) * 4;
    v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row0 + row < nrows && col < lw) v[i] = *reinterpret_cast<const float4*>(first + row * L + col);
  }
}

// ... and from the registers into dst [16 N][68]
template <int N>
__device__ __forceinline__ void store_rows(float* dst, const float4 (&v)[N], int tid) {
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const int e = tid + LT_NT * i, row = e >> 4, col = (e & 15) * 4;
    float* d = dst + row * LT_LDS + (col >> 1);
    *reinterpret_cast<float2*>(d) = make_float2(v[i].x, v[i].z);
    *reinterpret_cast<float2*>(d + 32) = make_float2(v[i].y, v[i].w);
  }
}

// the same rows straight into dst, float by float: any L, any alignment
template <int ROWS>
__device__ __forceinline__ void stage_scalar(float* dst, const float* src, long long row0, long long nrows, int L, int l0, int lw, int tid) {
#pragma unroll 4
  for (int i = 0; i < ROWS * LT_LC / LT_NT; ++i) {
    const int e = tid + LT_NT * i, row = e >> 6, col = e & 63;
    float v = 0.f;
    if (row0 + row < nrows && col < lw) v = src[(size_t)(row0 + row) * L + l0 + col];
    dst[row * LT_LDS + lds_col(col)] = v;
  }
}

// s continued over the 64 staged columns of a row in ascending column order: row_sq_chain's order (the zeros beyond L change
// nothing: fma(0, 0, s) = s)
__device__ __forceinline__ float chain64(const float* row, float s) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float4 e = *reinterpret_cast<const float4*>(row + 4 * j), o = *reinterpret_cast<const float4*>(row + 32 + 4 * j);
    s = __builtin_fmaf(e.x, e.x, s); s = __builtin_fmaf(o.x, o.x, s);
    s = __builtin_fmaf(e.y, e.y, s); s = __builtin_fmaf(o.y, o.y, s);
    s = __builtin_fmaf(e.z, e.z, s); s = __builtin_fmaf(o.z, o.z, s);
    s = __builtin_fmaf(e.w, e.w, s); s = __builtin_fmaf(o.w, o.w, s);
  }
  return s;
}

// the first pass of the workgroup's first tile into the prefetch registers (16-byte loads only: nothing without bvec)
__device__ __forceinline__ void tile_prefetch(float4 (&pre)[LT_BT / 16], const TileSrc& a, long long m0, long long me, int tid) {
  if (a.bvec) load_rows(pre, a.bank, m0, me, a.L, 0, a.L < LT_LC ? a.L : LT_LC, tid);
}

// One bank tile, rows [m0, m0 + 64) cut at `me`, against queries n0 .. n0 + 127: acc = the lane's 2 x 16 dot products.  The columns
// are walked in passes of 64: the bank tile's columns are staged in LDS (and the queries' too -- once per workgroup, in its `first`
// tile, when L <= 64); the coming pass's bank columns -- this tile's next, or the first of the tile at `m_next`, if that is below
// `me` -- are loaded into `pre` before this pass's MFMAs and written to LDS after them (`pre` comes in holding this tile's first
// pass).  Wave 0 continues ||b||^2 of the tile's rows from the staged columns (thread = row, ascending l: the chain does not depend
// on the pass width) into bn, raw or with MASK_BN NaN for a row at or past `me` or not finite; waves 0 and 1 do the same for
// ||q||^2 (`qnrm`, kept by the caller across the passes) during the first tile and set qn of a finite query; every `busy` wave (one
// that has a query) runs one MFMA per 32-row half and pair of columns.  Ends with the barrier that completes bn and qn.
template <bool MASK_BN>
__device__ __forceinline__ void pair_tile(f32x16 (&acc)[2], float4 (&pre)[LT_BT / 16], float& qnrm, const TileSrc& a, const TileLds& s,
                                          long long n0, long long m0, long long me, long long m_next, bool first, bool busy, int tid) {
  const int lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5, qrow = wave * 32 + r;
  const int L = a.L, npass = (L + LT_LC - 1) / LT_LC;
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[t][i] = 0.f;
  float nrm = 0.f;                                             // wave 0: thread = bank row of the tile

  for (int p = 0; p < npass; ++p) {
    const int l0 = p * LT_LC;
    const int lw = L - l0 < LT_LC ? L - l0 : LT_LC;            // real columns of this pass
    lt_barrier();                                              // the previous pass (or tile, or the set-up) is done with the LDS
    const bool newq = npass > 1 || first;
    if (newq && a.qvec) {
      float4 qv[LT_QT / 16];
      load_rows(qv, a.q, n0, a.Nq, L, l0, lw, tid);
      store_rows(s.qs, qv, tid);
    } else if (newq) {
      stage_scalar<LT_QT>(s.qs, a.q, n0, a.Nq, L, l0, lw, tid);
    }
    if (a.bvec) store_rows(s.bs, pre, tid);
    else stage_scalar<LT_BT>(s.bs, a.bank, m0, me, L, l0, lw, tid);
    lt_barrier();
    if (a.bvec) {                                              // the coming pass: the next columns, or the next tile's first
      const long long m1 = p + 1 < npass ? m0 : m_next;
      const int l1 = p + 1 < npass ? l0 + LT_LC : 0;
      if (m1 < me) load_rows(pre, a.bank, m1, me, L, l1, L - l1 < LT_LC ? L - l1 : LT_LC, tid);
    }
    if (wave == 0) {
      nrm = chain64(s.bs + lane * LT_LDS, nrm);
      if (p == npass - 1) s.bn[lane] = (!MASK_BN || (m0 + lane < me && nrm - nrm == 0.f)) ? nrm : __builtin_nanf("");
    }
    if (first && tid < LT_QT) {
      qnrm = chain64(s.qs + tid * LT_LDS, qnrm);
      if (p == npass - 1 && n0 + tid < a.Nq && qnrm - qnrm == 0.f) s.qn[tid] = qnrm;
    }
    if (busy) {
      const float* zrow = s.qs + qrow * LT_LDS + h * 32;
      const float* crow = s.bs + r * LT_LDS + h * 32;
      const int nj = ((lw + 1) / 2 + 3) >> 2;                  // groups of four column pairs; the last one may run into the zeros
      // the next group's operands are read while this group's MFMAs run (the read after the last group stays inside the row)
      float4 nb = *reinterpret_cast<const float4*>(zrow);
      float4 na0 = *reinterpret_cast<const float4*>(crow);
      float4 na1 = *reinterpret_cast<const float4*>(crow + 32 * LT_LDS);
      for (int j = 0; j < nj; ++j) {
        const float4 b = nb, a0 = na0, a1 = na1;
        nb = *reinterpret_cast<const float4*>(zrow + 4 * j + 4);
        na0 = *reinterpret_cast<const float4*>(crow + 4 * j + 4);
        na1 = *reinterpret_cast<const float4*>(crow + 32 * LT_LDS + 4 * j + 4);
        acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.x, b.x, acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.x, b.x, acc[1], 0, 0, 0);
        acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.y, b.y, acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.y, b.y, acc[1], 0, 0, 0);
        acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.z, b.z, acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.z, b.z, acc[1], 0, 0, 0);
        acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.w, b.w, acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.w, b.w, acc[1], 0, 0, 0);
      }
    }
  }
  lt_barrier();                                                // bn (and, in the first tile, qn) is complete
}
