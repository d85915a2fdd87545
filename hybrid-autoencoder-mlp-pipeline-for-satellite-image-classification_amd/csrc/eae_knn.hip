// Latent neighbours (include/eae.h, "latent neighbours"): the k nearest bank rows of every query row, both fp32,
// scored in exact fp32 on the f32-input MFMA (v_mfma_f32_32x32x2_f32: a k-ordered fma chain) as eae_kmeans_assign scores centroids:
//   score(n, m) = fma(-2, q_n . b_m, ||b_m||^2), the norm a sequential fma chain -- a function of the two rows alone.
//   search: the bank streams through eae_latent_tile.hip.h's tile body in 64-row tiles (a lane owns one query); every query keeps a
//           list of its k best (score, row) pairs, sorted by that pair, in LDS, and a lane touches it only for a score that beats the
//           list's last entry.  No Nq x M array is written.
//   merge:  with few queries the bank is cut into S slices, one workgroup per (query tile, slice) writes its list to the caller's
//           workspace, and a second kernel merges the S sorted lists of a query by the same order.  The order is total (a bank row
//           appears once), so the result is bitwise the same for every S.
// Outputs are written with plain vector stores (store policy 0 of eae_store_policy.h: no family of this file has an A/B that
// showed write-through to gain).  No float atomics.
#include "eae_internal.h"
#include "eae_common.hip.h"
#include "eae_latent_tile.hip.h"

namespace {

constexpr int KN_MAXK = 32;
constexpr int KN_MAXS = 512;        // most bank slices
constexpr int KN_EMPTY = 0x7fffffff;    // row of an empty list slot: (+Inf, KN_EMPTY) is the greatest pair

// (s, m) < (ps, pm), lexicographic; false when s is a NaN.  Without short-circuit branches: it sits in unrolled code.
__device__ __forceinline__ bool pair_less(float s, int m, float ps, int pm) { return (s < ps) | ((s == ps) & (m < pm)); }

struct SearchArgs {
  TileSrc src; long long M; int k; long long self_offset;
  long long* idx; float* dist;      // S == 1: the outputs
  int2* part;                       // S > 1: [S][Nq][k] (score bits, row)
  long long rows_per_slice;         // a multiple of LT_BT
};

// ---------------------------------------------------------------------------------------------------------------
// search.  Workgroup (tile, slice): queries 128 tile .. + 127 (wave w owns 32 w .. 32 w + 31 of them) against the bank rows of the
// slice, in 64-row tiles (pair_tile).  After a tile a lane holds 32 dot products, then scores, of its query; the two lanes of a query
// take turns (h = 0, then h = 1) at the query's list.  A bank row that is not finite, lies beyond the slice or is the query's
// excluded row scores NaN and never enters a list.
// ---------------------------------------------------------------------------------------------------------------
__global__ EAE_NO_PK __launch_bounds__(LT_NT, 2) void knn_search_kernel(SearchArgs a) {
  extern __shared__ __attribute__((aligned(16))) float kn_lds[];
  const TileLds lds(kn_lds);                           // bn: NaN for a row that cannot be returned (pair_tile<true>)
  float* qn = lds.qn;
  const float* bn = lds.bn;
  float* ls = kn_lds + LT_FLOATS;                      // [128][k] list scores, ascending
  int* li = reinterpret_cast<int*>(ls + LT_QT * a.k);  // [128][k] list rows
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
  const int k = a.k;
  const long long Nq = a.src.Nq;
  const long long n0 = (long long)blockIdx.x * LT_QT;
  const long long mb = (long long)blockIdx.y * a.rows_per_slice;
  const long long me = mb + a.rows_per_slice < a.M ? mb + a.rows_per_slice : a.M;

  for (int e = tid; e < LT_QT * k; e += LT_NT) { ls[e] = __builtin_inff(); li[e] = KN_EMPTY; }
  if (tid < LT_QT) qn[tid] = __builtin_nanf("");
  lt_barrier();

  const int qrow = wave * 32 + r;
  const long long n = n0 + qrow;
  const long long excl = a.self_offset >= 0 ? n + a.self_offset : -1;
  const bool busy = n0 + wave * 32 < Nq;                       // the wave has a query
  float* myls = ls + qrow * k;
  int* myli = li + qrow * k;
  float qnrm = 0.f;                                            // waves 0 and 1: thread = query of the tile
  float4 pre[LT_BT / 16];                                      // the bank columns of the coming pass
  tile_prefetch(pre, a.src, mb, me, tid);

  for (long long m0 = mb; m0 < me; m0 += LT_BT) {
    f32x16 acc[2];                                             // the tile's dot products, then its scores
    pair_tile<true>(acc, pre, qnrm, a.src, lds, n0, m0, me, m0 + LT_BT, m0 == mb, busy, tid);
    if (!busy) continue;

    // The lane's 32 scores of this tile.  Bit c = 16 t + i of `cand`: score c beats the last entry of the query's list as it stands
    // before this tile (the entry only falls: a superset of what will enter).  Then the two lanes of a query take turns at the list,
    // h = 0 first (one wave: its LDS accesses stay in order).
    const int mi0 = (int)m0;                                   // m0 + row < M < 2^31 wherever bn[row] is a number
    const int erow = excl >= m0 && excl < m0 + LT_BT ? (int)(excl - m0) : -1;
    unsigned cand = 0;
    {
      const float thr = myls[k - 1];
      const int thi = myli[k - 1];
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int row = t * 32 + acc_row(i, h);
          acc[t][i] = __builtin_fmaf(-2.f, acc[t][i], bn[row]);
          if (pair_less(acc[t][i], (int)((unsigned)mi0 + row), thr, thi) && row != erow) cand |= 1u << (t * 16 + i);
        }
    }
    for (int hh = 0; hh < 2; ++hh) {
      if (h == hh && cand) {
        float thr = myls[k - 1];
        int thi = myli[k - 1];
        while (cand) {                                         // one copy of the insertion for all 32 registers
          const int c = __builtin_ctz(cand);
          cand &= cand - 1;
          const f32x16 half = c & 16 ? acc[1] : acc[0];
          float s = half[0];
#pragma unroll
          for (int i = 1; i < 16; ++i) s = (c & 15) == i ? half[i] : s;
          const int m = (int)((unsigned)mi0 + (c >> 4) * 32 + acc_row(c & 15, h));
          if (!pair_less(s, m, thr, thi)) continue;
          int j = k - 1;
          while (j > 0) {
            const float ps = myls[j - 1];
            const int pm = myli[j - 1];
            if (pair_less(ps, pm, s, m)) break;
            myls[j] = ps; myli[j] = pm;
            --j;
          }
          myls[j] = s; myli[j] = m;
          thr = myls[k - 1]; thi = myli[k - 1];
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
      __builtin_amdgcn_wave_barrier();
    }
  }

  // the wave's 32 lists are 32 k consecutive entries of the output (or of the slice's partial): lanes stride over them
  for (int e = lane; e < 32 * k; e += 64) {
    const int qq = e / k, j = e - qq * k, lrow = wave * 32 + qq;
    const long long nn = n0 + lrow;
    if (nn >= Nq) continue;
    const float s = ls[lrow * k + j];
    const int m = li[lrow * k + j];
    if (a.part) {
      int2 e;
      e.x = __builtin_bit_cast(int, s); e.y = m;
      a.part[((size_t)blockIdx.y * Nq + nn) * k + j] = e;
    } else {
      const float nq = qn[lrow];
      const bool none = m == KN_EMPTY || !(nq == nq);
      a.idx[(size_t)nn * k + j] = none ? -1 : (long long)m;
      if (a.dist) a.dist[(size_t)nn * k + j] = none ? __builtin_nanf("") : fmaxf(s + nq, 0.f);
    }
  }
}

// merge: workgroup n (one wave) merges the S sorted lists of query n.  Lane x looks after slices x, x + 64, ...; every round each lane
// takes the least head among its slices, a butterfly makes the least of all known to every lane, and the slice it came from advances.
struct MergeArgs { const float* q; long long Nq; int L, k, S; const int2* part; long long* idx; float* dist; };

__global__ EAE_NO_PK __launch_bounds__(64) void knn_merge_kernel(MergeArgs a) {
  __shared__ int head[KN_MAXS];
  __shared__ float qnorm;
  const int lane = threadIdx.x, k = a.k, S = a.S;
  const long long n = blockIdx.x;
  for (int s = lane; s < S; s += 64) head[s] = 0;
  if (lane == 0) qnorm = row_norm2(a.q + (size_t)n * a.L, a.L);
  lt_barrier();
  const float nq = qnorm;
  const bool bad = !(nq == nq);
  for (int j = 0; j < k; ++j) {
    float bsc = __builtin_inff();
    int bm = KN_EMPTY, bsl = -1;
    for (int s = lane; s < S; s += 64) {
      const int p = head[s];
      if (p < k) {
        const int2 e = a.part[((size_t)s * a.Nq + n) * k + p];
        const float sc = __builtin_bit_cast(float, e.x);
        if (pair_less(sc, e.y, bsc, bm)) { bsc = sc; bm = e.y; bsl = s; }
      }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      const float osc = __shfl_xor(bsc, d, 64);
      const int om = __shfl_xor(bm, d, 64), osl = __shfl_xor(bsl, d, 64);
      if (pair_less(osc, om, bsc, bm)) { bsc = osc; bm = om; bsl = osl; }
    }
    if (bsl >= 0 && (bsl & 63) == lane) head[bsl] += 1;
    if (lane == 0) {
      const bool none = bad || bsl < 0;
      a.idx[(size_t)n * k + j] = none ? -1 : (long long)bm;
      if (a.dist) a.dist[(size_t)n * k + j] = none ? __builtin_nanf("") : fmaxf(bsc + nq, 0.f);
    }
    lt_barrier();
  }
}

int knn_dims_ok(long long Nq, long long M, int L, int k) {
  return latent_dims_ok(Nq, L) && latent_dims_ok(M, L) && k >= 1 && k <= KN_MAXK;
}

// The geometry, a function of (Nq, M) alone.  With 256 query tiles or more (two workgroups' worth of a 256-CU device at k <= 19, one
// round at greater k) the bank is not cut.  Below that it is cut into as many slices as bring the grid to 512 workgroups, of at least
// four 64-row bank tiles each, and never more than 512.
struct KnnPlan { long long tiles, rows_per_slice; int S; };
KnnPlan knn_plan(long long Nq, long long M) {
  KnnPlan p;
  p.tiles = (Nq + LT_QT - 1) / LT_QT;
  const long long nb = (M + LT_BT - 1) / LT_BT;
  long long want = p.tiles >= 256 ? 1 : 512 / p.tiles;
  const long long most = (nb + 3) / 4;
  if (want > most) want = most;
  if (want > KN_MAXS) want = KN_MAXS;
  if (want < 1) want = 1;
  const long long tps = (nb + want - 1) / want;                // bank tiles per slice
  p.S = (int)((nb + tps - 1) / tps);                           // no slice is empty
  p.rows_per_slice = tps * LT_BT;
  return p;
}

long long knn_ws_bytes(const KnnPlan& p, long long Nq, int k) { return p.S > 1 ? (long long)p.S * Nq * k * (long long)sizeof(int2) : 0; }

}  // namespace

extern "C" long long eae_knn_workspace_bytes(long long Nq, long long M, int L, int k) {
  if (!knn_dims_ok(Nq, M, L, k)) return eae_set_error(EAE_ERR_ARG, "knn: Nq and M must be in 1..2^31-1, L in 1..256, k in 1..32");
  return knn_ws_bytes(knn_plan(Nq, M), Nq, k);
}

extern "C" int eae_knn_slices(long long Nq, long long M, int L, int k) {
  if (!knn_dims_ok(Nq, M, L, k)) return eae_set_error(EAE_ERR_ARG, "knn: Nq and M must be in 1..2^31-1, L in 1..256, k in 1..32");
  return knn_plan(Nq, M).S;
}

extern "C" int eae_knn_search(void* stream, const float* q, long long Nq, const float* bank, long long M, int L, int k,
                              long long self_offset, long long* idx, float* dist, void* workspace, long long workspace_bytes) {
  if (!knn_dims_ok(Nq, M, L, k)) return eae_set_error(EAE_ERR_ARG, "knn_search: Nq and M must be in 1..2^31-1, L in 1..256, k in 1..32");
  if (!q || !bank || !idx) return eae_set_error(EAE_ERR_ARG, "knn_search: NULL q, bank or idx");
  if (self_offset < -1) return eae_set_error(EAE_ERR_ARG, "knn_search: self_offset must be -1 (off) or >= 0");
  const KnnPlan p = knn_plan(Nq, M);
  if (const int rc = latent_workspace_check(workspace, workspace_bytes, knn_ws_bytes(p, Nq, k),
                                            "knn_search: the workspace is NULL or smaller than eae_knn_workspace_bytes")) return rc;
  EAE_NO_GROUP("knn_search_kernel");
  const hipStream_t st = (hipStream_t)stream;
  const SearchArgs a = {tile_src(q, Nq, bank, L), M, k, self_offset, idx, dist, p.S > 1 ? (int2*)workspace : nullptr, p.rows_per_slice};
  const size_t lds = ((size_t)LT_FLOATS + (size_t)LT_QT * k * 2) * sizeof(float);
  EAE_HIP(eae_smem_attr((const void*)knn_search_kernel, (size_t)(LT_FLOATS + LT_QT * KN_MAXK * 2) * sizeof(float)));
  hipLaunchKernelGGL(knn_search_kernel, dim3((unsigned)p.tiles, (unsigned)p.S), dim3(LT_NT), lds, st, a);
  EAE_LAUNCH_CHECK();
  if (p.S > 1) {
    const MergeArgs g = {q, Nq, L, k, p.S, (const int2*)workspace, idx, dist};
    hipLaunchKernelGGL(knn_merge_kernel, dim3((unsigned)Nq), dim3(64), 0, st, g);
    EAE_LAUNCH_CHECK();
  }
  return 0;
}
