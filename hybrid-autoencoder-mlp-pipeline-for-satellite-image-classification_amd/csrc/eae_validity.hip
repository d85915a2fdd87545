// Latent validity (include/eae.h, "latent validity"): for every query row the sum of its distances to the bank
// rows of each class, both fp32, the bank sorted by class -- what a silhouette and a class-separation table are made of.  One of the
// four units of eae_latent.hip.h; its body is eae_knn.hip's search kernel without the selection, on eae_latent_tile.hip.h's constants,
// barrier and staging helpers, with the tile loop and the row loader written out here:
//   d^2(n, m) = max(0, fma(-2, q_n . b_m, ||b_m||^2) + ||q_n||^2), the dot product on v_mfma_f32_32x32x2_f32 with the BANK rows as
//   the A operand (a lane owns one query, its column of D, and 16 rows of a 32-row tile), the norms sequential fma chains.
//   sums: workgroup (query tile, class, slice) walks the 64-row tiles slice, slice + S, ... of its class's segment; a lane adds its
//         32 distances of a tile into one fp32 accumulator in register order, rows beyond the segment's end and the query's own row
//         masked to 0; the two lanes of a query are added once, at the end.  No Nq x M array is written.
//   add:  with S > 1 the partial sums go to the caller's workspace [S][Nq][K] and a second kernel adds them in ascending slice order.
// Every sum has one owner and one fixed order: the result is bitwise the same from run to run.  Outputs are written with plain vector
// stores (store policy 0 of eae_store_policy.h).  No float atomics.
#include "eae_internal.h"
#include "eae_common.hip.h"
#include "eae_latent_tile.hip.h"

namespace {

constexpr int CD_MAXS = 64;         // most slices of a segment

struct SumArgs {
  const float* q; const float* bank; long long Nq, M; int L, K, S, metric;
  const long long* seg; const long long* self_pos;
  float* out;                       // S == 1: sums [Nq][K]; S > 1: the partials [S][Nq][K]
  int qvec, bvec;                   // 16-byte loads of q / bank: L % 4 == 0 and an aligned base
};

// The header's load_rows with the address as this kernel has always formed it, (row0 + row) * L in 64 bits for every load: the one
// part of the tile body whose instructions differ between the two kernels
template <int N>
__device__ __forceinline__ void cd_load_rows(float4 (&v)[N], const float* src, long long row0, long long nrows, int L, int l0, int lw, int tid) {
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const int e = tid + LT_NT * i, row = e >> 4, col = (e & 15) * 4;
    v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row0 + row < nrows && col < lw) v[i] = *reinterpret_cast<const float4*>(src + (size_t)(row0 + row) * L + l0 + col);
  }
}

// ---------------------------------------------------------------------------------------------------------------
// sums.  Workgroup (tile, class, slice): queries 128 tile .. + 127 (wave w owns 32 w .. 32 w + 31 of them) against rows
// [seg[c], seg[c+1]) of the bank, the 64-row tiles slice, slice + S, ... counted from the segment's first row.  The staging, the
// passes of 64 columns, the register prefetch of the coming pass, the norms (wave 0: ||b||^2 of the tile's rows, waves 0 and 1:
// ||q||^2 during the first tile) and the MFMA loop are the search kernel's.  After a tile's last pass a lane holds 32 dot products of
// its query; each becomes a distance and is added, in register order, to the lane's running sum.  seg is clamped to [0, M]: whatever
// the device array holds, no row outside the bank is read.  A workgroup without a tile (an empty class, a slice beyond a short
// segment) takes the queries' norms straight from memory -- the same chain -- and writes 0, or NaN for a query that is not finite.
// ---------------------------------------------------------------------------------------------------------------
__global__ EAE_NO_PK __launch_bounds__(LT_NT, 2) void class_dist_kernel(SumArgs a) {
  __shared__ __attribute__((aligned(16))) float cd_lds[LT_FLOATS];
  float* qs = cd_lds;                                  // [128][68]
  float* bs = qs + LT_QT * LT_LDS;                     // [64][68]
  float* bn = bs + LT_BT * LT_LDS;                     // [64]   ||b||^2 of the tile's rows
  float* qn = bn + LT_BT;                              // [128]  ||q||^2, NaN for a query that is not finite (or beyond Nq)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
  const int L = a.L, c = blockIdx.y, S = a.S;
  const long long n0 = (long long)blockIdx.x * LT_QT;
  long long sb = a.seg[c], se = a.seg[c + 1];
  sb = sb < 0 ? 0 : sb;
  se = se > a.M ? a.M : se;
  const long long ntile = se > sb ? (se - sb + LT_BT - 1) / LT_BT : 0;
  const long long t0 = blockIdx.z;
  const int npass = (L + LT_LC - 1) / LT_LC;

  if (tid < LT_QT) qn[tid] = __builtin_nanf("");

  const int qrow = wave * 32 + r;
  const long long n = n0 + qrow;
  const bool busy = n0 + wave * 32 < a.Nq;                     // the wave has a query
  const long long self = (a.self_pos && n < a.Nq) ? a.self_pos[n] : -1;
  float sum = 0.f;

  if (t0 >= ntile) {                                           // nothing to walk (uniform over the workgroup)
    if (tid < LT_QT && n0 + tid < a.Nq) {
      const float s = row_sq_chain(a.q + (size_t)(n0 + tid) * L, L);
      if (s - s == 0.f) qn[tid] = s;
    }
  } else {
    float qnrm = 0.f;                                          // waves 0 and 1: thread = query of the tile
    float4 pre[LT_BT / 16];                                    // the bank columns of the coming pass (16-byte loads only)
    if (a.bvec) cd_load_rows(pre, a.bank, sb + t0 * LT_BT, se, L, 0, L < LT_LC ? L : LT_LC, tid);

    for (long long t = t0; t < ntile; t += S) {
      const long long m0 = sb + t * LT_BT;
      f32x16 acc[2];
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[u][i] = 0.f;
      float nrm = 0.f;                                         // wave 0: thread = bank row of the tile

      for (int p = 0; p < npass; ++p) {
        const int l0 = p * LT_LC;
        const int lw = L - l0 < LT_LC ? L - l0 : LT_LC;        // real columns of this pass
        lt_barrier();                                          // the previous pass (or tile, or the set-up) is done with the LDS
        const bool newq = npass > 1 || t == t0;
        if (newq && a.qvec) {
          float4 qv[LT_QT / 16];
          cd_load_rows(qv, a.q, n0, a.Nq, L, l0, lw, tid);
          store_rows(qs, qv, tid);
        } else if (newq) {
          stage_scalar<LT_QT>(qs, a.q, n0, a.Nq, L, l0, lw, tid);
        }
        if (a.bvec) store_rows(bs, pre, tid);
        else stage_scalar<LT_BT>(bs, a.bank, m0, se, L, l0, lw, tid);
        lt_barrier();
        if (a.bvec) {                                          // the coming pass: the next columns, or the next tile's first
          const long long t1 = p + 1 < npass ? t : t + S;
          const int l1 = p + 1 < npass ? l0 + LT_LC : 0;
          if (t1 < ntile) cd_load_rows(pre, a.bank, sb + t1 * LT_BT, se, L, l1, L - l1 < LT_LC ? L - l1 : LT_LC, tid);
        }
        if (wave == 0) {
          nrm = chain64(bs + lane * LT_LDS, nrm);
          if (p == npass - 1) bn[lane] = nrm;
        }
        if (t == t0 && tid < LT_QT) {
          qnrm = chain64(qs + tid * LT_LDS, qnrm);
          if (p == npass - 1 && n0 + tid < a.Nq && qnrm - qnrm == 0.f) qn[tid] = qnrm;
        }
        if (busy) {
          const float* zrow = qs + qrow * LT_LDS + h * 32;
          const float* crow = bs + r * LT_LDS + h * 32;
          const int nj = ((lw + 1) / 2 + 3) >> 2;              // groups of four column pairs; the last one may run into the zeros
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
      lt_barrier();                                            // bn (and, in the first tile, qn) is complete
      if (!busy) continue;

      // The lane's 32 distances of this tile, added in register order.  Rows from `lim` on lie beyond the segment (staged as zeros)
      // and row `erow` is the query itself: both add 0, by a select, whatever their distance is.
      const long long left = se - m0;
      const int lim = left < LT_BT ? (int)left : LT_BT;
      const int erow = self >= m0 && self < m0 + LT_BT ? (int)(self - m0) : -1;
      const float nq = qn[qrow];
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int row = u * 32 + acc_row(i, h);
          const float d2 = fmaxf(__builtin_fmaf(-2.f, acc[u][i], bn[row]) + nq, 0.f);
          const float d = a.metric ? d2 : __builtin_sqrtf(d2);
          sum += (row < lim && row != erow) ? d : 0.f;
        }
    }
  }
  lt_barrier();                                                // qn is complete on either path

  // lanes r and r + 32 hold the two halves of query 32 wave + r: h = 0 adds them and writes
  const float other = __shfl_xor(sum, 32, 64);
  if (h == 0 && n < a.Nq) {
    const float nq = qn[qrow];
    a.out[((size_t)blockIdx.z * a.Nq + n) * a.K + c] = nq == nq ? sum + other : __builtin_nanf("");
  }
}

// add: sums[e] = part[0][e] + part[1][e] + ... in ascending slice order, one thread per (query, class)
__global__ EAE_NO_PK __launch_bounds__(256) void class_dist_add_kernel(const float* part, long long count, int S, float* sums) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= count) return;
  float s = part[e];
  for (int j = 1; j < S; ++j) s += part[(size_t)j * count + e];
  sums[e] = s;
}

int cd_dims_ok(long long Nq, long long M, int L, int K) {
  return latent_dims_ok(Nq, L, K) && latent_dims_ok(M, L);
}

// The number of slices, a function of (Nq, M) alone (seg is device data: the longest segment the plan can count on is the bank).
// With 256 query tiles or more a segment is not cut.  Below that it is cut into as many slices as bring the grid of ONE class to
// 512 workgroups, of at least four 64-row tiles each were the class the whole bank, and never more than 64.
int cd_slices(long long Nq, long long M) {
  const long long tiles = (Nq + LT_QT - 1) / LT_QT;
  const long long nb = (M + LT_BT - 1) / LT_BT;
  long long want = tiles >= 256 ? 1 : (512 + tiles - 1) / tiles;
  const long long most = (nb + 3) / 4;
  if (want > most) want = most;
  if (want > CD_MAXS) want = CD_MAXS;
  if (want < 1) want = 1;
  return (int)want;
}

long long cd_ws_bytes(int S, long long Nq, int K) { return S > 1 ? (long long)S * Nq * K * (long long)sizeof(float) : 0; }

const char* const CD_DIMS = "class_dist: Nq and M must be in 1..2^31-1, L in 1..256, K in 1..256";

}  // namespace

extern "C" long long eae_class_dist_workspace_bytes(long long Nq, long long M, int L, int K) {
  if (!cd_dims_ok(Nq, M, L, K)) return eae_set_error(EAE_ERR_ARG, CD_DIMS);
  return cd_ws_bytes(cd_slices(Nq, M), Nq, K);
}

extern "C" int eae_class_dist_sums(void* stream, const float* q, long long Nq, const float* bank, long long M, int L, const long long* seg,
                                   int K, const long long* self_pos, int metric, float* sums, void* workspace, long long workspace_bytes) {
  if (!cd_dims_ok(Nq, M, L, K)) return eae_set_error(EAE_ERR_ARG, CD_DIMS);
  if (!q || !bank || !seg || !sums) return eae_set_error(EAE_ERR_ARG, "class_dist_sums: NULL q, bank, seg or sums");
  if (metric != 0 && metric != 1) return eae_set_error(EAE_ERR_ARG, "class_dist_sums: metric must be 0 (euclidean) or 1 (squared euclidean)");
  const int S = cd_slices(Nq, M);
  if (const int rc = latent_workspace_check(workspace, workspace_bytes, cd_ws_bytes(S, Nq, K),
                                            "class_dist_sums: the workspace is NULL or smaller than eae_class_dist_workspace_bytes")) return rc;
  EAE_NO_GROUP("class_dist_kernel");
  const hipStream_t st = (hipStream_t)stream;
  const SumArgs a = {q, bank, Nq, M, L, K, S, metric, seg, self_pos, S > 1 ? (float*)workspace : sums, latent_vec16(q, L), latent_vec16(bank, L)};
  const long long tiles = (Nq + LT_QT - 1) / LT_QT;
  hipLaunchKernelGGL(class_dist_kernel, dim3((unsigned)tiles, (unsigned)K, (unsigned)S), dim3(LT_NT), 0, st, a);
  EAE_LAUNCH_CHECK();
  if (S > 1) {
    const long long count = Nq * K;
    hipLaunchKernelGGL(class_dist_add_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, st, (const float*)workspace, count, S, sums);
    EAE_LAUNCH_CHECK();
  }
  return 0;
}
