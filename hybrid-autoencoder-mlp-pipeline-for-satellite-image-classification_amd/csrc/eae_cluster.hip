// Latent clustering (include/eae.h, "latent clustering"): the two halves of a Lloyd iteration over fp32 latents
// z [N][L] and centroids c [K][L], both on the f32-input MFMA (v_mfma_f32_32x32x2_f32: exact fp32, a k-ordered fma chain).
//   assign: D[c][n] = c_c . z_n with the CENTROIDS as the A operand, so that a lane owns one row n (its column of D) and holds 16
//           centroids of every 32-centroid tile in registers: the running (min, argmin) never leaves the lane, and N x K is written
//           nowhere.
//   update: sums[K][L] = onehot^T[K][rows] . z[rows][L], the one-hot operand made in registers from the labels; per-workgroup partial
//           sums go to the caller's workspace and a second kernel adds them in one fixed order and divides.  No float atomics.
#include "eae_internal.h"
#include "eae_common.hip.h"
#include "eae_latent.hip.h"

namespace {

constexpr int KM_NT = 256;        // threads per workgroup: 4 waves
constexpr int KM_ROWS = 128;      // assign: rows of z per workgroup tile, 32 per wave
constexpr int KM_LC = 64;         // assign: columns of z and c staged per pass
constexpr int KM_LDS = KM_LC + 2; // LDS row stride in floats: lane (r, h) reads word r * 66 + kk + h -> bank 2r + h + kk, 64 different banks

// ---------------------------------------------------------------------------------------------------------------
// assign.  Workgroup tile = 128 rows; wave w owns rows 32 w .. 32 w + 31 of it.  The columns are walked in passes of 64: the z tile's
// and the centroids' 64 columns are staged in LDS (zero beyond L, beyond N and beyond K), then for every pair of columns one MFMA per
// 32-centroid tile, all KT tiles' accumulators staying in registers across the passes.  ||z_n||^2 and the row's finiteness are
// accumulated by the lanes from the B operands they read anyway; ||c_k||^2 is a sequential fma chain per centroid, the same in every
// workgroup.  score = fma(-2, dot, ||c||^2); strict < in ascending k keeps the lowest index on a tie, in the lane and between the two
// lane halves.  Nothing here depends on the grid: a row's label is a function of its own values and the centroids.
// ---------------------------------------------------------------------------------------------------------------
struct AssignArgs {
  const float* z; const float* c; long long N; int L, K; long long* labels; int have_prev; float* dist; unsigned long long* changed;
  int vec;        // 16-byte loads of z: L % 4 == 0 and an aligned base
};

template <int KT>
__global__ EAE_NO_PK __launch_bounds__(KM_NT) void kmeans_assign_kernel(AssignArgs a) {
  extern __shared__ __attribute__((aligned(16))) float km_lds[];
  float* zs = km_lds;                                  // [128][66]
  float* cs = zs + KM_ROWS * KM_LDS;                   // [KT * 32][66]
  float* cn = cs + KT * 32 * KM_LDS;                   // [KT * 32]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
  const int L = a.L, K = a.K;
  const long long N = a.N;

  // ||c_k||^2: thread k, one fixed-order chain
  for (int k = tid; k < KT * 32; k += KM_NT) {
    cn[k] = k < K ? row_sq_chain(a.c + (size_t)k * L, L) : 0.f;
  }

  const long long ntiles = (N + KM_ROWS - 1) / KM_ROWS;
  for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const long long n0 = tile * KM_ROWS;
    f32x16 acc[KT];
#pragma unroll
    for (int t = 0; t < KT; ++t)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[t][i] = 0.f;
    float zn = 0.f, zbad = 0.f;

    for (int l0 = 0; l0 < L; l0 += KM_LC) {
      const int lw = L - l0 < KM_LC ? L - l0 : KM_LC;          // real columns of this pass
      const int lw2 = (lw + 1) & ~1;                           // walked in pairs
      __syncthreads();                                         // the previous pass (or tile, or the cn loop) is done with the LDS
      // z tile: [128][64] of z[n0 ..][l0 ..]
      if (a.vec) {
#pragma unroll
        for (int i = 0; i < KM_ROWS * (KM_LC / 4) / KM_NT; ++i) {
          const int idx = tid + KM_NT * i, row = idx >> 4, col = (idx & 15) * 4;
          float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
          if (n0 + row < N && col < lw) v = *reinterpret_cast<const float4*>(a.z + (size_t)(n0 + row) * L + l0 + col);
          float2* d = reinterpret_cast<float2*>(zs + row * KM_LDS + col);
          d[0] = make_float2(v.x, v.y); d[1] = make_float2(v.z, v.w);
        }
      } else {
#pragma unroll 4
        for (int i = 0; i < KM_ROWS * KM_LC / KM_NT; ++i) {
          const int idx = tid + KM_NT * i, row = idx >> 6, col = idx & 63;
          float v = 0.f;
          if (n0 + row < N && col < lw) v = a.z[(size_t)(n0 + row) * L + l0 + col];
          zs[row * KM_LDS + col] = v;
        }
      }
      // centroids: [KT * 32][64] of c[..][l0 ..]
#pragma unroll 4
      for (int i = 0; i < KT * 32 * KM_LC / KM_NT; ++i) {
        const int idx = tid + KM_NT * i, row = idx >> 6, col = idx & 63;
        float v = 0.f;
        if (row < K && col < lw) v = a.c[(size_t)row * L + l0 + col];
        cs[row * KM_LDS + col] = v;
      }
      __syncthreads();
      const float* zrow = zs + (wave * 32 + r) * KM_LDS + h;
      const float* crow = cs + r * KM_LDS + h;
      for (int kk = 0; kk < lw2; kk += 2) {
        const float b = zrow[kk];
        zn = __builtin_fmaf(b, b, zn);
        zbad = __builtin_fmaf(b, 0.f, zbad);                   // 0, or NaN once the row has shown an Inf or a NaN
#pragma unroll
        for (int t = 0; t < KT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(crow[t * 32 * KM_LDS + kk], b, acc[t], 0, 0, 0);
      }
    }

    // the lane's 16 * KT centroids in ascending k, then the other half's
    float best = __builtin_inff();
    int bk = 0;
#pragma unroll
    for (int t = 0; t < KT; ++t)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int k = t * 32 + acc_row(i, h);
        const float s = __builtin_fmaf(-2.f, acc[t][i], cn[k]);
        if (k < K && s < best) { best = s; bk = k; }
      }
    const float obest = __shfl_xor(best, 32, 64);
    const int obk = __shfl_xor(bk, 32, 64);
    if (obest < best || (obest == best && obk < bk)) { best = obest; bk = obk; }
    zn += __shfl_xor(zn, 32, 64);                              // (commutative: both halves hold the same bits)
    zbad += __shfl_xor(zbad, 32, 64);
    const long long n = n0 + wave * 32 + r;
    bool diff = false;
    if (h == 0 && n < N) {
      const bool bad = zbad != 0.f;                            // NaN != 0
      const long long lab = bad ? -1 : (long long)bk;
      if (a.have_prev) diff = a.labels[n] != lab;
      a.labels[n] = lab;
      if (a.dist) a.dist[n] = bad ? __builtin_nanf("") : fmaxf(best + zn, 0.f);
    }
    if (a.have_prev && a.changed) {
      const unsigned long long m = __ballot(diff);
      if (lane == 0 && m) atomicAdd(a.changed, (unsigned long long)__popcll(m));
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------
// update, first kernel.  Workgroup (g, lt): rows [g * rpc, (g + 1) * rpc) of z, columns 32 lt .. 32 lt + 31, every centroid.  An MFMA
// takes two rows: A[k][row] = (label[row] == k) made in the lane from the label, B[row][l] = z read straight from global memory (a
// half wave reads 128 contiguous bytes).  Wave w takes the row groups w, w + 4, ... of the chunk (16 rows = 8 MFMA steps per group, 8 rows at K > 128), a group's
// loads issued up front.  A row whose label is outside [0, K) contributes B = 0 as well, so that the non-finite rows that assign
// labelled -1 poison nothing.  The four waves' tiles are added through LDS in wave order and stored as partial g.
// Workgroups with lt == 0 also count their chunk's labels (LDS integers, then one 64-bit global add per cluster).
// ---------------------------------------------------------------------------------------------------------------
struct UpdateArgs {
  const float* z; const long long* labels; long long N; int L, K; long long rpc; float* part; int Kp, Lp; unsigned long long* counts;
};

template <int KT>
__global__ EAE_NO_PK __launch_bounds__(KM_NT) void kmeans_partial_kernel(UpdateArgs a) {
  __shared__ float red[KT * 16 * 64];
  __shared__ int hist[LATENT_MAXK];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
  const int L = a.L, K = a.K, lt = blockIdx.y;
  const long long g = blockIdx.x, N = a.N;
  const long long r0 = g * a.rpc, r1 = r0 + a.rpc < N ? r0 + a.rpc : N;
  const int col = lt * 32 + r;
  const bool colok = col < L;

  f32x16 acc[KT];
#pragma unroll
  for (int t = 0; t < KT; ++t)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[t][i] = 0.f;

  constexpr int S = KT == 8 ? 4 : 8;          // MFMA steps (pairs of rows) per group; 4 where 128 accumulators leave fewer registers
  for (long long rb = r0 + wave * 2 * S; rb < r1; rb += 8 * S) {
    float b[S];
    int lab[S];
#pragma unroll
    for (int s = 0; s < S; ++s) {
      const long long n = rb + 2 * s + h;
      long long lb = -1;
      if (n < r1) lb = a.labels[n];
      const bool ok = lb >= 0 && lb < K;
      lab[s] = ok ? (int)lb : -1;
      b[s] = ok && colok ? a.z[(size_t)n * L + col] : 0.f;
    }
#pragma unroll
    for (int s = 0; s < S; ++s)
#pragma unroll
      for (int t = 0; t < KT; ++t)
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(lab[s] == t * 32 + r ? 1.f : 0.f, b[s], acc[t], 0, 0, 0);
  }

  // ((wave 0 + wave 1) + wave 2) + wave 3, element by element; wave 3 stores
  for (int w = 0; w < 4; ++w) {
    if (wave == w) {
#pragma unroll
      for (int t = 0; t < KT; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          float* p = red + (t * 16 + i) * 64 + lane;
          const float v = w == 0 ? acc[t][i] : *p + acc[t][i];
          if (w < 3) *p = v;
          else a.part[((size_t)g * a.Kp + t * 32 + acc_row(i, h)) * a.Lp + col] = v;       // col < Lp, row < Kp: inside slot g
        }
    }
    if (w < 3) __syncthreads();
  }

  if (lt == 0) {
    for (int k = tid; k < LATENT_MAXK; k += KM_NT) hist[k] = 0;
    __syncthreads();
    for (long long n = r0 + tid; n < r1; n += KM_NT) {
      const long long lb = a.labels[n];
      if (lb >= 0 && lb < K) atomicAdd(&hist[(int)lb], 1);
    }
    __syncthreads();
    for (int k = tid; k < K; k += KM_NT)
      if (hist[k]) atomicAdd(a.counts + k, (unsigned long long)hist[k]);
  }
}

// update, second kernel: workgroup k adds the G partials of centroid k in one fixed order and divides.  256 threads = ngrp groups of Lr
// columns (Lr = L rounded up to 32): group q adds partials q, q + ngrp, ... in ascending order, then the groups are added in ascending
// order.  An empty cluster keeps its centroid.
struct FinalArgs { const float* part; long long G; int Kp, Lp, L; const unsigned long long* counts; float* c; };

__global__ EAE_NO_PK __launch_bounds__(KM_NT) void kmeans_finalize_kernel(FinalArgs a) {
  __shared__ float red[KM_NT];
  const int k = blockIdx.x, tid = threadIdx.x, Lr = a.Lp, ngrp = KM_NT / Lr, q = tid / Lr, l = tid - q * Lr;
  float s = 0.f;
  if (q < ngrp) {
    const float* p = a.part + (size_t)k * a.Lp + l;
    const size_t slot = (size_t)a.Kp * a.Lp;
#pragma unroll 4
    for (long long g = q; g < a.G; g += ngrp) s += p[(size_t)g * slot];
  }
  red[tid] = s;
  __syncthreads();
  const unsigned long long cnt = a.counts[k];
  if (q == 0 && l < a.L && cnt != 0) {
    float t = red[l];
    for (int j = 1; j < ngrp; ++j) t += red[j * Lr + l];
    a.c[(size_t)k * a.L + l] = t / (float)cnt;
  }
}

// The update's geometry, a function of (N, L, K) alone: G row chunks of rpc rows (a multiple of 64: whole 16-row groups for 4 waves),
// as many as keep the partials near 32 MB, between 128 and 2048, and no more than the rows fill.
struct UpdatePlan { int Kp, Lp; long long rpc, G; };
UpdatePlan kmeans_update_plan(long long N, int L, int K) {
  UpdatePlan p;
  p.Kp = latent_tiles32(K) * 32;
  p.Lp = (L + 31) & ~31;
  long long gmax = (32LL << 20) / ((long long)p.Kp * p.Lp * 4);
  gmax = gmax < 128 ? 128 : gmax > 2048 ? 2048 : gmax;
  long long rpc = (N + gmax - 1) / gmax;
  if (rpc < 512) rpc = 512;
  p.rpc = (rpc + 63) & ~63LL;
  p.G = (N + p.rpc - 1) / p.rpc;
  return p;
}

template <int KT> int launch_assign(hipStream_t st, const AssignArgs& a) {
  const size_t lds = ((size_t)(KM_ROWS + KT * 32) * KM_LDS + KT * 32) * sizeof(float);
  EAE_HIP(eae_smem_attr((const void*)kmeans_assign_kernel<KT>, lds));
  hipLaunchKernelGGL(kmeans_assign_kernel<KT>, dim3(latent_row_tile_grid(a.N, KM_ROWS)), dim3(KM_NT), lds, st, a);
  EAE_LAUNCH_CHECK();
  return 0;
}
template <int KT> int launch_partial(hipStream_t st, const UpdateArgs& a, const UpdatePlan& p) {
  hipLaunchKernelGGL(kmeans_partial_kernel<KT>, dim3((unsigned)p.G, (unsigned)(p.Lp / 32)), dim3(KM_NT), 0, st, a);
  EAE_LAUNCH_CHECK();
  return 0;
}

}  // namespace

extern "C" long long eae_kmeans_workspace_bytes(long long N, int L, int K) {
  if (!latent_dims_ok(N, L, K)) return eae_set_error(EAE_ERR_ARG, "kmeans: N must be in 1..2^31-1, L and K in 1..256");
  const UpdatePlan p = kmeans_update_plan(N, L, K);
  return p.G * p.Kp * p.Lp * (long long)sizeof(float);
}

extern "C" int eae_kmeans_assign(void* stream, const float* z, long long N, int L, const float* centroids, int K, long long* labels,
                                 int have_prev, float* dist, long long* changed) {
  if (!latent_dims_ok(N, L, K)) return eae_set_error(EAE_ERR_ARG, "kmeans_assign: N must be in 1..2^31-1, L and K in 1..256");
  if (!z || !centroids || !labels) return eae_set_error(EAE_ERR_ARG, "kmeans_assign: NULL z, centroids or labels");
  EAE_NO_GROUP("kmeans_assign_kernel");
  const hipStream_t st = (hipStream_t)stream;
  const bool count = have_prev != 0 && changed != nullptr;
  if (count && hipMemsetAsync(changed, 0, sizeof(long long), st) != hipSuccess)
    return eae_set_error(EAE_ERR_HIP, "kmeans_assign: clearing the changed counter failed");
  const AssignArgs a = {z, centroids, N, L, K, labels, have_prev != 0, dist, count ? (unsigned long long*)changed : nullptr, latent_vec16(z, L)};
  return latent_for_tiles(latent_tiles32(K), [&](auto kt) { return launch_assign<kt.value>(st, a); });
}

extern "C" int eae_kmeans_update(void* stream, const float* z, long long N, int L, const long long* labels, int K, float* centroids,
                                 long long* counts, void* workspace, long long workspace_bytes) {
  if (!latent_dims_ok(N, L, K)) return eae_set_error(EAE_ERR_ARG, "kmeans_update: N must be in 1..2^31-1, L and K in 1..256");
  if (!z || !labels || !centroids || !counts) return eae_set_error(EAE_ERR_ARG, "kmeans_update: NULL z, labels, centroids or counts");
  const UpdatePlan p = kmeans_update_plan(N, L, K);
  if (const int rc = latent_workspace_check(workspace, workspace_bytes, p.G * p.Kp * p.Lp * (long long)sizeof(float),
                                            "kmeans_update: the workspace is NULL or smaller than eae_kmeans_workspace_bytes")) return rc;
  EAE_NO_GROUP("kmeans_partial_kernel");
  const hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(counts, 0, (size_t)K * sizeof(long long), st) != hipSuccess)
    return eae_set_error(EAE_ERR_HIP, "kmeans_update: clearing counts failed");
  const UpdateArgs a = {z, labels, N, L, K, p.rpc, (float*)workspace, p.Kp, p.Lp, (unsigned long long*)counts};
  if (const int rc = latent_for_tiles(latent_tiles32(K), [&](auto kt) { return launch_partial<kt.value>(st, a, p); })) return rc;
  const FinalArgs f = {(const float*)workspace, p.G, p.Kp, p.Lp, L, (const unsigned long long*)counts, centroids};
  hipLaunchKernelGGL(kmeans_finalize_kernel, dim3(K), dim3(KM_NT), 0, st, f);
  EAE_LAUNCH_CHECK();
  return 0;
}
