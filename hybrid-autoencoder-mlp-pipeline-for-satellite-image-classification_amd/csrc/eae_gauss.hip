// Latent Gaussian models (include/eae.h, "latent Gaussian models"): the two kernels of a Gaussian
// maximum-likelihood classifier over fp32 latents z [N][L], both on the f32-input MFMA (v_mfma_f32_32x32x2_f32: exact fp32, a k-ordered
// fma chain).
//   scatter: S_k = sum over the rows of class k of (z - m_k)(z - m_k)^T.  The rows arrive grouped by class (a row order and K + 1 segment
//            offsets); a wave takes one chunk of one class's segment and one pair of 32-column tiles (i-tile <= j-tile), centres the two
//            operands in the lane and feeds two rows to every MFMA.  Partial tiles go to the caller's workspace; a second kernel adds them
//            in ascending chunk order and writes each tile and its mirror image.  No float atomics.
//   score:   u = W_k^T (z_n - mu_k) with W_k as the A operand, so that a lane owns one row n and holds 16 of every 32 components of u in
//            registers; it squares and adds them, adds the class offset and keeps the running (min, argmin) across the class loop.  N x K x L
//            is written nowhere.
#include "eae_internal.h"
#include "eae_common.hip.h"
#include "eae_latent.hip.h"

namespace {


// ---------------------------------------------------------------------------------------------------------------
// scatter, first kernel.  One wave a workgroup, (g, p, k): chunk g of class k's segment of `order`, tile pair p = (ti <= tj).  The segment
// [seg[k], seg[k + 1]) (clamped into [0, N]) is cut into G chunks of rpc = ceil(n_k / G) rows rounded up to even.  An MFMA takes two
// rows: A[i][row] = z[row][32 ti + i] - m[32 ti + i], B[row][j] = z[row][32 tj + j] - m[32 tj + j], each one fp32 subtraction in the
// lane, the values read straight from global memory (a half wave reads 128 contiguous bytes of a row).  A position beyond the chunk, a
// row index outside [0, N), a row whose label is not k and a column beyond L contribute exact zeros.  Every wave stores its whole
// 32 x 32 tile (zeros for an empty chunk), register-major, so that the second kernel reads nothing that was not written.
// ---------------------------------------------------------------------------------------------------------------
struct ScatterArgs {
  const float* z; const long long* labels; const long long* order; const long long* seg; const float* m; long long N; int L, K, G, T;
  float* part;
};

__device__ __forceinline__ void tile_pair(int p, int jt, int& ti, int& tj) {     // p-th pair (ti <= tj) in row-major order
  ti = 0;
  while (p >= jt - ti) { p -= jt - ti; ++ti; }
  tj = ti + p;
}

__global__ EAE_NO_PK __launch_bounds__(64) void gauss_scatter_kernel(ScatterArgs a) {
  const int lane = threadIdx.x, r = lane & 31, h = lane >> 5;
  const int g = blockIdx.x, p = blockIdx.y, k = blockIdx.z, L = a.L;
  int ti, tj;
  tile_pair(p, (L + 31) >> 5, ti, tj);
  long long s0 = a.seg[k], s1 = a.seg[k + 1];
  s0 = s0 < 0 ? 0 : s0 > a.N ? a.N : s0;
  s1 = s1 < s0 ? s0 : s1 > a.N ? a.N : s1;
  const long long rpc = (((s1 - s0) + a.G - 1) / a.G + 1) & ~1LL;
  const long long r0 = s0 + g * rpc, r1 = r0 + rpc < s1 ? r0 + rpc : s1;
  const int ci = ti * 32 + r, cj = tj * 32 + r;
  const bool iok = ci < L, jok = cj < L;
  const float mi = iok ? a.m[(size_t)k * L + ci] : 0.f, mj = jok ? a.m[(size_t)k * L + cj] : 0.f;

  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;

  constexpr int S = 8;                        // MFMA steps (pairs of rows) whose loads are issued up front
  for (long long rb = r0; rb < r1; rb += 2 * S) {
    float av[S], bv[S];
#pragma unroll
    for (int s = 0; s < S; ++s) {
      const long long pos = rb + 2 * s + h;
      long long row = -1;
      if (pos < r1) row = a.order[pos];
      const bool ok = row >= 0 && row < a.N && a.labels[row] == k;
      av[s] = ok && iok ? a.z[(size_t)row * L + ci] - mi : 0.f;
      bv[s] = ok && jok ? a.z[(size_t)row * L + cj] - mj : 0.f;
    }
#pragma unroll
    for (int s = 0; s < S; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[s], bv[s], acc, 0, 0, 0);
  }

  float* out = a.part + (((size_t)k * a.T + p) * a.G + g) * 1024 + lane;       // slot (k, p, g) of K * T * G: inside the workspace
#pragma unroll
  for (int i = 0; i < 16; ++i) out[i * 64] = acc[i];
}

// scatter, second kernel: workgroup (p, k) adds the G partial tiles of (class k, pair p) element by element in ascending chunk order and
// writes S_k[i][j] and S_k[j][i], i <= j, from the same register: bitwise symmetric by construction.
struct ScatterFinalArgs { const float* part; int L, G, T; float* S; };

__global__ EAE_NO_PK __launch_bounds__(256) void gauss_scatter_finalize_kernel(ScatterFinalArgs a) {
  const int p = blockIdx.x, k = blockIdx.y, L = a.L;
  int ti, tj;
  tile_pair(p, (L + 31) >> 5, ti, tj);
  const float* src = a.part + ((size_t)k * a.T + p) * a.G * 1024;
  float* Sk = a.S + (size_t)k * L * L;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int e = threadIdx.x + 256 * q, reg = e >> 6, lane = e & 63;
    const int gi = ti * 32 + acc_row(reg, lane >> 5), gj = tj * 32 + (lane & 31);
    float s = 0.f;
    for (int g = 0; g < a.G; ++g) s += src[(size_t)g * 1024 + e];
    if (gi <= gj && gj < L) {                 // (a diagonal tile's upper triangle only: the lower one is its mirror image)
      Sk[(size_t)gi * L + gj] = s;
      Sk[(size_t)gj * L + gi] = s;
    }
  }
}

// The scatter's geometry, a function of (N, L, K) alone: T tile pairs and G chunks a class, one chunk for every 1024 rows of z, at most
// 256 and no more than keep the partials near 64 MB.
struct ScatterPlan { int T, G; };
ScatterPlan gauss_scatter_plan(long long N, int L, int K) {
  ScatterPlan p;
  const int jt = (L + 31) >> 5;
  p.T = jt * (jt + 1) / 2;
  long long gmax = (64LL << 20) / ((long long)K * p.T * 4096);
  gmax = gmax < 1 ? 1 : gmax > 256 ? 256 : gmax;
  const long long g = (N + 1023) / 1024;
  p.G = (int)(g < gmax ? g : gmax);
  return p;
}
long long gauss_scatter_bytes(const ScatterPlan& p, int K) { return (long long)K * p.T * p.G * 4096; }

// ---------------------------------------------------------------------------------------------------------------
// score.  Workgroup tile = 128 rows; wave w owns rows 32 w .. 32 w + 31 of it.  For every class the rows of W_k are walked in passes of
// LC (gs_lc): the pass's LC columns of the z tile and of mu_k and its LC rows of W_k (all JT * 32 columns) are staged in LDS, zero beyond
// L and beyond N (with L <= 64 the z tile is staged once per tile, not once per class).  Then for every pair of l one MFMA per 32-column tile
// of u: A[j][l] = W_k[l][j], B[l][n] = z_n[l] - mu_k[l], the subtraction made in the lane as it reads the operand.  All JT accumulator
// tiles stay in registers across the passes.  d = sum_j u_j^2: the lane's 16 * JT values in one fma chain, then the other lane half's
// (commutative: both halves hold the same bits).  score = d + offset_k, or +inf where offset_k is +inf; strict < in ascending k keeps
// the lowest index on a tie.  Nothing here depends on the grid or on the row's place in its tile.
// ---------------------------------------------------------------------------------------------------------------
constexpr int GS_NT = 256;
constexpr int GS_ROWS = 128;
// columns of z (= rows of W_k) staged per pass: 64, and 32 at JT = 8, where 64 rows of 256 columns of W_k would leave the LDS room for
// one workgroup a CU; with two, one stages while the other multiplies
constexpr int gs_lc(int JT) { return JT == 8 ? 32 : 64; }
// z rows of LC + 2 floats, as eae_cluster.hip: lane (r, h) reads word r * (LC + 2) + kk + h, 64 different banks for LC = 64 and 32
// W rows: lane (r, h) reads word (kk + h) * WS + 32 t + r; WS = 32 mod 64 puts the two lane halves on different banks
constexpr int gs_ws(int JT) { return JT == 1 ? 32 : JT * 32 + 32; }

struct ScoreArgs {
  const float* z; long long N; int L, K; const float* mu; const float* W; long long wstride; const float* offset;
  long long* labels; float* maha; float* best; float* scores;
  int vec;        // 16-byte loads of z: L % 4 == 0 and an aligned base
};

template <int JT>
__global__ EAE_NO_PK __launch_bounds__(GS_NT, 2) void gauss_score_kernel(ScoreArgs a) {
  extern __shared__ __attribute__((aligned(16))) float gs_lds[];
  constexpr int WS = gs_ws(JT), GS_LC = gs_lc(JT), GS_LDS = GS_LC + 2;
  float* zs = gs_lds;                                  // [128][LC + 2]
  float* ws = zs + GS_ROWS * GS_LDS;                   // [LC][WS]
  float* ms = ws + GS_LC * WS;                         // [LC]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
  const int L = a.L, K = a.K;
  const long long N = a.N;
  const bool onepass = L <= GS_LC;

  const long long ntiles = (N + GS_ROWS - 1) / GS_ROWS;
  for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const long long n0 = tile * GS_ROWS;
    const long long n = n0 + wave * 32 + r;
    float best = __builtin_inff(), bd = 0.f, zbad = 0.f;
    int bk = -1;

    for (int k = 0; k < K; ++k) {
      f32x16 acc[JT];
#pragma unroll
      for (int t = 0; t < JT; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[t][i] = 0.f;
      const float* Wk = a.W + (size_t)k * a.wstride;

      for (int l0 = 0; l0 < L; l0 += GS_LC) {
        const int lw = L - l0 < GS_LC ? L - l0 : GS_LC;          // real columns of this pass
        const int lw2 = (lw + 1) & ~1;                           // walked in pairs
        __syncthreads();                                         // the previous pass (or class, or tile) is done with the LDS
        if (!onepass || k == 0) {                                // z tile: [128][LC] of z[n0 ..][l0 ..]
          if (a.vec) {
#pragma unroll
            for (int i = 0; i < GS_ROWS * (GS_LC / 4) / GS_NT; ++i) {
              const int idx = tid + GS_NT * i, row = idx / (GS_LC / 4), col = (idx % (GS_LC / 4)) * 4;
              float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
              if (n0 + row < N && col < lw) v = *reinterpret_cast<const float4*>(a.z + (size_t)(n0 + row) * L + l0 + col);
              float2* d = reinterpret_cast<float2*>(zs + row * GS_LDS + col);
              d[0] = make_float2(v.x, v.y); d[1] = make_float2(v.z, v.w);
            }
          } else {
#pragma unroll 4
            for (int i = 0; i < GS_ROWS * GS_LC / GS_NT; ++i) {
              const int idx = tid + GS_NT * i, row = idx / GS_LC, col = idx % GS_LC;
              float v = 0.f;
              if (n0 + row < N && col < lw) v = a.z[(size_t)(n0 + row) * L + l0 + col];
              zs[row * GS_LDS + col] = v;
            }
          }
        }
        // W_k rows l0 .. l0 + LC - 1, columns 0 .. JT * 32 - 1
#pragma unroll 4
        for (int i = 0; i < GS_LC * JT * 32 / GS_NT; ++i) {
          const int idx = tid + GS_NT * i, row = idx / (JT * 32), col = idx % (JT * 32);
          float v = 0.f;
          if (row < lw && col < L) v = Wk[(size_t)(l0 + row) * L + col];
          ws[row * WS + col] = v;
        }
        if (tid < GS_LC) ms[tid] = tid < lw ? a.mu[(size_t)k * L + l0 + tid] : 0.f;
        __syncthreads();
        const float* zrow = zs + (wave * 32 + r) * GS_LDS + h;
        const float* wrow = ws + h * WS + r;
        for (int kk = 0; kk < lw2; kk += 2) {
          const float zv = zrow[kk];
          zbad = __builtin_fmaf(zv, 0.f, zbad);                  // 0, or NaN once the row has shown an Inf or a NaN
          const float b = zv - ms[kk + h];
#pragma unroll
          for (int t = 0; t < JT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(wrow[kk * WS + t * 32], b, acc[t], 0, 0, 0);
        }
      }

      float d = 0.f;
#pragma unroll
      for (int t = 0; t < JT; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) d = __builtin_fmaf(acc[t][i], acc[t][i], d);
      d += __shfl_xor(d, 32, 64);
      const float off = a.offset[k];
      const float s = off == __builtin_inff() ? off : d + off;
      if (s < best) { best = s; bk = k; bd = d; }
      if (a.scores && h == 0 && n < N) a.scores[(size_t)n * K + k] = s;      // (a non-finite row's are overwritten below)
    }

    zbad += __shfl_xor(zbad, 32, 64);
    if (h == 0 && n < N) {
      const bool bad = zbad != 0.f;                              // NaN != 0
      const float nan = __builtin_nanf("");
      a.labels[n] = bad ? -1 : (long long)bk;
      if (a.maha) a.maha[n] = bad || bk < 0 ? nan : fmaxf(bd, 0.f);
      if (a.best) a.best[n] = bad ? nan : best;
      if (a.scores && bad)
        for (int k = 0; k < K; ++k) a.scores[(size_t)n * K + k] = nan;
    }
  }
}

template <int JT> int launch_score(hipStream_t st, const ScoreArgs& a) {
  const size_t lds = ((size_t)GS_ROWS * (gs_lc(JT) + 2) + (size_t)gs_lc(JT) * gs_ws(JT) + gs_lc(JT)) * sizeof(float);
  EAE_HIP(eae_smem_attr((const void*)gauss_score_kernel<JT>, lds));
  hipLaunchKernelGGL(gauss_score_kernel<JT>, dim3(latent_row_tile_grid(a.N, GS_ROWS)), dim3(GS_NT), lds, st, a);
  EAE_LAUNCH_CHECK();
  return 0;
}

}  // namespace

extern "C" long long eae_class_scatter_workspace_bytes(long long N, int L, int K) {
  if (!latent_dims_ok(N, L, K)) return eae_set_error(EAE_ERR_ARG, "class_scatter: N must be in 1..2^31-1, L and K in 1..256");
  return gauss_scatter_bytes(gauss_scatter_plan(N, L, K), K);
}

extern "C" int eae_class_scatter(void* stream, const float* z, long long N, int L, const long long* labels, const long long* order,
                                 const long long* seg, int K, const float* means, float* scatter, void* workspace,
                                 long long workspace_bytes) {
  if (!latent_dims_ok(N, L, K)) return eae_set_error(EAE_ERR_ARG, "class_scatter: N must be in 1..2^31-1, L and K in 1..256");
  if (!z || !labels || !order || !seg || !means || !scatter)
    return eae_set_error(EAE_ERR_ARG, "class_scatter: NULL z, labels, order, seg, means or scatter");
  const ScatterPlan p = gauss_scatter_plan(N, L, K);
  if (const int rc = latent_workspace_check(workspace, workspace_bytes, gauss_scatter_bytes(p, K),
                                            "class_scatter: the workspace is NULL or smaller than eae_class_scatter_workspace_bytes")) return rc;
  EAE_NO_GROUP("gauss_scatter_kernel");
  const hipStream_t st = (hipStream_t)stream;
  const ScatterArgs a = {z, labels, order, seg, means, N, L, K, p.G, p.T, (float*)workspace};
  hipLaunchKernelGGL(gauss_scatter_kernel, dim3((unsigned)p.G, (unsigned)p.T, (unsigned)K), dim3(64), 0, st, a);
  EAE_LAUNCH_CHECK();
  const ScatterFinalArgs f = {(const float*)workspace, L, p.G, p.T, scatter};
  hipLaunchKernelGGL(gauss_scatter_finalize_kernel, dim3((unsigned)p.T, (unsigned)K), dim3(256), 0, st, f);
  EAE_LAUNCH_CHECK();
  return 0;
}

extern "C" int eae_gauss_score(void* stream, const float* z, long long N, int L, const float* mu, const float* W, long long w_stride,
                               const float* offset, int K, long long* labels, float* maha, float* best, float* scores) {
  if (!latent_dims_ok(N, L, K)) return eae_set_error(EAE_ERR_ARG, "gauss_score: N must be in 1..2^31-1, L and K in 1..256");
  if (!z || !mu || !W || !offset || !labels) return eae_set_error(EAE_ERR_ARG, "gauss_score: NULL z, mu, W, offset or labels");
  if (w_stride != 0 && w_stride != (long long)L * L)
    return eae_set_error(EAE_ERR_ARG, "gauss_score: w_stride must be L * L (a matrix a class) or 0 (one shared matrix)");
  EAE_NO_GROUP("gauss_score_kernel");
  const hipStream_t st = (hipStream_t)stream;
  const ScoreArgs a = {z, N, L, K, mu, W, w_stride, offset, labels, maha, best, scores, latent_vec16(z, L)};
  return latent_for_tiles(latent_tiles32(L), [&](auto jt) { return launch_score<jt.value>(st, a); });
}
