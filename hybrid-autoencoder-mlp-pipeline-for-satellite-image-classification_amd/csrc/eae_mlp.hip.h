// Argument block and helpers of the MLP kernel, shared by the two translation units that define it from eae_mlp_kernel.hip.h:
// eae_mlp.hip (the plain kernel) and eae_mlp_wce.hip (class-weighted CrossEntropyLoss with ignored labels).
#pragma once
#include "eae_internal.h"
#include "eae_common.hip.h"

struct MlpArgs {
  const float* x; const long long* labels;
  int B, IN, C;
  float *P, *G, *M, *V;
  long long off[11];
  float* bnrun;            // rm1[128] rv1[128] rm2[64] rv2[64]
  long long* nbt;          // [2]
  float *h1, *a1, *h2, *a2, *dlog, *g2, *g1;   // workspace
  int train, backward, adam;
  float step_size, bc2_sqrt, b1, b2, omb1, omb2, eps, wd;   // omb = 1 - beta, rounded from double as torch does
  unsigned long long seed, step;
  const float* drop_mask;
  const float* dlog_in;    // externally supplied dL/dlogits [B][C] (autograd path) or nullptr
  int update_running;      // 0: do not touch running statistics / num_batches_tracked (recompute pass of the autograd path)
  float p_drop;
  float* logits; float* stats;    // stats: += loss*B, += B, += correct
  int ldx;                 // row stride of x (IN, or the AE engine's padded latent width)
  float* probs;            // eval-mode predict epilogue (scene classification): softmax -> probs[c * plane + win0 + row], or nullptr
  long long* plabels;      // argmax (first maximum) -> plabels[win0 + row]
  long long win0, plane;
  const long long* index;  // predict epilogue: row r goes to window index[win0 + r] (skipped outside [0, plane)), or nullptr: win0 + r
};
// eae_mlp_set_class_weights: what the weighted kernel receives; valid: device word, += the counted rows of the batch, or nullptr
struct MlpArgsW { MlpArgs a; const float* class_w; long long ignore_index; long long* valid; };
void eae_mlp_launch_wce(hipStream_t st, int grid, const MlpArgs& a, const float* class_w, long long ignore_index, long long* valid);   // eae_mlp_wce.hip

namespace {
constexpr int H1 = 128, H2 = 64, T = 1024;
constexpr float BN_EPS = 1e-5f, BN_MOM = 0.1f;


// Philox4x32-10 (counter-based): keep-mask of nn.Dropout, keyed by (seed, optimisation step), counter = element index
__device__ __forceinline__ uint32_t mulhi(uint32_t a, uint32_t b) { return __umulhi(a, b); }
__device__ float philox_uniform(unsigned long long seed, unsigned long long step, uint32_t idx) {
  uint32_t c0 = idx, c1 = (uint32_t)step, c2 = (uint32_t)(step >> 32), c3 = 0x9E3779B9u;
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    uint32_t h0 = mulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
    uint32_t h1 = mulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
    uint32_t n0 = h1 ^ c1 ^ k0, n1 = l1, n2 = h0 ^ c3 ^ k1, n3 = l0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return (float)(c0 >> 8) * (1.0f / 16777216.0f);
}

// per-column batch statistics of v[rows][W] (two-pass), 1024 threads = W columns x (1024/W) row lanes
__device__ void col_stats(const float* v, int rows, int W, float* s_mean, float* s_var, float* red) {
  const int tid = threadIdx.x, lanes = T / W, col = tid % W, rl = tid / W;
  float s = 0.f;
  for (int r = rl; r < rows; r += lanes) s += v[r * W + col];
  red[rl * W + col] = s;
  __syncthreads();
  if (tid < W) { float a = 0.f; for (int i = 0; i < lanes; ++i) a += red[i * W + tid]; s_mean[tid] = a / rows; }
  __syncthreads();
  const float m = s_mean[col];
  s = 0.f;
  for (int r = rl; r < rows; r += lanes) { float d = v[r * W + col] - m; s = fmaf(d, d, s); }
  red[rl * W + col] = s;
  __syncthreads();
  if (tid < W) { float a = 0.f; for (int i = 0; i < lanes; ++i) a += red[i * W + tid]; s_var[tid] = a / rows; }
  __syncthreads();
}

// column sums of g[rows][W] and of g*xhat with xhat = (h-mean)*invstd
__device__ void col_sums2(const float* g, const float* h, const float* s_mean, const float* s_inv, int rows, int W, float* o1,
                          float* o2, float* red) {
  const int tid = threadIdx.x, lanes = T / W, col = tid % W, rl = tid / W;
  float a = 0.f, b = 0.f;
  for (int r = rl; r < rows; r += lanes) {
    float gv = g[r * W + col];
    a += gv;
    b = fmaf(gv, (h[r * W + col] - s_mean[col]) * s_inv[col], b);
  }
  red[rl * W + col] = a; red[T + rl * W + col] = b;
  __syncthreads();
  if (tid < W) {
    float x = 0.f, y = 0.f;
    for (int i = 0; i < lanes; ++i) { x += red[i * W + tid]; y += red[T + i * W + tid]; }
    o1[tid] = x; o2[tid] = y;
  }
  __syncthreads();
}

}  // namespace
