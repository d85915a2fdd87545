// The external classifier with a configurable architecture (eae_mlp_create_ex): 1..4 hidden layers of width 1..512, each
//   Linear -> BatchNorm1d -> ReLU -> Dropout(p_l)        (the Dropout only where p_l > 0),     then Linear(last, C).
// The design is eae_mlp.hip's, for the same reason (the work is launch latency): one training iteration -- forward, CrossEntropy,
// accuracy bookkeeping, backward, Adam with coupled L2 -- is ONE launch of a single 1024-thread workgroup, fp32 with explicit fmaf
// chains, activations in a global workspace of [max_batch][w_l] per layer for h (pre-BN), a (post-dropout) and g (gradient).
// What the fixed kernel unrolls by hand over (128, 64) is a loop over a layer table in the argument block here; the per-layer
// arithmetic is written as there, so in eval mode a row's logits are bitwise those of the fixed kernel at hidden = (128, 64).
// Class weights and ignore_index are a run-time branch of this one kernel (semantics: the header of eae_mlp_kernel.hip.h).
// Eval mode: rows are independent; the launcher spreads them over the device (rows per block = ceil(B / compute units), at most 64).
#include "eae_internal.h"
#include "eae_common.hip.h"
#include <cmath>

#include "eae_mlp_ctx.h"

namespace {
constexpr int NL = EAE_MLP_MAX_HIDDEN, MW = EAE_MLP_MAX_WIDTH;

struct MlpArchArgs {
  MlpArgs a;                       // as eae_mlp.hip fills it; off, h1 .. g1 and p_drop are not read
  int nh, rpb;                     // hidden layers; rows per block in eval mode
  int w[NL];                       // widths
  float p[NL];                     // dropout rates
  long long poff[4 * NL + 3];      // W, b, gamma, beta per hidden layer, last W, last b, total
  long long bnoff[2 * NL + 1];     // running mean, running variance per layer, total
  float *h[NL], *act[NL], *g[NL];  // workspace [max_batch][w_l]
  int weighted; const float* class_w; long long ignore_index; long long* valid;
};

// philox_uniform of eae_mlp.hip.h with the fourth counter word as an argument: hidden layer l draws with 0x9E3779B9 + l, so layer
// 0 is the fixed kernel's stream and two dropout layers do not share a mask
__device__ float philox_uniform_c3(unsigned long long seed, unsigned long long step, uint32_t idx, uint32_t c3) {
  uint32_t c0 = idx, c1 = (uint32_t)step, c2 = (uint32_t)(step >> 32);
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

// col_stats / col_sums2 (eae_mlp.hip.h) split the 1024 threads into W columns x (1024 / W) row lanes; with a W that does not divide
// 1024 the threads past lanes * W form a partial lane whose partial sums land in red[] behind the ones that are read, and are not used.
__global__ EAE_NO_PK __launch_bounds__(T) void mlp_arch_kernel(MlpArchArgs q) {
  const MlpArgs& a = q.a;
  __shared__ float red[2 * T];
  __shared__ float s_mean[NL][MW], s_inv[NL][MW];     // the backward needs every layer's: 4 x 512 x 2 floats = 16 KB
  __shared__ float s_var[MW], c1[MW], c2[MW];         // 8 + 16 + 6 = 30 KB of LDS in all
  const int tid = threadIdx.x;
  const int IN = a.IN, C = a.C, nh = q.nh;
  // rows handled by this block (training: the whole batch in block 0; eval: rpb rows per block)
  const int r0 = a.train ? 0 : blockIdx.x * q.rpb;
  const int nb = a.train ? a.B : min(q.rpb, a.B - r0);
  const int ldx = a.ldx;
  const float* x = a.x + (size_t)r0 * ldx;
  float* dlog = a.dlog + (size_t)r0 * 16;
  // ---- hidden layers
  const float* in = x;
  int ldin = ldx, K = IN;
  size_t mask_off = 0;            // drop_mask: the keep masks [B][w_l] of the layers with p > 0, back to back
  for (int l = 0; l < nh; ++l) {
    const int W = q.w[l];
    const float *Wl = a.P + q.poff[4 * l], *bl = a.P + q.poff[4 * l + 1], *gam = a.P + q.poff[4 * l + 2], *bet = a.P + q.poff[4 * l + 3];
    float *h = q.h[l] + (size_t)r0 * W, *act = q.act[l] + (size_t)r0 * W;
    float *mean = s_mean[l], *inv = s_inv[l];
    float *rm = a.bnrun + q.bnoff[2 * l], *rv = a.bnrun + q.bnoff[2 * l + 1];
    for (int i = tid; i < nb * W; i += T) {
      int b = i / W, j = i % W;
      float s = bl[j];
      for (int k = 0; k < K; ++k) s = fmaf(in[(size_t)b * ldin + k], Wl[j * K + k], s);
      h[i] = s;
    }
    __syncthreads();
    if (a.train) {
      col_stats(h, nb, W, mean, s_var, red);
      if (tid < W) {
        inv[tid] = 1.0f / sqrtf(s_var[tid] + BN_EPS);
        float unb = nb > 1 ? s_var[tid] * nb / (nb - 1) : s_var[tid];
        if (a.update_running) {
          rm[tid] = (1.f - BN_MOM) * rm[tid] + BN_MOM * mean[tid];
          rv[tid] = (1.f - BN_MOM) * rv[tid] + BN_MOM * unb;
        }
      }
      if (tid == 0 && a.nbt && a.update_running) a.nbt[l] += 1;
    } else if (tid < W) {
      mean[tid] = rm[tid];
      inv[tid] = 1.0f / sqrtf(rv[tid] + BN_EPS);
    }
    __syncthreads();
    const float p = q.p[l];
    const float keep_scale = 1.0f / (1.0f - p);
    for (int i = tid; i < nb * W; i += T) {
      int j = i % W;
      float o = fmaf(gam[j], (h[i] - mean[j]) * inv[j], bet[j]);
      float v = fmaxf(o, 0.f);
      if (a.train && p > 0.f) {
        float keep;
        if (a.drop_mask) keep = a.drop_mask[mask_off + i];
        else keep = philox_uniform_c3(a.seed, a.step, (uint32_t)i, 0x9E3779B9u + (uint32_t)l) >= p ? 1.f : 0.f;
        v = v * keep * keep_scale;
      }
      act[i] = v;
    }
    if (p > 0.f) mask_off += (size_t)a.B * W;
    __syncthreads();
    in = act; ldin = W; K = W;
  }
  // ---- last layer + softmax / CE
  const float *WL = a.P + q.poff[4 * nh], *bL = a.P + q.poff[4 * nh + 1];
  for (int i = tid; i < nb * C; i += T) {
    int b = i / C, c = i % C;
    float s = bL[c];
    for (int k = 0; k < K; ++k) s = fmaf(in[b * K + k], WL[c * K + k], s);
    dlog[b * 16 + c] = s;
    if (a.logits) a.logits[(size_t)(r0 + b) * C + c] = s;
  }
  __syncthreads();
  if (a.dlog_in) {
    for (int i = tid; i < nb * C; i += T) dlog[(i / C) * 16 + (i % C)] = a.dlog_in[(size_t)r0 * C + i];
    __syncthreads();
  }
  if (a.probs) {             // predict epilogue (eval mode): class probabilities and label of each row at its window's grid position
    for (int b = tid; b < nb; b += T) {
      const float* l = dlog + b * 16;
      float mx = l[0]; int am = 0;
      for (int c = 1; c < C; ++c) if (l[c] > mx) { mx = l[c]; am = c; }
      float se = 0.f;
      for (int c = 0; c < C; ++c) se += expf(l[c] - mx);
      long long w = a.win0 + r0 + b;
      if (a.index) {
        w = a.index[w];
        if (w < 0 || w >= a.plane) continue;
      }
      for (int c = 0; c < C; ++c) a.probs[c * a.plane + w] = expf(l[c] - mx) / se;
      a.plabels[w] = am;
    }
  }
  if (!a.labels && !a.dlog_in) return;
  float loss = 0.f, corr = 0.f;
  const float* cw = q.class_w;
  const long long ign = q.ignore_index;
  float inv_w = 0.f;
  if (q.weighted) {          // W = sum of cw[label] over the counted rows of the WHOLE batch, summed by every block in the same order
    float s = 0.f;
    int n = 0;
    for (int b = tid; b < a.B; b += T) {
      const long long lab = a.labels[b];
      if (lab != ign && lab >= 0 && lab < C) { s += cw ? cw[(int)lab] : 1.f; ++n; }
    }
    for (int o = 32; o >= 1; o >>= 1) { s += __shfl_xor(s, o, 64); n += __shfl_xor(n, o, 64); }
    if ((tid & 63) == 0) { red[tid >> 6] = s; red[T + (tid >> 6)] = (float)n; }
    __syncthreads();
    float wt = 0.f;
    for (int i = 0; i < T / 64; ++i) wt += red[i];
    if (tid == 0 && blockIdx.x == 0 && q.valid) {
      long long cnt = 0;
      for (int i = 0; i < T / 64; ++i) cnt += (long long)red[T + i];
      *q.valid += cnt;
    }
    inv_w = wt > 0.f ? 1.0f / wt : 0.f;
    __syncthreads();          // red takes the loss partials below
  }
  if (!a.dlog_in)
  for (int b = tid; b < nb; b += T) {
    float* l = dlog + b * 16;
    float mx = l[0]; int am = 0;
    for (int c = 1; c < C; ++c) if (l[c] > mx) { mx = l[c]; am = c; }
    float se = 0.f;
    for (int c = 0; c < C; ++c) se += expf(l[c] - mx);
    float lse = logf(se) + mx;
    if (q.weighted) {
      const long long lab64 = a.labels[r0 + b];
      if (lab64 != ign && lab64 >= 0 && lab64 < C) {
        const int lab = (int)lab64;
        const float wl = cw ? cw[lab] : 1.f;
        loss += wl * (lse - l[lab]) * ((float)a.B * inv_w);
        corr += (am == lab) ? 1.f : 0.f;
        const float sc = wl * inv_w;
        for (int c = 0; c < C; ++c) l[c] = (expf(l[c] - lse) - (c == lab ? 1.f : 0.f)) * sc;
      } else {
        for (int c = 0; c < C; ++c) l[c] = 0.f;
      }
    } else {
      int lab = (int)a.labels[r0 + b];
      loss += lse - l[lab];
      corr += (am == lab) ? 1.f : 0.f;
      for (int c = 0; c < C; ++c) l[c] = (expf(l[c] - lse) - (c == lab ? 1.f : 0.f)) / (float)a.B;
    }
  }
  red[tid] = loss; red[T + tid] = corr;
  __syncthreads();
  if (tid == 0 && a.stats) {
    double sd = 0.0;         // up to 1024 partial sums: a serial fp32 sum loses sqrt(lim) ulps of the mean loss
    float cr = 0.f;
    const int lim = nb < T ? nb : T;
    for (int i = 0; i < lim; ++i) { sd += (double)red[i]; cr += red[T + i]; }
    const float s = (float)sd;
    if (a.train) { a.stats[0] += s; a.stats[1] += (float)nb; a.stats[2] += cr; }   // sum_b CE_b = mean CE * B
    else { atomicAdd(&a.stats[0], s); atomicAdd(&a.stats[1], (float)nb); atomicAdd(&a.stats[2], cr); }
  }
  if (!a.backward) return;
  // =========================================================================================== backward (train only)
  float* G = a.G;
  // gin [nb][ldg]: the gradient at the output of the Linear whose weights are Wn [Cout][W] (first the last layer's dlogits)
  const float* gin = dlog;
  const float* Wn = WL;
  int ldg = 16, Cout = C;
  long long offW = q.poff[4 * nh], offb = q.poff[4 * nh + 1];
  for (int l = nh - 1; l >= 0; --l) {
    const int W = q.w[l];
    const float* gam = a.P + q.poff[4 * l + 2];
    const float *h = q.h[l], *act = q.act[l];
    float* gl = q.g[l];
    const float *mean = s_mean[l], *inv = s_inv[l];
    // dW, db of the Linear above; d(act) -> d(BN output) through ReLU and Dropout
    for (int i = tid; i < Cout * W; i += T) {
      int c = i / W, k = i % W;
      float s = 0.f;
      for (int b = 0; b < nb; ++b) s = fmaf(gin[b * ldg + c], act[b * W + k], s);
      G[offW + i] = s;
    }
    if (tid < Cout) { float s = 0.f; for (int b = 0; b < nb; ++b) s += gin[b * ldg + tid]; G[offb + tid] = s; }
    // d(ReLU o Dropout): act > 0 iff the unit was kept and its BN output was positive
    const float keep = q.p[l] > 0.f ? 1.0f / (1.0f - q.p[l]) : 1.f;
    for (int i = tid; i < nb * W; i += T) {
      int b = i / W, k = i % W;
      float s = 0.f;
      for (int c = 0; c < Cout; ++c) s = fmaf(gin[b * ldg + c], Wn[c * W + k], s);
      gl[i] = act[i] > 0.f ? s * keep : 0.f;
    }
    __syncthreads();
    // BatchNorm backward
    col_sums2(gl, h, mean, inv, nb, W, c1, c2, red);     // c1 = dbeta, c2 = dgamma
    if (tid < W) { G[q.poff[4 * l + 3] + tid] = c1[tid]; G[q.poff[4 * l + 2] + tid] = c2[tid]; }
    for (int i = tid; i < nb * W; i += T) {
      int j = i % W;
      float xh = (h[i] - mean[j]) * inv[j];
      gl[i] = gam[j] * inv[j] / nb * (nb * gl[i] - c1[j] - xh * c2[j]);
    }
    __syncthreads();
    gin = gl; ldg = W; Cout = W;
    Wn = a.P + q.poff[4 * l];
    offW = q.poff[4 * l]; offb = q.poff[4 * l + 1];
  }
  // the first Linear: its input is x
  for (int i = tid; i < Cout * IN; i += T) {
    int j = i / IN, k = i % IN;
    float s = 0.f;
    for (int b = 0; b < nb; ++b) s = fmaf(gin[b * ldg + j], x[(size_t)b * ldx + k], s);
    G[offW + i] = s;
  }
  if (tid < Cout) { float s = 0.f; for (int b = 0; b < nb; ++b) s += gin[b * ldg + tid]; G[offb + tid] = s; }
  __syncthreads();
  if (!a.adam) return;
  // ---- Adam with coupled L2 weight decay (torch.optim.Adam(lr, weight_decay=1e-4), R.md:2625)
  for (long i = tid; i < q.poff[4 * nh + 2]; i += T) {
    float p = a.P[i], g = G[i] + a.wd * p, m = a.M[i], v = a.V[i];
    m = m + a.omb1 * (g - m);
    v = a.b2 * v + a.omb2 * g * g;
    a.P[i] = p - a.step_size * (m / (sqrtf(v) / a.bc2_sqrt + a.eps));
    a.M[i] = m; a.V[i] = v;
  }
}
}  // namespace

static long long r4(long long n) { return (n + 3) & ~3LL; }

static int arch_check(int input_dim, int num_classes, int n_hidden, const int* hidden) {
  if (input_dim <= 0 || input_dim > 1024 || num_classes <= 0 || num_classes > 16) return eae_set_error(EAE_ERR_ARG, "mlp: input_dim in 1..1024, classes in 1..16");
  if (n_hidden < 1 || n_hidden > EAE_MLP_MAX_HIDDEN || !hidden) return eae_set_error(EAE_ERR_ARG, "mlp: 1..4 hidden layers");
  for (int l = 0; l < n_hidden; ++l)
    if (hidden[l] < 1 || hidden[l] > EAE_MLP_MAX_WIDTH) return eae_set_error(EAE_ERR_ARG, "mlp: hidden widths in 1..512");
  return 0;
}

extern "C" int eae_mlp_layout_ex(int input_dim, int num_classes, int n_hidden, const int* hidden, long long* param_off, long long* bn_off) {
  if (int rc = arch_check(input_dim, num_classes, n_hidden, hidden)) return rc;
  long long o = 0, bo = 0;
  int k = input_dim;
  for (int l = 0; l < n_hidden; ++l) {
    const long long w = hidden[l], sz[4] = {w * k, w, w, w};
    for (int i = 0; i < 4; ++i) { if (param_off) param_off[4 * l + i] = o; o += r4(sz[i]); }
    if (bn_off) { bn_off[2 * l] = bo; bn_off[2 * l + 1] = bo + w; }
    bo += 2 * w;
    k = hidden[l];
  }
  if (param_off) {
    param_off[4 * n_hidden] = o; o += r4((long long)num_classes * k);
    param_off[4 * n_hidden + 1] = o; o += r4(num_classes);
    param_off[4 * n_hidden + 2] = o;
  }
  if (bn_off) bn_off[2 * n_hidden] = bo;
  return 0;
}

extern "C" int eae_mlp_create_ex(int input_dim, int num_classes, int n_hidden, const int* hidden, const float* p_drop, int max_batch,
                                 eae_mlp** out) {
  if (!out || max_batch <= 0) return eae_set_error(EAE_ERR_ARG, "mlp_create_ex: bad argument");
  if (int rc = arch_check(input_dim, num_classes, n_hidden, hidden)) return rc;
  if (!p_drop) return eae_set_error(EAE_ERR_ARG, "mlp_create_ex: p_drop is NULL");
  for (int l = 0; l < n_hidden; ++l)
    if (!(p_drop[l] >= 0.f && p_drop[l] < 1.f)) return eae_set_error(EAE_ERR_ARG, "mlp_create_ex: dropout rates in [0, 1)");
  eae_mlp* m = new eae_mlp();
  m->general = 1; m->IN = input_dim; m->C = num_classes; m->Bm = max_batch; m->nh = n_hidden;
  eae_mlp_layout_ex(input_dim, num_classes, n_hidden, hidden, m->poff_ex, m->bnoff_ex);
  long long wsum = 0;
  for (int l = 0; l < n_hidden; ++l) { m->hw[l] = hidden[l]; m->pdrop[l] = p_drop[l]; wsum += hidden[l]; }
  const size_t n = (size_t)max_batch * (size_t)(3 * wsum + 16) * 4;
  hipError_t e = hipMalloc(&m->ws, n);
  if (e != hipSuccess) { delete m; return eae_set_error(EAE_ERR_HIP, hipGetErrorString(e)); }
  float* p = (float*)m->ws;
  for (int l = 0; l < n_hidden; ++l) {
    const size_t s = (size_t)max_batch * hidden[l];
    m->hx[l] = p; p += s; m->ax[l] = p; p += s; m->gx[l] = p; p += s;
  }
  m->dlog = p;
  *out = m;
  return 0;
}

void eae_mlp_arch_bound(eae_mlp* m) {
  hipPointerAttribute_t at;
  int ncu = 0;
  if (hipPointerGetAttributes(&at, m->P) == hipSuccess &&
      hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, at.device) == hipSuccess && ncu > 0)
    m->ncu = ncu;
  else
    (void)hipGetLastError();      // an arena HIP does not know (host memory in a test of the argument checks): keep the default
}

int eae_mlp_arch_launch(eae_mlp* m, hipStream_t st, const MlpArgs& a, int weighted, const float* class_w, long long ignore_index,
                        long long* valid) {
  MlpArchArgs q;
  q.a = a;
  q.nh = m->nh;
  for (int l = 0; l < NL; ++l) {
    const bool on = l < m->nh;
    q.w[l] = on ? m->hw[l] : 0; q.p[l] = on ? m->pdrop[l] : 0.f;
    q.h[l] = on ? m->hx[l] : nullptr; q.act[l] = on ? m->ax[l] : nullptr; q.g[l] = on ? m->gx[l] : nullptr;
  }
  for (int i = 0; i < 4 * NL + 3; ++i) q.poff[i] = i < 4 * m->nh + 3 ? m->poff_ex[i] : 0;
  for (int i = 0; i < 2 * NL + 1; ++i) q.bnoff[i] = i < 2 * m->nh + 1 ? m->bnoff_ex[i] : 0;
  q.weighted = weighted; q.class_w = class_w; q.ignore_index = ignore_index; q.valid = valid;
  // eval mode: one row costs a serial chain over every layer's inputs whatever the block holds, so the rows go to as many
  // compute units as there are; 64 rows per block (the fixed kernel's split) is the cap for batches beyond 64 x the device
  int rpb = (a.B + m->ncu - 1) / m->ncu;
  rpb = rpb < 1 ? 1 : (rpb > 64 ? 64 : rpb);
  q.rpb = rpb;
  const int grid = a.train ? 1 : (a.B + rpb - 1) / rpb;
  hipLaunchKernelGGL(mlp_arch_kernel, dim3(grid), dim3(T), 0, st, q);
  EAE_LAUNCH_CHECK();
  return 0;
}
