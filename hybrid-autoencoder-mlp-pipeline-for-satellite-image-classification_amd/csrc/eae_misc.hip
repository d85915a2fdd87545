// Small kernels: BatchNorm finalisation (forward statistics -> apply coefficients + running stats, backward
// reductions -> dgamma/dbeta + apply coefficients), device-side stream gates, weight packing (fp32 master -> bf16 kernel layouts),
// fp8 delayed scaling.  (The optimizer is eae_optim.hip.)
#include "eae_internal.h"
#include "eae_common.hip.h"
#include "eae_misc.h"


// Sum the partials of ONE channel: part = [2][C][ntiles] (channel-major, so the reads are contiguous); 256 threads stride
// over the tiles with fp64 accumulation, then a fixed-order reduction: xor-butterfly inside each wave (every lane ends with
// the wave's sum), the four wave sums added in wave order -> bitwise reproducible, one barrier instead of a 9-step LDS tree.
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ void reduce_partials_ch(const float* __restrict__ part, int ntiles, int C, int ch, double* red,
                                                   double& a, double& b) {
  const int tid = threadIdx.x;
  const float* p1 = part + (size_t)ch * ntiles;
  const float* p2 = part + ((size_t)C + ch) * ntiles;
  double s1 = 0.0, s2 = 0.0;
  for (int t = tid; t < ntiles; t += 256) { s1 += (double)p1[t]; s2 += (double)p2[t]; }
  s1 = wave_sum_f64(s1); s2 = wave_sum_f64(s2);
  if ((tid & 63) == 0) { red[tid >> 6] = s1; red[4 + (tid >> 6)] = s2; }
  __syncthreads();
  a = ((red[0] + red[1]) + red[2]) + red[3];
  b = ((red[4] + red[5]) + red[6]) + red[7];
}

// ---------------------------------------------------------------------------------------------------------------
// BatchNorm forward finalize.  part = [2][C][ntiles] (sum y, sum y^2) -> coef [4][C] = s, t, mean, invstd
//   s = gamma*invstd, t = beta - mean*s  so that  BN(y) = s*y + t           (nn.BatchNorm2d, eps 1e-5, R.md:293)
// running_mean/var updated with momentum (unbiased variance), num_batches_tracked += 1   
// grid = C blocks (one channel each) of 256 threads.
// ---------------------------------------------------------------------------------------------------------------
__global__ EAE_NO_PK __launch_bounds__(256) void bn_finalize_kernel(const float* __restrict__ part, int ntiles, int C, float count,
                                                           const float* __restrict__ gamma, const float* __restrict__ beta,
                                                           float* running_mean, float* running_var, long long* nbt,
                                                           float momentum, float eps, float* __restrict__ coef) {
  __shared__ double red[512];
  const int tid = threadIdx.x;
  const int ch = blockIdx.x;
  double a, b;
  reduce_partials_ch(part, ntiles, C, ch, red, a, b);
  if (tid == 0) {
    double mean = a / count;
    double var = b / count - mean * mean;
    if (var < 0.0) var = 0.0;
    float invstd = 1.0f / sqrtf((float)var + eps);
    float s = gamma[ch] * invstd;
    coef[ch] = s;
    coef[C + ch] = beta[ch] - (float)mean * s;
    coef[2 * C + ch] = (float)mean;
    coef[3 * C + ch] = invstd;
    if (running_mean) {
      double unb = count > 1.f ? var * (double)count / ((double)count - 1.0) : var;
      running_mean[ch] = (1.f - momentum) * running_mean[ch] + momentum * (float)mean;
      running_var[ch] = (1.f - momentum) * running_var[ch] + momentum * (float)unb;
    }
  }
  if (nbt && blockIdx.x == 0 && tid == 0) *nbt += 1;
}

// eval mode: coefficients from the running statistics
struct BnEvalCoefArgs { int C; const float* gamma; const float* beta; const float* rm; const float* rv; float eps; float* coef; };
__device__ __forceinline__ EAE_NO_PK void bn_eval_coef_body(const BnEvalCoefArgs& a) {
  const int C = a.C;
  int ch = blockIdx.x * blockDim.x + threadIdx.x;
  if (ch >= C) return;
  float invstd = 1.0f / sqrtf(a.rv[ch] + a.eps);
  float s = a.gamma[ch] * invstd;
  a.coef[ch] = s;
  a.coef[C + ch] = a.beta[ch] - a.rm[ch] * s;
  a.coef[2 * C + ch] = a.rm[ch];
  a.coef[3 * C + ch] = invstd;
}
__global__ EAE_NO_PK void bn_eval_coef_kernel(BnEvalCoefArgs a) { bn_eval_coef_body(a); }
__global__ EAE_NO_PK void bn_eval_coef_kernel_g(GroupPack<BnEvalCoefArgs> p, int gz) { bn_eval_coef_body(group_args<BnEvalCoefArgs>(gz)); }

// BatchNorm backward finalize.  part = [2][C][ntiles] (sum g, sum g*xhat), g = ReLU-masked upstream gradient.
//   dbeta = sum g ; dgamma = sum g*xhat ;  dy = A*g + B*y + Cc  with
//   A = gamma*invstd, B = -A*invstd*dgamma/N, Cc = -A*dbeta/N + A*invstd*mean*dgamma/N   (native_batch_norm_backward)
__global__ EAE_NO_PK __launch_bounds__(256) void bn_bwd_finalize_kernel(const float* __restrict__ part, int ntiles, int C, float count,
                                                               const float* __restrict__ gamma, const float* __restrict__ coef_fwd,
                                                               float* dgamma, float* dbeta, float* __restrict__ coef_bwd) {
  __shared__ double red[512];
  const int tid = threadIdx.x;
  const int ch = blockIdx.x;
  double a, b;
  reduce_partials_ch(part, ntiles, C, ch, red, a, b);
  if (tid == 0) {
    float db = (float)a, dg = (float)b;
    if (dbeta) dbeta[ch] = db;
    if (dgamma) dgamma[ch] = dg;
    float mean = coef_fwd[2 * C + ch], invstd = coef_fwd[3 * C + ch];
    float A = gamma[ch] * invstd;
    float Bc = -A * invstd * dg / count;
    coef_bwd[ch] = A;
    coef_bwd[C + ch] = Bc;
    coef_bwd[2 * C + ch] = -A * db / count - Bc * mean;
  }
}

// SyncBN form of the backward finalize, split at the point where the replicas exchange their sums (dp.py):
//   reduce: part -> sums[2][C] in fp64 (this replica's sum g, sum g*xhat) and its LOCAL dgamma / dbeta (the gradient exchange sums them)
//   coef  : A, B, C from the GLOBAL sums (after the all-reduce) and the global element count
__global__ EAE_NO_PK __launch_bounds__(256) void bn_bwd_reduce_kernel(const float* __restrict__ part, int ntiles, int C, double* __restrict__ sums,
                                                             float* dgamma, float* dbeta) {
  __shared__ double red[512];
  const int ch = blockIdx.x;
  double a, b;
  reduce_partials_ch(part, ntiles, C, ch, red, a, b);
  if (threadIdx.x == 0) {
    sums[ch] = a; sums[C + ch] = b;
    if (dbeta) dbeta[ch] = (float)a;
    if (dgamma) dgamma[ch] = (float)b;
  }
}
__global__ EAE_NO_PK void bn_bwd_coef_kernel(const double* __restrict__ sums, int C, float count, const float* __restrict__ gamma,
                                             const float* __restrict__ coef_fwd, float* __restrict__ coef_bwd) {
  const int ch = blockIdx.x * blockDim.x + threadIdx.x;
  if (ch >= C) return;
  const float db = (float)sums[ch], dg = (float)sums[C + ch];
  const float mean = coef_fwd[2 * C + ch], invstd = coef_fwd[3 * C + ch];
  const float A = gamma[ch] * invstd;
  const float Bc = -A * invstd * dg / count;
  coef_bwd[ch] = A;
  coef_bwd[C + ch] = Bc;
  coef_bwd[2 * C + ch] = -A * db / count - Bc * mean;
}
int eae_launch_bn_bwd_reduce(hipStream_t st, const float* part, int ntiles, int C, double* sums, float* dgamma, float* dbeta) {
  EAE_NO_GROUP("bn_bwd_reduce_kernel");
  hipLaunchKernelGGL(bn_bwd_reduce_kernel, dim3(C), dim3(256), 0, st, part, ntiles, C, sums, dgamma, dbeta);
  EAE_LAUNCH_CHECK();
  return 0;
}
int eae_launch_bn_bwd_coef(hipStream_t st, const double* sums, int C, long long count, const float* gamma, const float* coef_fwd,
                           float* coef_bwd) {
  EAE_NO_GROUP("bn_bwd_coef_kernel");
  hipLaunchKernelGGL(bn_bwd_coef_kernel, dim3((C + 63) / 64), dim3(64), 0, st, sums, C, (float)count, gamma, coef_fwd, coef_bwd);
  EAE_LAUNCH_CHECK();
  return 0;
}

int eae_launch_bn_finalize(hipStream_t st, const float* part, int ntiles, int C, long long count, const float* gamma,
                           const float* beta, float* rm, float* rv, long long* nbt, float momentum, float eps, float* coef) {
  EAE_NO_GROUP("bn_finalize_kernel");
  hipLaunchKernelGGL(bn_finalize_kernel, dim3(C), dim3(256), 0, st, part, ntiles, C, (float)count, gamma, beta, rm,
                     rv, nbt, momentum, eps, coef);
  EAE_LAUNCH_CHECK();
  return 0;
}
int eae_launch_bn_eval_coef(hipStream_t st, int C, const float* gamma, const float* beta, const float* rm, const float* rv,
                            float eps, float* coef) {
  const BnEvalCoefArgs ba = {C, gamma, beta, rm, rv, eps, coef};
  eae_launch(bn_eval_coef_kernel, bn_eval_coef_kernel_g, dim3((C + 63) / 64), dim3(64), 0, st, ba);
  EAE_LAUNCH_CHECK();
  return 0;
}
int eae_launch_bn_bwd_finalize(hipStream_t st, const float* part, int ntiles, int C, long long count, const float* gamma,
                               const float* coef_fwd, float* dgamma, float* dbeta, float* coef_bwd) {
  EAE_NO_GROUP("bn_bwd_finalize_kernel");
  hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3(C), dim3(256), 0, st, part, ntiles, C, (float)count, gamma,
                     coef_fwd, dgamma, dbeta, coef_bwd);
  EAE_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// Device-side stream dependencies.  gate_kernel: one lane polls up to 4 progress words (relaxed agent-scope loads, s_sleep
// between polls) until each has reached its value; the kernels behind it on the same stream then see everything the signalling
// stream had completed when it published the value (kernel-boundary acquire).  Values only grow (wrap-safe signed compare).
// The spin is bounded by WALL-CLOCK time (s_memrealtime, 100 MHz; default 30 s, EAE_GATE_TIMEOUT_MS): a caller's stream that is
// stalled for seconds in front of the step (a late data-parallel peer inside the previous step's all-reduce, a long copy) is waited
// for.  A gate that does give up records the value it was waiting for in the STICKY word `timeout`: the work behind it then ran too
// early, so every later optimizer kernel of the context refuses to update the parameters and writes NaN losses
// (adam_kernel `bad`), the steppers raise (eae_gate_timeouts()).  signal_kernel publishes a value from a stream that has no other
// kernel to carry it.
// ---------------------------------------------------------------------------------------------------------------
__global__ EAE_NO_PK __launch_bounds__(64) void gate_kernel(GateArgs g) {
  if (threadIdx.x == 0) gate_wait(g);
}
__global__ EAE_NO_PK __launch_bounds__(64) void gate_kernel_g(GroupPack<GateArgs> p, int gz) {      // grouped twins (eae_group.h): one wave per member
  if (threadIdx.x == 0) gate_wait(group_args<GateArgs>(gz));
}
struct SignalArgs { unsigned* word; unsigned val; };
__global__ EAE_NO_PK void signal_kernel(SignalArgs a) {
  if (threadIdx.x == 0 && blockIdx.x == 0) __hip_atomic_store(a.word, a.val, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__global__ EAE_NO_PK void signal_kernel_g(GroupPack<SignalArgs> p, int gz) {
  const SignalArgs a = group_args<SignalArgs>(gz);
  if (threadIdx.x == 0 && blockIdx.x == 0) __hip_atomic_store(a.word, a.val, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
int eae_launch_gate(hipStream_t st, const GateArgs& g) {
  eae_launch(gate_kernel, gate_kernel_g, dim3(1), dim3(64), 0, st, g);
  EAE_LAUNCH_CHECK();
  return 0;
}
int eae_launch_signal(hipStream_t st, unsigned* word, unsigned val) {
  const SignalArgs sa = {word, val};
  eae_launch(signal_kernel, signal_kernel_g, dim3(1), dim3(64), 0, st, sa);
  EAE_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// Weight packing: one launch converts every fp32 master weight into the bf16 layouts the kernels read.
// ---------------------------------------------------------------------------------------------------------------
// (32-bit unsigned index arithmetic: destination and source element counts stay below 2^32, and a 64-bit division costs ~5x a
// 32-bit one on this target -- the all-64-bit version of this kernel took 14 us per step)
__device__ __forceinline__ float pack_fetch(const PackDesc& d, const float* __restrict__ src, unsigned i) {
  const unsigned d0 = (unsigned)d.d0, d1 = (unsigned)d.d1, d2 = (unsigned)d.d2;
  switch (d.mode) {
    case PACK_3x3_P1: {   // dst [A][9][B]  <- src [A][B][3][3]
      unsigned b = i % d1, r = i / d1, tap = r % 9u, a = r / 9u;
      return src[(a * d1 + b) * 9u + tap];
    }
    case PACK_3x3_P2: {   // dst [B][9][A]  <- src [A][B][3][3]
      unsigned a = i % d0, r = i / d0, tap = r % 9u, b = r / 9u;
      return src[(a * d1 + b) * 9u + tap];
    }
    case PACK_K27: {      // dst [A][32] with k = tap*3 + c (zero for k >= 27)  <- src [A][3][3][3]
      unsigned k = i & 31u, a = i >> 5;
      if (k >= 27u) return 0.f;
      unsigned tap = k / 3u, c = k % 3u;
      return src[(a * 3u + c) * 9u + tap];
    }
    case PACK_KCP: {      // dst [A][KP] with k = tap*CP + c, KP = 9*CP padded to 32 (zero for c >= C and k >= 9*CP)  <- src [A][C][3][3]
      // (d1 = C, d2 = CP; edge_conv_kernel.  CP = 4: dst [A][64])
      const unsigned KP = (9u * d2 + 31u) & ~31u, k = i % KP, a = i / KP, tap = k / d2, c = k % d2;
      if (tap >= 9u || c >= d1) return 0.f;
      return src[(a * d1 + c) * 9u + tap];
    }
    case PACK_DECONV4_JOINT: {   // dst [16*NT][128]: n = phase*C+co, k = nb*32+ci  <- src [32 ci][C co][3][3]   (d1 = C)
      int k = i & 127; int n = i >> 7;
      const int C = (int)d1;
      if (n >= 4 * C) return 0.f;
      int ph = n / C, co = n % C, nb = k >> 5, ci = k & 31;
      int py = ph >> 1, px = ph & 1, dy = nb >> 1, dx = nb & 1;
      int ky = py == 0 ? (dy == 0 ? 1 : -1) : (dy == 0 ? 2 : 0);
      int kx = px == 0 ? (dx == 0 ? 1 : -1) : (dx == 0 ? 2 : 0);
      if (ky < 0 || kx < 0) return 0.f;
      return src[(ci * C + co) * 9 + ky * 3 + kx];
    }
    // FC modes: d0 = latent width PADDED to a multiple of 64, d.lv = the real width (rows / columns >= lv are zero; the source
    // tensor has lv of them)
    case PACK_FC_ROWMAJOR_KPERM: {   // dst [R][K'] with k' = p*Cc + c  <- src [R][K] with k = c*P + p   (d0=R, d1=Cc, d2=P)
      unsigned K = d1 * d2, k2 = i % K, r = i / K;
      if (r >= (unsigned)d.lv) return 0.f;
      unsigned c = k2 % d1, p = k2 / d1;
      return src[r * K + c * d2 + p];
    }
    case PACK_FC_TRANS_KPERM: {      // dst [K'][R]  <- src [R][K]   (transpose + permute)
      unsigned r = i % d0, k2 = i / d0, K = d1 * d2;
      if (r >= (unsigned)d.lv) return 0.f;
      unsigned c = k2 % d1, p = k2 / d1;
      return src[r * K + c * d2 + p];
    }
    case PACK_FC_ROWPERM: {          // dst [J'][L] with j' = p*Cc + c <- src [J][L] with j = c*P + p   (d0=L, d1=Cc, d2=P)
      unsigned l = i % d0, j2 = i / d0;
      if (l >= (unsigned)d.lv) return 0.f;
      unsigned c = j2 % d1, p = j2 / d1;
      return src[(c * d2 + p) * (unsigned)d.lv + l];
    }
    case PACK_FC_ROWPERM_TRANS: {    // dst [L][J']  <- src [J][L]
      unsigned J = d1 * d2, j2 = i % J, l = i / J;
      if (l >= (unsigned)d.lv) return 0.f;
      unsigned c = j2 % d1, p = j2 / d1;
      return src[(c * d2 + p) * (unsigned)d.lv + l];
    }
    case PACK_PAD_COLS: {            // dst [R][d0] <- src [R][lv], zero beyond column lv
      unsigned l = i % d0, r = i / d0;
      return l < (unsigned)d.lv ? src[r * (unsigned)d.lv + l] : 0.f;
    }
    default: return src[i];          // PACK_COPY
  }
}

// Destination of one pack descriptor: a window over its bytes (the stores of a workgroup are spread over the whole layout, so the
// window is the descriptor's, not a tile's).  A destination of 2 GiB or more -- element counts go up to 2^32 -- keeps plain pointer
// stores: `big` is uniform over the launch's workgroups of that descriptor.
struct PackOut {
  OutRsrc o; uint8_t* base; bool big;
  __device__ __forceinline__ void init(uint8_t* b, size_t bytes) { base = b; big = bytes >= (size_t)OOB_OFF; o.init(b, big ? 0 : (long)bytes); }
  __device__ __forceinline__ void put16(size_t off, const uint4& v) const { if (big) *reinterpret_cast<uint4*>(base + off) = v; else o.st16<EAE_WT_OPT>((uint32_t)off, v); }
  __device__ __forceinline__ void put4(size_t off, float v) const { if (big) *reinterpret_cast<float*>(base + off) = v; else o.st4<EAE_WT_OPT>((uint32_t)off, v); }
  __device__ __forceinline__ void put2(size_t off, uint16_t v) const { if (big) *reinterpret_cast<uint16_t*>(base + off) = v; else o.st2<EAE_WT_OPT>((uint32_t)off, v); }
  __device__ __forceinline__ void put1(size_t off, uint8_t v) const { if (big) base[off] = v; else o.st1<EAE_WT_OPT>((uint32_t)off, v); }
};
struct PackAllArgs { const PackDesc* descs; const float* params; uint8_t* pack_base; Fp8State* q; unsigned* clear_word; const unsigned short* blkmap; int blk_begin; };
__device__ __forceinline__ EAE_NO_PK void pack_all_body(const PackAllArgs& pa) {
  const PackDesc* __restrict__ descs = pa.descs; const float* __restrict__ params = pa.params; uint8_t* __restrict__ pack_base = pa.pack_base;
  Fp8State* __restrict__ q = pa.q; unsigned* __restrict__ clear_word = pa.clear_word;
  // the workgroup's descriptor and its place among the descriptor's workgroups: 2-D launch (y = descriptor, the same number of
  // workgroups for each) or flattened (blkmap: a descriptor has as many workgroups as its work needs -- the 2-D form spent most of its
  // workgroups on the ~20 small descriptors while a handful looped over the four 262 K-element projections)
  const bool flat = pa.blkmap != nullptr;
  const unsigned gb = flat ? (unsigned)pa.blk_begin + blockIdx.x : 0u;
  const PackDesc d = descs[flat ? (unsigned)pa.blkmap[gb] : blockIdx.y];
  const unsigned bx = flat ? gb - (unsigned)d.blk0 : blockIdx.x, nbx = flat ? (unsigned)d.nblk : gridDim.x;
  if (clear_word != nullptr && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) *clear_word = 0u;
  const float* src = params + d.src_off;
  const unsigned count = (unsigned)d.count;
  PackOut po;
  po.init(pack_base + d.dst_off, (size_t)count * (d.q_layer >= 0 ? 1u : d.out_f32 ? 4u : 2u));
  if (d.q_layer >= 0) {        // e4m3 bytes = sat(w * s_w); also reports max |w| for the next step's scale (delayed scaling)
    const float sw = q->s_w[d.q_layer];
    float mx = 0.f;
    for (unsigned i = bx * 256u + threadIdx.x; i < count; i += nbx * 256u) {
      const float v = pack_fetch(d, src, i);
      mx = fmaxf(mx, fabsf(v));
      const float sv = fminf(fmaxf(v * sw, -448.f), 448.f);
      po.put1(i, (uint8_t)(__builtin_amdgcn_cvt_pk_fp8_f32(sv, 0.f, 0, false) & 0xff));
    }
#pragma unroll
    for (int sh = 32; sh >= 1; sh >>= 1) mx = fmaxf(mx, __shfl_xor(mx, sh));
    if ((threadIdx.x & 63) == 0 && mx > 0.f) atomicMax(&q->amax_w[d.q_layer][((bx * 4 + (threadIdx.x >> 6)) & (FP8_AMAX_SLOTS - 1)) * FP8_AMAX_STRIDE], __float_as_uint(mx));
    return;
  }
  if ((d.mode == PACK_3x3_P1 || d.mode == PACK_3x3_P2) && !d.out_f32) {
    // 3x3 weights W[a][b][3][3]: one thread per (a, b) reads its 9 consecutive floats and writes them one tap-row apart; the lanes of
    // a wave run over b for P1 = [a][9][b] and over a for P2 = [b][9][a], so every store instruction of a wave is contiguous and
    // every source line is read once (the element-per-thread mapping gathered one float per line and lane for P2)
    const unsigned A = (unsigned)d.d0, Bq = (unsigned)d.d1;
    const bool p1 = d.mode == PACK_3x3_P1;
    for (unsigned t = bx * 256u + threadIdx.x; t < A * Bq; t += nbx * 256u) {
      const unsigned a = p1 ? t / Bq : t % A, b = p1 ? t % Bq : t / A;
      const float* sp = src + ((size_t)a * Bq + b) * 9;
      float w[9];
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) w[tap] = sp[tap];
#pragma unroll
      for (int tap = 0; tap < 9; ++tap)
        po.put2((p1 ? ((size_t)a * 9 + tap) * Bq + b : ((size_t)b * 9 + tap) * A + a) * 2, (uint16_t)f2bf(w[tap]));
    }
    return;
  }
  if (d.mode == PACK_FC_ROWPERM_TRANS && !d.out_f32 && (unsigned)d.d2 * ((unsigned)d.d1 / 64) * ((unsigned)d.d0 / 64) >= 1024u) {
    // dec.fc's transposed layout dst[l][p*Cc + c] <- src[(c*P + p)][l]: 64 x 64 tiles through LDS (rows of the source are read whole,
    // rows of the destination are written in 128-byte pieces); element-per-thread gathers one float per source line and lane.
    // Only for the big shapes (>= 1024 tiles: 256x256 inputs): at 64x64 the 64 tiles are too few blocks (11.4 vs 8.9 us per step).
    // (round 4: 16-byte loads and 16-byte stores -- a thread converts 8 consecutive destination elements -- instead of one float per
    //  lane in and one bf16 per lane out: a 2-byte store costs ~12x a 16-byte one per byte, the kernel was store-instruction-bound)
    __shared__ float tile[64][65];
    const unsigned Lp = (unsigned)d.d0, Cc = (unsigned)d.d1, P = (unsigned)d.d2, lv = (unsigned)d.lv, J = Cc * P;
    const unsigned ncc = Cc / 64, nlc = Lp / 64, ntiles = P * ncc * nlc;
    const bool vec = (lv & 3u) == 0;
    for (unsigned tl = bx; tl < ntiles; tl += nbx) {
      const unsigned lc = tl % nlc, cch = (tl / nlc) % ncc, p = tl / (nlc * ncc);
      const unsigned c0 = cch * 64, l0 = lc * 64;
      __syncthreads();
#pragma unroll
      for (unsigned k = 0; k < 4; ++k) {         // 64 rows (ci) x 16 float4 (l)
        const unsigned idx = threadIdx.x + 256u * k, l4 = (idx & 15u) * 4u, ci = idx >> 4;
        const float* sp = src + ((size_t)(c0 + ci) * P + p) * lv + l0 + l4;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (vec && l0 + l4 + 3 < lv) v = *reinterpret_cast<const float4*>(sp);
        else { if (l0 + l4 < lv) v.x = sp[0]; if (l0 + l4 + 1 < lv) v.y = sp[1]; if (l0 + l4 + 2 < lv) v.z = sp[2]; if (l0 + l4 + 3 < lv) v.w = sp[3]; }
        tile[ci][l4] = v.x; tile[ci][l4 + 1] = v.y; tile[ci][l4 + 2] = v.z; tile[ci][l4 + 3] = v.w;
      }
      __syncthreads();
#pragma unroll
      for (unsigned k = 0; k < 2; ++k) {         // 64 destination rows (l) x 8 pieces of 8 consecutive channels
        const unsigned idx = threadIdx.x + 256u * k, c8 = (idx & 7u) * 8u, l = idx >> 3;
        uint4 o;
        o.x = pack2(tile[c8][l], tile[c8 + 1][l]); o.y = pack2(tile[c8 + 2][l], tile[c8 + 3][l]);
        o.z = pack2(tile[c8 + 4][l], tile[c8 + 5][l]); o.w = pack2(tile[c8 + 6][l], tile[c8 + 7][l]);
        po.put16(((size_t)(l0 + l) * J + (size_t)p * Cc + c0 + c8) * 2, o);
      }
    }
    return;
  }
  if ((d.mode == PACK_FC_ROWMAJOR_KPERM || d.mode == PACK_FC_TRANS_KPERM) && !d.out_f32 && (d.d2 & 63) == 0 && (d.d1 & 63) == 0 && (d.d0 & 63) == 0 &&
      (unsigned)d.d0 * ((unsigned)d.d1 / 64) * ((unsigned)d.d2 / 64) >= 1024u) {
    // enc.fc's two layouts on the big shapes (256x256 inputs: 16.7 M weights, P = 256 positions): 64 x 64 tiles through LDS.
    //   row-major form  dst[r][p*Cc + c] <- src[r][c*P + p]: for one r, a tile of 64 channels x 64 positions;
    //   transposed form dst[p*Cc + c][r] <- src[r][c*P + p]: for one c, a tile of 64 rows x 64 positions.
    // Either way the source is read in 256-byte runs along p and the destination written in 128-byte runs (the thread-per-(r, c)
    // mapping below touches 64 source lines per load instruction: 256 us of the 2.1 ms config-5 step went into this kernel).
    __shared__ float tile[64][65];
    const unsigned R = (unsigned)d.d0, Cc = (unsigned)d.d1, P = (unsigned)d.d2, K = Cc * P, lv = (unsigned)d.lv;
    const bool rowmajor = d.mode == PACK_FC_ROWMAJOR_KPERM;
    const unsigned npc = P / 64, nA = rowmajor ? Cc / 64 : R / 64, nfix = rowmajor ? R : Cc, ntiles = nfix * nA * npc;
    for (unsigned tl = bx; tl < ntiles; tl += nbx) {
      const unsigned pc = tl % npc, ac = (tl / npc) % nA, fix = tl / (npc * nA);
      const unsigned p0 = pc * 64, a0 = ac * 64;                 // a = channel (row-major form) or row (transposed form)
      __syncthreads();
#pragma unroll
      for (unsigned k = 0; k < 4; ++k) {         // 64 rows (a) x 16 float4 along p (16-byte loads: see the transposed dec.fc form above)
        const unsigned idx = threadIdx.x + 256u * k, p4 = (idx & 15u) * 4u, ai = idx >> 4;
        const unsigned r = rowmajor ? fix : a0 + ai, c = rowmajor ? a0 + ai : fix;
        const float4 v = r < lv ? *reinterpret_cast<const float4*>(src + (size_t)r * K + (size_t)c * P + p0 + p4) : make_float4(0.f, 0.f, 0.f, 0.f);
        tile[ai][p4] = v.x; tile[ai][p4 + 1] = v.y; tile[ai][p4 + 2] = v.z; tile[ai][p4 + 3] = v.w;
      }
      __syncthreads();
#pragma unroll
      for (unsigned k = 0; k < 2; ++k) {         // 64 destination rows (p) x 8 pieces of 8 consecutive a
        const unsigned idx = threadIdx.x + 256u * k, a8 = (idx & 7u) * 8u, pp = idx >> 3;
        uint4 o;
        o.x = pack2(tile[a8][pp], tile[a8 + 1][pp]); o.y = pack2(tile[a8 + 2][pp], tile[a8 + 3][pp]);
        o.z = pack2(tile[a8 + 4][pp], tile[a8 + 5][pp]); o.w = pack2(tile[a8 + 6][pp], tile[a8 + 7][pp]);
        const size_t oo = rowmajor ? (size_t)fix * K + (size_t)(p0 + pp) * Cc + a0 + a8
                                   : ((size_t)(p0 + pp) * Cc + fix) * R + a0 + a8;
        po.put16(oo * 2, o);
      }
    }
    return;
  }
  if ((d.mode == PACK_FC_ROWMAJOR_KPERM || d.mode == PACK_FC_TRANS_KPERM) && (d.d2 & 3) == 0 && !d.out_f32) {
    // enc.fc's two layouts (k' = p*Cc + c <- k = c*P + p).  One thread per (row r, channel c) reads its P consecutive source floats
    // (whole cache lines, each read once) and writes them P rows apart; the lanes of a wave run over c (row-major form) or over r
    // (transposed form), so every store instruction of a wave covers 128 contiguous bytes.  The element-per-thread mapping of
    // pack_fetch reads one float per 64-byte line and lane: 16x the L2 traffic for these two packs.
    const unsigned R = (unsigned)d.d0, Cc = (unsigned)d.d1, P = (unsigned)d.d2, K = Cc * P, lv = (unsigned)d.lv;
    const bool rowmajor = d.mode == PACK_FC_ROWMAJOR_KPERM;
    for (unsigned t = bx * 256u + threadIdx.x; t < R * Cc; t += nbx * 256u) {
      const unsigned r = rowmajor ? t / Cc : t % R, c = rowmajor ? t % Cc : t / R;
      const float* sp = src + (size_t)r * K + (size_t)c * P;
      for (unsigned p = 0; p < P; p += 4) {
        const float4 v = r < lv ? *reinterpret_cast<const float4*>(sp + p) : make_float4(0.f, 0.f, 0.f, 0.f);
        const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (unsigned q = 0; q < 4; ++q) {
          const size_t o = rowmajor ? (size_t)r * K + (size_t)(p + q) * Cc + c : ((size_t)(p + q) * Cc + c) * R + r;
          po.put2(o * 2, (uint16_t)f2bf(e[q]));
        }
      }
    }
    return;
  }
  if (d.mode == PACK_FC_ROWPERM && !d.out_f32 && (d.lv & 7) == 0 && (d.d0 & 7) == 0) {
    // dec.fc's row-permuted layout dst[p*Cc + c][l] <- src[c*P + p][l]: whole rows move, so a thread takes 8 consecutive l (two 16-byte
    // loads, one 16-byte store) instead of one float in and one bf16 out (16.7 M elements at 256x256 inputs)
    const unsigned Lp = (unsigned)d.d0, Cc = (unsigned)d.d1, P = (unsigned)d.d2, lv = (unsigned)d.lv, n8 = count / 8u, l8n = Lp / 8u;
    for (unsigned i = bx * 256u + threadIdx.x; i < n8; i += nbx * 256u) {
      const unsigned l = (i % l8n) * 8u, j2 = i / l8n, cc = j2 % Cc, pp = j2 / Cc;
      uint4 o = make_uint4(0, 0, 0, 0);
      if (l < lv) {
        const float4* sp = reinterpret_cast<const float4*>(src + (size_t)(cc * P + pp) * lv + l);
        const float4 a = sp[0], b = sp[1];
        o.x = pack2(a.x, a.y); o.y = pack2(a.z, a.w); o.z = pack2(b.x, b.y); o.w = pack2(b.z, b.w);
      }
      po.put16((size_t)i * 16u, o);
    }
    return;
  }
  for (unsigned i = bx * 256u + threadIdx.x; i < count; i += nbx * 256u) {
    float v = pack_fetch(d, src, i);
    if (d.out_f32) po.put4((size_t)i * 4u, v);
    else po.put2((size_t)i * 2u, (uint16_t)f2bf(v));
  }
}
__global__ EAE_NO_PK __launch_bounds__(256) void pack_all_kernel(PackAllArgs a) { pack_all_body(a); }
__global__ EAE_NO_PK __launch_bounds__(256) void pack_all_kernel_g(GroupPack<PackAllArgs> p, int gz) { pack_all_body(group_args<PackAllArgs>(gz)); }

int eae_launch_pack_all(hipStream_t st, const PackDesc* descs_dev, int ndesc, const float* params, void* pack_base, Fp8State* q, unsigned* clear_word,
                        int blocks_per_desc) {
  const PackAllArgs pa = {descs_dev, params, (uint8_t*)pack_base, q, clear_word, nullptr, 0};
  if (blocks_per_desc <= 0) blocks_per_desc = 256;
  // member of a grouped step: the launch carries eae_geo_mult members' descriptors (8 x 256 x ~20 workgroups, most of them with a few
  // hundred elements, took 54 us: the dispatch of 41 K workgroups, not the 62 MB they move)
  if (eae_geo_mult > 1) blocks_per_desc = blocks_per_desc / eae_geo_mult > 16 ? blocks_per_desc / eae_geo_mult : 16;
  eae_launch(pack_all_kernel, pack_all_kernel_g, dim3(blocks_per_desc, ndesc), dim3(256), 0, st, pa);
  EAE_LAUNCH_CHECK();
  return 0;
}

// Workgroups of a descriptor in the flattened launch: one pass of its loop per workgroup (2048 destination elements, one 64 x 64
// tile, 256 (a, b) pairs of a 3 x 3 weight, 256 (row, channel) pairs of a projection), at most 1024.
static int pack_desc_blocks(const PackDesc& d) {
  long long items;
  const bool big_rpt = d.mode == PACK_FC_ROWPERM_TRANS && !d.out_f32 && (long long)d.d2 * (d.d1 / 64) * (d.d0 / 64) >= 1024;
  const bool big_kp = (d.mode == PACK_FC_ROWMAJOR_KPERM || d.mode == PACK_FC_TRANS_KPERM) && !d.out_f32 && (d.d2 & 63) == 0 && (d.d1 & 63) == 0 &&
                      (d.d0 & 63) == 0 && (long long)d.d0 * (d.d1 / 64) * (d.d2 / 64) >= 1024;
  if (d.q_layer >= 0) items = (d.count + 2047) / 2048;
  else if ((d.mode == PACK_3x3_P1 || d.mode == PACK_3x3_P2) && !d.out_f32) items = ((long long)d.d0 * d.d1 + 255) / 256;
  else if (big_rpt) items = (long long)d.d2 * (d.d1 / 64) * (d.d0 / 64);
  else if (big_kp) items = (long long)d.d0 * (d.d1 / 64) * (d.d2 / 64);
  else if ((d.mode == PACK_FC_ROWMAJOR_KPERM || d.mode == PACK_FC_TRANS_KPERM) && (d.d2 & 3) == 0 && !d.out_f32) items = ((long long)d.d0 * d.d1 + 255) / 256;
  else items = (d.count + 2047) / 2048;
  if (items < 1) items = 1;
  if (items > 1024) items = 1024;
  return (int)items;
}
int eae_pack_assign_blocks(PackDesc* descs, int ndesc, unsigned short* blkmap, int cap) {
  int tot = 0;
  for (int i = 0; i < ndesc; ++i) {
    descs[i].blk0 = tot; descs[i].nblk = pack_desc_blocks(descs[i]);
    for (int b = 0; b < descs[i].nblk; ++b) { if (tot + b >= cap) return -1; blkmap[tot + b] = (unsigned short)i; }
    tot += descs[i].nblk;
  }
  return tot;
}
int eae_launch_pack_flat(hipStream_t st, const PackDesc* descs_all, const unsigned short* blkmap, int blk_begin, int blk_count, const float* params,
                         void* pack_base, Fp8State* q, unsigned* clear_word) {
  if (blk_count <= 0) return 0;
  const PackAllArgs pa = {descs_all, params, (uint8_t*)pack_base, q, clear_word, blkmap, blk_begin};
  eae_launch(pack_all_kernel, pack_all_kernel_g, dim3(blk_count), dim3(256), 0, st, pa);
  EAE_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// fp8 variant: delayed scaling.  Once per step (after every kernel that reads the current scales has finished) the scales of
// the NEXT step are derived from the maxima this step's kernels reported:  s = 2^floor(log2(MAX / (2 * amax)))  (a factor 2 of
// head room because the operand of the next step is not the one measured), MAX = 448 (e4m3: activations, weights) or 57344
// (e5m2: gradients).  A tensor whose maximum is 0 or not finite keeps its scale.  The maxima are cleared for the next step.
// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float fp8_scale_from(unsigned amax_bits, float maxv, float keep) {
  const float amax = __uint_as_float(amax_bits);
  if (!(amax > 0.f) || !(amax < 3.0e38f)) return keep;
  const float e = floorf(log2f(maxv / (2.f * amax)));
  return exp2f(fminf(fmaxf(e, -60.f), 60.f));
}
__global__ EAE_NO_PK void fp8_scales_kernel(Fp8State* q) {
  static_assert(FP8_AMAX_SLOTS % 64 == 0, "whole rounds of one slot per lane");
  const int lane = threadIdx.x;
  unsigned ma[6], mg[6], mw[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    ma[i] = mg[i] = mw[i] = 0u;
#pragma unroll
    for (int s0 = 0; s0 < FP8_AMAX_SLOTS; s0 += 64) {
      const int w_ = (s0 + lane) * FP8_AMAX_STRIDE;
      const unsigned a_ = q->amax_act[i][w_], g_ = q->amax_grad[i][w_], x_ = q->amax_w[i][w_];
      ma[i] = a_ > ma[i] ? a_ : ma[i]; mg[i] = g_ > mg[i] ? g_ : mg[i]; mw[i] = x_ > mw[i] ? x_ : mw[i];
      q->amax_act[i][w_] = 0; q->amax_grad[i][w_] = 0; q->amax_w[i][w_] = 0;
    }
#pragma unroll
    for (int sh = 32; sh >= 1; sh >>= 1) {       // (non-negative float bits order like unsigned integers)
      const unsigned a = __shfl_xor(ma[i], sh), g = __shfl_xor(mg[i], sh), w = __shfl_xor(mw[i], sh);
      ma[i] = a > ma[i] ? a : ma[i]; mg[i] = g > mg[i] ? g : mg[i]; mw[i] = w > mw[i] ? w : mw[i];
    }
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    if (lane != i) continue;
    q->s_act[i] = fp8_scale_from(ma[i], 448.f, q->s_act[i]);
    q->s_grad[i] = fp8_scale_from(mg[i], 57344.f, q->s_grad[i]);
    q->s_w[i] = fp8_scale_from(mw[i], 448.f, q->s_w[i]);
    const float sa = q->s_act[i], sg = q->s_grad[i], sw = q->s_w[i];
    q->qs_fwd[i][0] = 1.f / sa; q->qs_fwd[i][1] = 1.f / (sa * sw);
    q->qs_bwd[i][0] = 1.f / sg; q->qs_bwd[i][1] = 1.f / (sg * sw);
    // weight gradient: conv layers (i < 3): small operand = output gradient, big = input activation; transposed layers: the reverse
    const float ss = i < 3 ? sg : sa, sb = i < 3 ? sa : sg;
    q->qs_wg[i][0] = 1.f / ss; q->qs_wg[i][1] = 1.f / sb; q->qs_wg[i][2] = 1.f / (ss * sb); q->qs_wg[i][3] = 0.f;
  }
}
int eae_launch_fp8_scales(hipStream_t st, Fp8State* q) {
  EAE_NO_GROUP("fp8_scales_kernel");
  hipLaunchKernelGGL(fp8_scales_kernel, dim3(1), dim3(64), 0, st, q);
  EAE_LAUNCH_CHECK();
  return 0;
}
void eae_fp8_state_init(Fp8State* h) {
  *h = Fp8State();
  for (int i = 0; i < 6; ++i) {
    h->s_act[i] = h->s_grad[i] = h->s_w[i] = 1.f;
    h->qs_fwd[i][0] = h->qs_fwd[i][1] = h->qs_bwd[i][0] = h->qs_bwd[i][1] = 1.f;
    h->qs_wg[i][0] = h->qs_wg[i][1] = h->qs_wg[i][2] = 1.f;
  }
}
