// The optimizer: global gradient-norm clipping (sum-of-squares partials, clip coefficient) and the fused multi-tensor Adam, one kernel
// body for the eager, grouped, clipped and graph-replayed steps.
#include "eae_internal.h"
#include "eae_common.hip.h"

// ---------------------------------------------------------------------------------------------------------------
// Fused multi-tensor Adam over the flat fp32 arenas (torch.optim.Adam defaults, R.md:624; L2 decay for the MLP, R.md:2625)
//   g += wd*p ; m = b1*m + (1-b1)*g ; v = b2*v + (1-b2)*g*g ; p -= step_size * m / (sqrt(v)/sqrt(bc2) + eps)
// ---------------------------------------------------------------------------------------------------------------
// One element of the update with every rounding step written out (no fp contraction left to the compiler): the eager step and the
// replayed step must agree bit for bit (tests/test_gpu_ae.py::test_graph_replay_equals_eager, tests/test_gpu_graph_optimizer.py), and a
// refactoring must not move a rounding -- round 4 found the compiler fusing  b2*v + ((1-b2)*g)*g  as fma(g, t, b2*v) in one of the
// then two kernel bodies and as fma(b2, v, g*t) in the other after the first was turned into an inlined body.  There is ONE body now
// (adam_body), and one gradient expression in it, fma(g, geff, wd * p).  The replayed step used to compute fma(wd, p, g) with wd = 0
// where the eager step computed fma(g, 1, 0 * p): for finite p both add the same two terms, g and the signed zero 0 * p, exactly
// (g + (+-0) is g, and -0 only when both are -0), so taking the eager form moved no bit of the replay.
__device__ __forceinline__ EAE_NO_PK void adam_update(float& p, float gj, float& m, float& v, float b1, float b2, float step_size, float bc2_sqrt, float eps) {
#pragma clang fp contract(off)
  m = __builtin_fmaf(1.f - b1, gj - m, m);                   // exp_avg.lerp_(grad, 1-beta1)
  const float t = (1.f - b2) * gj;
  v = __builtin_fmaf(b2, v, gj * t);                         // mul_(beta2).addcmul_(grad, grad, 1-beta2)
  const float denom = sqrtf(v) / bc2_sqrt + eps;
  p = __builtin_fmaf(-step_size, m / denom, p);
}
struct AdamArgs {
  float* p; const float* g; float* m; float* v; long n4; float b1, b2;
  // the per-step scalars by value, or (adam_body<CLIP, true>) where to read them: step_size = dyn[0], bc2_sqrt = dyn[1].  One or the
  // other, in the same 8 bytes: the argument block of the eager kernels keeps its size and its offsets
  union { struct { float step_size, bc2_sqrt; }; const float* dyn; };
  float eps, wd, gscale; uint4* zbuf; long zn16;
  const unsigned* bad; const unsigned* bad2; float* nan_out; int nan_fill;
};
static_assert(sizeof(AdamArgs) == 120, "the grouped twins stride over the kernel arguments by this size");

// ---- global gradient-norm clipping (eae_set_grad_clip)
// grad_sumsq_kernel leaves GradNormArgs-many fp64 partial sums of g^2 in a workspace; EVERY workgroup of the optimizer kernel behind it
// adds them in one fixed order (the idiom of the weighted head kernel's W), so all of them hold the same bits of
//   total = s * sqrt(sum g^2)      coef = min(1, max_norm / (total + 1e-6))      (torch.nn.utils.clip_grad_norm_, norm_type 2)
// and Adam consumes fma(g, fl32(s * coef), wd * p): with coef == 1 the unclipped arithmetic.  No atomics, nothing depends on the
// optimizer's grid (eae_launch_adam shrinks it for a member of a grouped step).
struct ClipArgs { const double* part; int nparts; float max_norm; float* norm_out; };
struct AdamClipArgs { AdamArgs a; ClipArgs c; };
struct ClipCoef { float coef; bool finite; };

// sum of 256 per-thread fp64 values in a fixed order, the same value in every thread: lanes by xor-butterfly (each level adds the
// same pairs in every lane, and fp64 addition commutes), then the four waves 0 + 1 + 2 + 3
__device__ __forceinline__ double block_sum_fixed(double v, double* lds4) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if ((threadIdx.x & 63) == 0) lds4[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((lds4[0] + lds4[1]) + lds4[2]) + lds4[3];
}
__device__ __forceinline__ EAE_NO_PK ClipCoef clip_coef(const ClipArgs& ca, float gscale) {
#pragma clang fp contract(off)
  __shared__ double lds4[4];
  double v = 0.0;
  for (int i = threadIdx.x; i < ca.nparts; i += 256) v += ca.part[i];
  const double ss = block_sum_fixed(v, lds4);
  const float total = (float)((double)gscale * sqrt(ss));
  const float coef = fminf(1.0f, ca.max_norm / (total + 1e-6f));
  if (ca.norm_out != nullptr && blockIdx.x == 0 && threadIdx.x == 0) { ca.norm_out[0] = total; ca.norm_out[1] = coef; }
  ClipCoef r; r.coef = coef; r.finite = total - total == 0.0f;      // (inf - inf and NaN - NaN are NaN)
  return r;
}

// CLIP: scale the gradient by the clip coefficient of *ca.  DYN: the per-step scalars (lr / bias_correction1, sqrt(bias_correction2))
// are read from device memory, so that a captured hipGraph of the whole train step can be replayed while the step count advances.
// A template parameter, not a test of aa.dyn: the eager kernels compile to what they compiled to without it.  The replayed step
// has never had the two side jobs (its own memset clears the accumulators, nan_fill is not honoured: DESIGN.md section 19); they are
// compiled out of its kernels.
template <bool CLIP, bool DYN> __device__ __forceinline__ EAE_NO_PK void adam_body(const AdamArgs& aa, const ClipArgs* ca = nullptr) {
  float* __restrict__ p = aa.p; const float* __restrict__ g = aa.g; float* __restrict__ m = aa.m; float* __restrict__ v = aa.v;
  const long n4 = aa.n4; const float b1 = aa.b1, b2 = aa.b2, eps = aa.eps, wd = aa.wd, gscale = aa.gscale;
  float step_size = DYN ? 0.f : aa.step_size, bc2_sqrt = DYN ? 0.f : aa.bc2_sqrt;      // (DYN: read behind the refuse check)
  uint4* __restrict__ zbuf = aa.zbuf; const long zn16 = aa.zn16;
  const unsigned* __restrict__ bad = aa.bad; const unsigned* __restrict__ bad2 = aa.bad2; float* __restrict__ nan_out = aa.nan_out;
  const int nan_fill = aa.nan_fill;
  // side job: clear the BatchNorm statistics accumulators for the next step (every consumer of this step has finished)
  // (the stores of this kernel go through per-round windows of 256 pieces: the round's first piece is wave-uniform, a piece past the
  //  end of the arena lies behind the window's end and is dropped by the hardware)
  if constexpr (!DYN)
  for (long i0 = (long)blockIdx.x * 256; i0 < zn16; i0 += (long)gridDim.x * 256) {
    OutRsrc oz;
    oz.init(zbuf + i0, ((zn16 - i0) < 256 ? (zn16 - i0) : 256) * 16);
    oz.st16<EAE_WT_OPT>(threadIdx.x * 16u, make_uint4(0, 0, 0, 0));
  }
  // a side-stream gate of this context has timed out at some point (sticky word): gradients may have been computed from stale
  // activations -- no update, and the step's loss scalars become NaN so that the run cannot go on unnoticed
  const bool stale = bad != nullptr && __hip_atomic_load(bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u;
  bool diverged = bad2 != nullptr && __hip_atomic_load(bad2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u;
  float geff = gscale;
  if constexpr (CLIP) {      // norm_out is written also when the update is refused; a non-finite norm refuses it (diverged)
    const ClipCoef cc = clip_coef(*ca, gscale);
    diverged = diverged || !cc.finite;
    geff = gscale * cc.coef;
  }
  if (stale || diverged) {
    if (nan_out != nullptr && blockIdx.x == 0 && threadIdx.x < 3) nan_out[threadIdx.x] = __builtin_nanf("");
    // nan_fill (eae_config.nan_exact / EAE_NAN_EXACT=1): a DIVERGED step does to the replica what it does to the reference's model --
    // loss.backward() on a non-finite loss hands every parameter a NaN gradient and Adam writes NaN into the parameter and both moments
    // (R.md:653-654); the default leaves the last finite parameters in place.  Never for a stale step.
    if (!DYN && nan_fill && diverged && !stale) {
      const float4 nn = make_float4(__builtin_nanf(""), __builtin_nanf(""), __builtin_nanf(""), __builtin_nanf(""));
      for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        reinterpret_cast<float4*>(p)[i] = nn; reinterpret_cast<float4*>(m)[i] = nn; reinterpret_cast<float4*>(v)[i] = nn;
      }
    }
    return;
  }
  if constexpr (DYN) { step_size = aa.dyn[0]; bc2_sqrt = aa.dyn[1]; }
  for (long i0 = (long)blockIdx.x * 256; i0 < n4; i0 += (long)gridDim.x * 256) {      // one window of 256 pieces per round and arena
    const long i = i0 + threadIdx.x;
    if (i >= n4) break;
    const long wb = ((n4 - i0) < 256 ? (n4 - i0) : 256) * 16;
    OutRsrc op, om, ov;
    op.init(p + i0 * 4, wb); om.init(m + i0 * 4, wb); ov.init(v + i0 * 4, wb);
    float4 pp = reinterpret_cast<float4*>(p)[i];
    float4 gg = reinterpret_cast<const float4*>(g)[i];
    float4 mm = reinterpret_cast<float4*>(m)[i];
    float4 vv = reinterpret_cast<float4*>(v)[i];
    float* P = &pp.x; float* G = &gg.x; float* M = &mm.x; float* V = &vv.x;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float wp = wd * P[j];
      adam_update(P[j], __builtin_fmaf(G[j], CLIP ? geff : gscale, wp), M[j], V[j], b1, b2, step_size, bc2_sqrt, eps);
    }
    op.st16<EAE_WT_OPT>(threadIdx.x * 16u, pp);
    om.st16<EAE_WT_OPT>(threadIdx.x * 16u, mm);
    ov.st16<EAE_WT_OPT>(threadIdx.x * 16u, vv);
  }
}
__global__ EAE_NO_PK __launch_bounds__(256) void adam_kernel(AdamArgs a) { adam_body<false, false>(a); }
__global__ EAE_NO_PK __launch_bounds__(256) void adam_kernel_g(GroupPack<AdamArgs> p, int gz) { adam_body<false, false>(group_args<AdamArgs>(gz)); }
__global__ EAE_NO_PK __launch_bounds__(256) void adam_clip_kernel(AdamClipArgs a) { adam_body<true, false>(a.a, &a.c); }
__global__ EAE_NO_PK __launch_bounds__(256) void adam_clip_kernel_g(GroupPack<AdamClipArgs> p, int gz) {
  const AdamClipArgs a = group_args<AdamClipArgs>(gz);
  adam_body<true, false>(a.a, &a.c);
}
__global__ EAE_NO_PK __launch_bounds__(256) void adam_dyn_kernel(AdamArgs a) { adam_body<false, true>(a); }
__global__ EAE_NO_PK __launch_bounds__(256) void adam_dyn_clip_kernel(AdamClipArgs a) { adam_body<true, true>(a.a, &a.c); }
__global__ EAE_NO_PK void set_dyn_kernel(float* dyn, float step_size, float bc2_sqrt) { dyn[0] = step_size; dyn[1] = bc2_sqrt; }

// Sum of squares of the 38 gradient tensors, fp64, one partial per workgroup.  The arena is caller-owned and every tensor is rounded
// up to 4 elements: the 1..3 padding floats behind a tensor must not count.  They sit in the tensor's LAST 16-byte piece only, so the
// segment table shrinks to the few pieces that hold padding (tail[k] = piece index * 4 + valid elements; ntail <= 38, 3 at most for
// this model: enc.fc.bias [L], deconv4.bias [bands], classifier.2.bias [C]) and every other piece is summed whole.  Thread t of the
// grid takes pieces t, t + T, ...: four independent 16-byte loads in flight per round; the grid is a function of the arena length
// alone, so which elements a partial covers is too.
struct GradNormArgs { const float* g; double* part; unsigned n4; int ntail; unsigned tail[38]; };
__device__ __forceinline__ EAE_NO_PK void grad_sumsq_body(const GradNormArgs& a) {
#pragma clang fp contract(off)
  __shared__ double lds4[4];
  const unsigned T = gridDim.x * 256u, t = blockIdx.x * 256u + threadIdx.x, n4 = a.n4;
  const float4* __restrict__ g4 = reinterpret_cast<const float4*>(a.g);
  double acc = 0.0;
  for (unsigned i0 = t; i0 < n4; i0 += 4u * T) {      // (n4 < 2^30 and T <= 2^17: no wrap)
    float4 q[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {      // (past the end: piece n4 - 1 again, counted with 0 valid elements below)
      const unsigned i = i0 + (unsigned)u * T;
      q[u] = g4[i < n4 ? i : n4 - 1];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const unsigned i = i0 + (unsigned)u * T;
      unsigned valid = i < n4 ? 4u : 0u;
      for (int k = 0; k < a.ntail; ++k) if ((a.tail[k] >> 2) == i) valid = a.tail[k] & 3u;
      const double x = valid > 0 ? q[u].x : 0.f, y = valid > 1 ? q[u].y : 0.f, z = valid > 2 ? q[u].z : 0.f, w = valid > 3 ? q[u].w : 0.f;
      acc += x * x; acc += y * y; acc += z * z; acc += w * w;
    }
  }
  const double tot = block_sum_fixed(acc, lds4);
  if (threadIdx.x == 0) a.part[blockIdx.x] = tot;
}
__global__ EAE_NO_PK __launch_bounds__(256) void grad_sumsq_kernel(GradNormArgs a) { grad_sumsq_body(a); }
// (the member's block is read in place: a copy indexed with the run-time k of the tail loop would live in scratch)
__global__ EAE_NO_PK __launch_bounds__(256) void grad_sumsq_kernel_g(GroupPack<GradNormArgs> p, int gz) {
  const char* base = (const char*)__builtin_amdgcn_kernarg_segment_ptr();
  grad_sumsq_body(*reinterpret_cast<const GradNormArgs*>(base + (size_t)(blockIdx.z / (unsigned)gz) * sizeof(GradNormArgs)));
}

int eae_launch_set_dyn(hipStream_t st, float* dyn, double lr, double b1, double b2, long long step) {
  double bc1 = 1.0 - pow(b1, (double)step), bc2 = 1.0 - pow(b2, (double)step);
  EAE_NO_GROUP("set_dyn_kernel");
  hipLaunchKernelGGL(set_dyn_kernel, dim3(1), dim3(1), 0, st, dyn, (float)(lr / bc1), (float)sqrt(bc2));
  EAE_LAUNCH_CHECK();
  return 0;
}

int eae_launch_adam(hipStream_t st, const AdamLaunch& a) {
  if (a.n % 4) return eae_set_error(-2, "adam: arena length must be a multiple of 4");
  const bool dyn = a.dyn != nullptr;
  if (dyn) EAE_NO_GROUP("adam_dyn_kernel");
  double bc1 = 1.0 - pow(a.b1, (double)a.step), bc2 = 1.0 - pow(a.b2, (double)a.step);
  long n4 = a.n / 4;
  int blocks = (int)((n4 + 255) / 256);
  const int max_blocks = a.max_blocks > 0 ? a.max_blocks : 2048;
  if (blocks > max_blocks) blocks = max_blocks;
  if (eae_geo_mult > 1) blocks = blocks / eae_geo_mult > 64 ? blocks / eae_geo_mult : (blocks < 64 ? blocks : 64);      // member of a grouped step
  AdamArgs aa = {a.p, a.g, a.m, a.v, n4, (float)a.b1, (float)a.b2, {{(float)(a.lr / bc1), (float)sqrt(bc2)}}, (float)a.eps, (float)a.wd,
                 a.gscale, (uint4*)a.zero_buf, (long)(a.zero_bytes / 16), a.bad, a.bad2, a.nan_out, a.nan_fill};
  if (dyn) aa.dyn = a.dyn;      // (in place of the two scalars by value)
  const AdamClipArgs ac = {aa, {a.clip.part, a.clip.nparts, a.clip.max_norm, a.clip.norm_out}};
  const dim3 grid(blocks), block(256);
  if (dyn) {
    if (a.clip.part) hipLaunchKernelGGL(adam_dyn_clip_kernel, grid, block, 0, st, ac);
    else hipLaunchKernelGGL(adam_dyn_kernel, grid, block, 0, st, aa);
  } else if (a.clip.part) eae_launch(adam_clip_kernel, adam_clip_kernel_g, grid, block, 0, st, ac);
  else eae_launch(adam_kernel, adam_kernel_g, grid, block, 0, st, aa);
  EAE_LAUNCH_CHECK();
  return 0;
}

// number of fp64 partials grad_sumsq_kernel writes for an arena of n elements: one workgroup per 4096 elements, 512 at the most
int eae_grad_sumsq_parts(long long n) {
  const long long b = (n + 4095) / 4096;
  return (int)(b < 1 ? 1 : b > EAE_CLIP_MAX_PARTS ? EAE_CLIP_MAX_PARTS : b);
}
int eae_launch_grad_sumsq(hipStream_t st, const float* g, const long long* poff39, const long long* sizes38, double* part) {
  GradNormArgs a = GradNormArgs();
  a.g = g; a.part = part;
  if (poff39[0] != 0 || poff39[38] <= 0 || poff39[38] >= (1LL << 32)) return eae_set_error(-2, "grad norm: arena of 1 .. 2^32 - 1 elements");
  for (int s = 0; s < 38; ++s) {
    if (sizes38[s] <= 0 || poff39[s + 1] != poff39[s] + ((sizes38[s] + 3) & ~3LL))
      return eae_set_error(-2, "grad norm: every tensor must be followed by its padding to 4 elements and the next tensor");
    if (sizes38[s] % 4) a.tail[a.ntail++] = (unsigned)((poff39[s] + sizes38[s]) / 4 * 4 + sizes38[s] % 4);
  }
  a.n4 = (unsigned)(poff39[38] / 4);
  eae_launch(grad_sumsq_kernel, grad_sumsq_kernel_g, dim3(eae_grad_sumsq_parts(poff39[38])), dim3(256), 0, st, a);
  EAE_LAUNCH_CHECK();
  return 0;
}
