// The optimizer unit (eae_optim.hip): fused multi-tensor Adam over the flat fp32 arenas and the global gradient-norm clipping in front of it.
#pragma once
#include <hip/hip_runtime.h>

// global gradient-norm clipping (eae_set_grad_clip): the partials of eae_launch_grad_sumsq and what the optimizer launch behind it
// does with them; part == nullptr = the plain optimizer kernels
constexpr int EAE_CLIP_MAX_PARTS = 512;
struct EaeClip { const double* part; int nparts; float max_norm; float* norm_out; };
int eae_grad_sumsq_parts(long long n);
// sum of squares over the 38 tensors at poff39[s] .. + sizes38[s] of the gradient arena `g` -> eae_grad_sumsq_parts(poff39[38]) partials
int eae_launch_grad_sumsq(hipStream_t st, const float* g, const long long* poff39, const long long* sizes38, double* part);

// One optimizer launch over the first n elements (a multiple of 4) of the arenas.
struct AdamLaunch {
  float* p = nullptr; const float* g = nullptr; float* m = nullptr; float* v = nullptr;
  long long n = 0;
  double lr = 0.0, b1 = 0.9, b2 = 0.999, eps = 1e-8, wd = 0.0;
  long long step = 1;                  // bias correction 1 - b^step
  float gscale = 1.0f;                 // the gradient is gscale * g (1 / world for summed data-parallel gradients)
  void* zero_buf = nullptr; long long zero_bytes = 0;      // side job: clear this buffer (the step's accumulators)
  const unsigned* bad = nullptr;       // device words, non-zero = no update and NaN into nan_out[0..2]: stale (a gate timed out) ...
  const unsigned* bad2 = nullptr;      // ... and diverged (a non-finite norm under `clip` counts as diverged too)
  float* nan_out = nullptr;
  int nan_fill = 0;                    // a diverged step writes NaN into p, m and v (eae_config.nan_exact)
  int max_blocks = 0;                  // 0: 2048; the grid-stride loop covers the rest
  EaeClip clip = {nullptr, 0, 0.f, nullptr};
  // non-null: lr / bias_correction1 and sqrt(bias_correction2) are read from dyn[0], dyn[1] on the device (eae_launch_set_dyn), so that
  // a captured launch can be replayed while the step count advances; lr and step are not used.  Never part of a grouped step.
  const float* dyn = nullptr;
};
int eae_launch_adam(hipStream_t st, const AdamLaunch& a);
int eae_launch_set_dyn(hipStream_t st, float* dyn, double lr, double b1, double b2, long long step);
