// Internal (non-ABI) declarations shared by the translation units of libeae.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/eae.h"

int eae_set_error(int code, const char* msg);   // records the message for eae_last_error(), returns code

struct ConvArgs;
int eae_launch_conv_s2(const ConvArgs& a, int cin, int cout, int src, int epi, hipStream_t st);
int eae_launch_deconv_s2(const ConvArgs& a, int cin, int cout, int src, int epi, hipStream_t st);
int eae_conv_s2_ntiles(int kind, int cin, int cout, int B, int Hin, int Win);   // statistics partials per channel of that launch (-1: no geometry)

#define EAE_HIP(x) do { hipError_t e__ = (x); if (e__ != hipSuccess) return eae_set_error(-3, hipGetErrorString(e__)); } while (0)
#define EAE_LAUNCH_CHECK() do { hipError_t e__ = hipGetLastError(); if (e__ != hipSuccess) return eae_set_error(-3, hipGetErrorString(e__)); } while (0)

// Raise a kernel's dynamic-LDS limit once per (kernel, device): the attribute belongs to the device's code object, so a
// process-wide "done" flag would skip it for a context created later on another device.
#include <utility>
#include <vector>
inline hipError_t eae_smem_attr(const void* func, size_t bytes) {
  static thread_local std::vector<std::pair<const void*, int>> done;
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  for (const auto& d : done) if (d.first == func && d.second == dev) return hipSuccess;
  e = hipFuncSetAttribute(func, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  if (e == hipSuccess) done.emplace_back(func, dev);
  return e;
}

#include "eae_group.h"
#include "eae_misc.h"
#include "eae_optim.h"
#include "eae_head.h"
// optional bracket around the MAIN kernel of a launcher that enqueues more than one (weight gradient + slice reduction)
struct EaeProfHook { void (*begin)(void* user, hipStream_t st); void (*end)(void* user, hipStream_t st); void* user; };
struct SrcDesc;
struct EdgeArgs; struct Deconv4Args; struct WgradArgs; struct FcNtArgs; struct FcTnArgs;
int eae_launch_edge_conv(hipStream_t st, int src3_kind, int epi, const EdgeArgs& a);
struct SceneSrc;
int eae_launch_edge_conv_scene(hipStream_t st, int src3_kind, const EdgeArgs& a, const SceneSrc& s);
// eval-mode MLP over rows x[b * ldx ..] (b < B) of windows win0.. of a scene (or windows index[win0 ..]): probs [K][plane] (column =
// window), labels [plane] (argmax)
int eae_mlp_predict(eae_mlp* m, hipStream_t st, const float* x, int ldx, int B, long long win0, long long plane, float* probs,
                    long long* labels, const long long* index = nullptr);
int eae_mlp_dims(const eae_mlp* m, int* input_dim, int* classes, int* max_batch);
// eae_scene.hip: argument checks (-> window grid nH x nW), conv1 source kind and kernel-side description of a scene
int eae_scene_check(const eae_scene* s, long long* nH, long long* nW);
int eae_scene_src3_kind(const eae_scene* s);
void eae_scene_fill_src(const eae_scene* s, long long nW, long long first, SceneSrc* out);
long long eae_scene_extent(long long n, int patch, int stride);   // (n - 1) * S + P: the pixels a grid of n windows spans on one axis
int eae_edge_tiles(int B, int H, int W);
int eae_launch_edge_wgrad(hipStream_t st, int src3_kind, const void* src3, int B, int H, int W, const SrcDesc& side, int smode,
                          float* scratch, long long scratch_floats, float* dw, const EaeProfHook* hook = nullptr,
                          const struct BnBwdFold* bfold = nullptr, unsigned* sig = nullptr, unsigned sig_val = 0,
                          int (*mid)(void*, GateArgs*) = nullptr, void* mid_user = nullptr, int C = 3);
int eae_launch_deconv4_loss(hipStream_t st, int smode, const Deconv4Args& a);
// deconv4 + sigmoid against windows of a scene (eval mode, BNRELU source): per-tile per-band squared-error partials into r.part, and
// with r.recon set the owned pixels of the stitched x_hat (and residual) raster; windows s.first + n, or s.index[s.first + n]
struct Deconv4SceneArgs;
int eae_launch_deconv4_scene(hipStream_t st, int src3_kind, const Deconv4Args& a, const SceneSrc& s, const Deconv4SceneArgs& r);
// err[w] = mean over the C * P * P elements of window w of the launch (w = first + n, or index[first + n]; n < B), band_err[c][w] (or
// nullptr) the mean over band c; part as eae_launch_deconv4_scene left it.  An id outside [0, nwin) is skipped.
int eae_launch_scene_err_finalize(hipStream_t st, const float* part, int B, int P, int C, long long first, const long long* index,
                                  long long nwin, float* err, float* band_err);
int eae_launch_wgrad_s2(hipStream_t st, const WgradArgs& a, int cs, int cb, int smode, int bmode, float* scratch,
                        long long scratch_floats, float* dw, const EaeProfHook* hook = nullptr);
// out[i] = scale * sum_s part[s][i] over float4 elements i < n4 (reduce_slices_kernel, eae_wgrad.hip.h), for callers outside the kernel units
int eae_launch_reduce_slices(hipStream_t st, const float* part, int nslices, long n4, float* out, float scale);
int eae_launch_fc_nt(hipStream_t st, const FcNtArgs& a, int amode, int epi, int ksplit);
int eae_launch_fc_reduce(hipStream_t st, const float* part, int nsl, int M, int N, const float* bias, const float* addend,
                         const float* addend2, float* out);
int eae_launch_sigmoid_bwd(hipStream_t st, const float* x_hat, const float* dx_hat, void* g4, float* part, int B, int H, int W, int C = 3);
int eae_launch_fc_tn(hipStream_t st, const FcTnArgs& a, int pmode, int qmode);
