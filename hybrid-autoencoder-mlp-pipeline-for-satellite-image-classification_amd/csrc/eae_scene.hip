// Scene classification helpers (include/eae.h, "scene classification"): the window gather (the public way to get patches, and the
// reference the fused conv1 scene source is tested against) and the cell blend of window probabilities.  Neither uses matrix
// instructions, so both are built with packed FP32 disabled (EAE_NO_PK, tests/test_isa_guard.py).
#include "eae_internal.h"
#include "eae_common.hip.h"
#include "eae_edge.hip.h"

namespace {

// out[b][c][y][x] = scene[c][oy + y][ox + x] / divisor[c] for window first + b; one thread per output pixel, all bands
template <typename T>
__global__ EAE_NO_PK __launch_bounds__(256) void scene_windows_kernel(const T* __restrict__ src, const float* __restrict__ divisor, int C,
                                                                  long long plane, int Ws, int P, int S, int nW, long long first, int B,
                                                                  float* __restrict__ out) {
  const long long pp = (long long)P * P;
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= pp * B) return;
  const long long b = p / pp, r = p - b * pp;
  const int y = (int)(r / P), x = (int)(r - (long long)y * P);
  const long long w = first + b, wi = w / nW, wj = w - wi * nW;
  const T* q = src + (wi * S + y) * (long long)Ws + wj * S + x;
  for (int c = 0; c < C; ++c) out[(b * C + c) * pp + r] = scene_val(q[c * plane], divisor[c]);
}

// cell (ci, cj) of the [nH + k - 1][nW + k - 1] map: mean over windows i in [ci - k + 1, ci] x j in [cj - k + 1, cj] inside the grid
__global__ EAE_NO_PK __launch_bounds__(256) void scene_blend_kernel(const float* __restrict__ probs, int K, int nH, int nW, int k,
                                                                float* __restrict__ cell, long long* __restrict__ cell_labels) {
  const int cH = nH + k - 1, cW = nW + k - 1;
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= (long long)cH * cW) return;
  const int ci = (int)(p / cW), cj = (int)(p - (long long)ci * cW);
  const int i0 = ci - k + 1 > 0 ? ci - k + 1 : 0, i1 = ci < nH - 1 ? ci : nH - 1;
  const int j0 = cj - k + 1 > 0 ? cj - k + 1 : 0, j1 = cj < nW - 1 ? cj : nW - 1;
  const float cnt = (float)((i1 - i0 + 1) * (j1 - j0 + 1));
  const long long wplane = (long long)nH * nW, cplane = (long long)cH * cW;
  float mx = 0.f;
  int am = 0;
  for (int c = 0; c < K; ++c) {
    const float* q = probs + c * wplane;
    float s = 0.f;
    for (int i = i0; i <= i1; ++i)
      for (int j = j0; j <= j1; ++j) s += q[(long long)i * nW + j];
    const float v = s / cnt;
    cell[c * cplane + p] = v;
    if (c == 0 || v > mx) { mx = v; am = c; }
  }
  cell_labels[p] = am;
}

}  // namespace

int eae_scene_check(const eae_scene* s, long long* nH, long long* nW) {
  if (!s) return eae_set_error(EAE_ERR_ARG, "scene: NULL scene");
  if (!s->data) return eae_set_error(EAE_ERR_ARG, "scene: NULL data");
  if (!s->divisor) return eae_set_error(EAE_ERR_ARG, "scene: NULL divisor");
  if (s->dtype != EAE_SCENE_U8 && s->dtype != EAE_SCENE_U16 && s->dtype != EAE_SCENE_F32)
    return eae_set_error(EAE_ERR_ARG, "scene: dtype must be EAE_SCENE_U8, EAE_SCENE_U16 or EAE_SCENE_F32");
  if (s->C < 1 || s->C > 16) return eae_set_error(EAE_ERR_ARG, "scene: in_channels must be in 1..16");
  if (s->patch <= 0 || s->patch % 64) return eae_set_error(EAE_ERR_ARG, "scene: the patch size must be a positive multiple of 64");
  if (s->H < s->patch || s->W < s->patch) return eae_set_error(EAE_ERR_ARG, "scene: smaller than one window");
  if (s->stride < 1 || s->stride > s->patch) return eae_set_error(EAE_ERR_ARG, "scene: stride must be in 1..patch");
  *nH = (s->H - s->patch) / s->stride + 1;
  *nW = (s->W - s->patch) / s->stride + 1;
  return 0;
}

int eae_scene_src3_kind(const eae_scene* s) {
  return s->dtype == EAE_SCENE_U8 ? SRC3_SCENE_U8 : s->dtype == EAE_SCENE_U16 ? SRC3_SCENE_U16 : SRC3_SCENE_F32;
}

void eae_scene_fill_src(const eae_scene* s, long long nW, long long first, SceneSrc* out) {
  out->data = s->data; out->div = s->divisor; out->first = first; out->plane = (long long)s->H * s->W;
  out->Ws = s->W; out->S = s->stride; out->nW = (int)nW;
}

extern "C" int eae_scene_windows(void* stream, const eae_scene* s, long long first, int B, float* out) {
  long long nH = 0, nW = 0;
  if (int rc = eae_scene_check(s, &nH, &nW)) return rc;
  if (!out) return eae_set_error(EAE_ERR_ARG, "scene_windows: NULL output");
  if (B <= 0 || first < 0 || first + B > nH * nW) return eae_set_error(EAE_ERR_ARG, "scene_windows: windows outside the grid");
  EAE_NO_GROUP("scene_windows_kernel");
  const hipStream_t st = (hipStream_t)stream;
  const long long plane = (long long)s->H * s->W, tot = (long long)B * s->patch * s->patch;
  const dim3 grid((unsigned)((tot + 255) / 256));
  if (s->dtype == EAE_SCENE_U8)
    hipLaunchKernelGGL(scene_windows_kernel<uint8_t>, grid, dim3(256), 0, st, (const uint8_t*)s->data, s->divisor, s->C, plane, s->W,
                       s->patch, s->stride, (int)nW, first, B, out);
  else if (s->dtype == EAE_SCENE_U16)
    hipLaunchKernelGGL(scene_windows_kernel<uint16_t>, grid, dim3(256), 0, st, (const uint16_t*)s->data, s->divisor, s->C, plane, s->W,
                       s->patch, s->stride, (int)nW, first, B, out);
  else
    hipLaunchKernelGGL(scene_windows_kernel<float>, grid, dim3(256), 0, st, (const float*)s->data, s->divisor, s->C, plane, s->W,
                       s->patch, s->stride, (int)nW, first, B, out);
  EAE_LAUNCH_CHECK();
  return 0;
}

extern "C" int eae_scene_blend(void* stream, const float* probs, int K, int nH, int nW, int k, float* cell, long long* cell_labels) {
  if (!probs || !cell || !cell_labels) return eae_set_error(EAE_ERR_ARG, "scene_blend: NULL argument");
  if (K < 1 || nH < 1 || nW < 1 || k < 1) return eae_set_error(EAE_ERR_ARG, "scene_blend: bad shape");
  EAE_NO_GROUP("scene_blend_kernel");
  const long long tot = (long long)(nH + k - 1) * (nW + k - 1);
  hipLaunchKernelGGL(scene_blend_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, (hipStream_t)stream, probs, K, nH, nW, k,
                     cell, cell_labels);
  EAE_LAUNCH_CHECK();
  return 0;
}
