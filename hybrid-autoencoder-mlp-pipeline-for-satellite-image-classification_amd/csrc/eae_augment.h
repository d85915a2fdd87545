#pragma once
// The augmentation policy of the staging calls (include/eae.h, "augmentation policy") as the kernels of eae_augment.hip read it, and
// their launchers.
#include "eae_internal.h"

struct StageAug {
  int dihedral;                        // draw rot from the geometric call
  int affine_on, radio_on;             // the policy draws (a, b) / gains and offsets
  float rot_lo, rot_w, sc_lo, sc_w;    // uniforms as (lo, hi - lo): theta in degrees, sigma
  float g_lo, g_w, bg_lo, bg_w, of_lo, of_w;
  const int* geom;                     // explicit draws, or nullptr
  const float* affine;
  const float* radio;
  int lds;                             // 1: the per-image draws are made once per workgroup
};
// Validates the policy and the explicit draws for H x W images; *active = 0 when the call is the plain one (nothing to do here).
int eae_stage_aug_prepare(const eae_aug* aug, const int* geom, const float* affine, const float* radio, int H, int W, const char* who,
                          StageAug* out, int* active);
int eae_launch_augment_aug(hipStream_t st, const void* in_u8, float* out, int B, int H, int W, float std, unsigned long long seed,
                           unsigned long long step, const StageAug& aug, const float* noise);
int eae_launch_stage_bands_aug(hipStream_t st, const void* src, int elem_bytes, long long N, int C, int H, int W, const long long* index,
                               int B, const float* divisor, float* out, float std, unsigned long long seed, unsigned long long step,
                               const StageAug& aug, const float* noise);
// the scene already checked (eae_scene_stage_windows_aug, eae_scene.hip); nW, nwin: its grid
int eae_launch_scene_stage_aug(hipStream_t st, const eae_scene* s, long long nW, long long nwin, const long long* windows, int B,
                               float* out, float std, unsigned long long seed, unsigned long long step, const StageAug& aug,
                               const float* noise, int crop);
