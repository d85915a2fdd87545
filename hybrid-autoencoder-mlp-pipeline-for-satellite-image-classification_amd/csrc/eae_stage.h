#pragma once
// Staging (eae_stage.hip): what a launch of the one staging kernel reads, its launchers, and the random stream of its draws.
#include "eae_internal.h"

struct StageAug {
  int fixed;                           // train = 0: nothing is drawn -- flip 0, top = left = 4, rot 0 (and the launcher passes std 0)
  int dihedral;                        // draw rot from the geometric call
  int affine_on, radio_on;             // the policy draws (a, b) / gains and offsets
  float rot_lo, rot_w, sc_lo, sc_w;    // uniforms as (lo, hi - lo): theta in degrees, sigma
  float g_lo, g_w, bg_lo, bg_w, of_lo, of_w;
  const int* geom;                     // explicit draws, or nullptr: rows of geom_stride ints, (flip, top, left[, rot])
  int geom_stride;                     // 4: the policy calls' geom; 3: the plain calls' params (rot = 0)
  const float* affine;
  const float* radio;
  int lds;                             // 1: the per-image draws are made once per workgroup; ignored by a PLAIN launch (per thread)
};
// Validates the policy and the explicit draws for H x W images.
int eae_stage_aug_prepare(const eae_aug* aug, const int* geom, const float* affine, const float* radio, int H, int W, const char* who,
                          StageAug* out);
// a plain call: no policy, explicit (flip, top, left) rows in `params` [B][3] or nullptr
StageAug eae_stage_plain(const int* params);
// The plain launchers (eae_augment, eae_stage_bands: eae_ops.hip), and what they and the policy entry points share.  train = 0: the
// division only, whatever the policy.
int eae_launch_augment(hipStream_t st, const void* in_u8, float* out, int B, int H, int W, int train, float std, unsigned long long seed,
                       unsigned long long step, const int* params, const float* noise);
int eae_launch_stage_bands(hipStream_t st, const void* src, int elem_bytes, long long N, int C, int H, int W, const long long* index, int B,
                           const float* divisor, float* out, int train, float std, unsigned long long seed, unsigned long long step,
                           const int* params, const float* noise);
// the scene and the other arguments already checked (eae_scene_stage_windows[_aug], eae_scene.hip); nW, nwin: its grid
int eae_launch_scene_stage(hipStream_t st, const eae_scene* s, long long nW, long long nwin, const long long* windows, int B, float* out,
                           int train, float std, unsigned long long seed, unsigned long long step, const StageAug& aug, const float* noise,
                           int crop);
// the plain scene call (eae_scene_stage_windows): its own kernel, kept for its speed (eae_stage.hip); params [B][3] or nullptr
int eae_launch_scene_stage_plain(hipStream_t st, const eae_scene* s, long long nW, long long nwin, const long long* windows, int B,
                                 float* out, int train, float std, unsigned long long seed, unsigned long long step, const int* params,
                                 const float* noise, int crop);

// The random stream of the staging kernel: counter-based Philox4x32-10 keyed by (seed, step).  Every source runs these bodies, so the
// same (b, p, c0, seed, step) draws the same values for each of them.  Three families of calls, which differ in their keys for every
// seed, so no counter of one can meet one of another:
//   geometric, key (seed lo, seed hi), counter (b, 0x5eed, step lo, step hi), b the batch position:
//     flip = w0 >> 31, top = (w1 * 9) >> 32, left = (w2 * 9) >> 32 (0..8), rot = w3 >> 30
//   policy (include/eae.h, eae_aug), key (~seed lo, seed hi), counter (b, tag + (c0 << 16), step lo, step hi):
//     AUG_TAG_IMAGE (c0 = 0)        w0 -> theta (degrees), w1 -> sigma, w2 -> the image gain g
//     AUG_TAG_GAIN, band group c0   w_j -> the gain of band c0 + j
//     AUG_TAG_OFFSET, band group c0 w_j -> the offset of band c0 + j
//   noise, key (seed lo, ~seed hi), counter (p lo, (p hi ^ 0xA5A5) + (c0 << 16), step lo, step hi), p the flat index over [B][H][W]
__device__ __forceinline__ void philox4(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t* o) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
    uint32_t h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
    uint32_t n0 = h1 ^ c1 ^ k0, n1 = l1, n2 = h0 ^ c3 ^ k1, n3 = l0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  o[0] = c0; o[1] = c1; o[2] = c2; o[3] = c3;
}
constexpr uint32_t AUG_TAG_IMAGE = 0xA061u, AUG_TAG_GAIN = 0xA062u, AUG_TAG_OFFSET = 0xA063u;
__device__ __forceinline__ void stage_draw_geom(int b, unsigned long long seed, unsigned long long step, int& flip, int& top, int& left, int& rot) {
  uint32_t o[4];
  philox4((uint32_t)b, 0x5eedu, (uint32_t)step, (uint32_t)(step >> 32), (uint32_t)seed, (uint32_t)(seed >> 32), o);
  flip = o[0] >> 31; top = (int)(((unsigned long long)o[1] * 9) >> 32); left = (int)(((unsigned long long)o[2] * 9) >> 32);
  rot = (int)(o[3] >> 30);
}
__device__ __forceinline__ void stage_aug_words(int b, uint32_t tag, int c0, unsigned long long seed, unsigned long long step, uint32_t* o) {
  philox4((uint32_t)b, tag + ((uint32_t)c0 << 16), (uint32_t)step, (uint32_t)(step >> 32), ~(uint32_t)seed, (uint32_t)(seed >> 32), o);
}
// uniform in [lo, lo + width): (w >> 8) 2^-24, exact in fp32, mapped with one fma
__device__ __forceinline__ float stage_uniform(uint32_t w, float lo, float width) {
  return fmaf((float)(w >> 8) * (1.0f / 16777216.0f), width, lo);
}
// z[0..3]: the standard normals of bands c0 .. c0 + 3 of pixel p, the flat index over [B][H][W] (two Box-Muller pairs of one call)
__device__ __forceinline__ void stage_draw_noise4(long long p, int c0, unsigned long long seed, unsigned long long step, float* z) {
  uint32_t o[4];
  philox4((uint32_t)p, ((uint32_t)(p >> 32) ^ 0xA5A5u) + ((uint32_t)c0 << 16), (uint32_t)step, (uint32_t)(step >> 32), (uint32_t)seed,
          ~(uint32_t)(seed >> 32), o);
  const float u1 = ((o[0] >> 8) + 1) * (1.0f / 16777216.0f), u2 = (o[1] >> 8) * (1.0f / 16777216.0f);
  const float u3 = ((o[2] >> 8) + 1) * (1.0f / 16777216.0f), u4 = (o[3] >> 8) * (1.0f / 16777216.0f);
  const float r1 = sqrtf(-2.0f * __logf(u1)), r2 = sqrtf(-2.0f * __logf(u3));
  z[0] = r1 * __cosf(6.28318530718f * u2); z[1] = r1 * __sinf(6.28318530718f * u2);
  z[2] = r2 * __cosf(6.28318530718f * u4); z[3] = r2 * __sinf(6.28318530718f * u4);
}
