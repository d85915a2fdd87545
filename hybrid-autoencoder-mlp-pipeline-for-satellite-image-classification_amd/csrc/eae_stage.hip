// On-device input staging: uint8 / uint16 / fp32 source -> the fp32 NCHW batch conv1 reads, so a batch crosses PCIe
// as 12 KB/img.  The reference's training transform (R.md:225-230)
//   RandomHorizontalFlip -> RandomCrop(H, padding=4) -> ToTensor -> AddGaussianNoise(0, 0.03)   (eval: ToTensor only, R.md:232-234)
// as ONE kernel body for every staging call of include/eae.h, plain or with an augmentation policy (but for the plain scene call, which
// keeps the kernel it had: scene_stage_windows_kernel below):
//   out[b,c,y,x] = src_b[c, y+top-4, flip ? W-1-(x+left-4) : x+left-4] / divisor[c] (0 outside) + std * N(0,1)
// The calls differ in the source src_b that a tap is read from: AugSrcHwc (eae_augment: uint8 HWC, / 255), AugSrcBands (eae_stage_bands:
// image index[b] of a planar dataset), AugSrcScene (eae_scene_stage_windows: window windows[b] of a scene).  The division is a true
// one, as ToTensor's; an image or window id out of range gives NaN for that image instead of a read outside the source.  Per image
// (flip, top, left) and the noise come from the Philox stream of eae_stage.h, keyed by (seed, step), unless explicit draws are given
// (parity tests); train = 0 is the division alone.  The policy ("augmentation policy", include/eae.h) adds quarter turns, a small
// rotation and scale, and a per-band gain and offset; a plain call is its integer path at rot = 0 with no radiometric step.  No matrix
// instructions: built with packed FP32 disabled (EAE_NO_PK, tests/test_isa_guard.py).
#include "eae_internal.h"
#include "eae_common.hip.h"
#include "eae_edge.hip.h"
#include "eae_stage.h"
#include <cmath>
#include <cstdio>
#include <type_traits>

namespace {

// ---------------------------------------------------------------------------------------------------------------- sources
// locate(): the element of band 0 that the integer path reads for the window-local position (sy, unflipped sx) of the image at batch
// position b, or false when that position reads 0; at(off, c): the raw value of band c there.  64-bit positions: a tap of the
// bilinear path may lie anywhere.
struct AugSrcHwc {                      // eae_augment: uint8 HWC [B][H][W][3], ToTensor's / 255
  typedef uint8_t T;
  static constexpr int BANDS = 3;
  const uint8_t* in; int H, W;
  struct Img { long long base; };
  __device__ __forceinline__ bool image(int b, Img& im) const { im.base = (long long)b * H * W * 3; return true; }
  __device__ __forceinline__ bool locate(const Img& im, long long sy, long long sx, int flip, long long& off) const {
    if (sy < 0 || sy >= H || sx < 0 || sx >= W) return false;
    if (flip) sx = W - 1 - sx;
    off = im.base + (sy * W + sx) * 3;
    return true;
  }
  __device__ __forceinline__ T at(long long off, int c) const { return in[off + c]; }
  __device__ __forceinline__ float div(int) const { return 255.0f; }
};

template <typename TT>
struct AugSrcBands {                    // eae_stage_bands: planar [N][C][H][W], gathered by index
  typedef TT T;
  static constexpr int BANDS = 0;
  const TT* src; const long long* index; const float* divisor; long long N; int C, H, W;
  struct Img { long long base; };
  __device__ __forceinline__ bool image(int b, Img& im) const {
    const long long n = index ? index[b] : (long long)b;
    im.base = n * C * H * W;
    return n >= 0 && n < N;
  }
  __device__ __forceinline__ bool locate(const Img& im, long long sy, long long sx, int flip, long long& off) const {
    if (sy < 0 || sy >= H || sx < 0 || sx >= W) return false;
    if (flip) sx = W - 1 - sx;
    off = im.base + sy * W + sx;
    return true;
  }
  __device__ __forceinline__ T at(long long off, int c) const { return src[off + (long long)c * H * W]; }
  __device__ __forceinline__ float div(int c) const { return divisor[c]; }
};

template <typename TT, bool CROP_SCENE>
struct AugSrcScene {                    // eae_scene_stage_windows: window windows[b] of a planar scene [C][Hs][Ws]
  typedef TT T;
  static constexpr int BANDS = 0;
  const TT* src; const long long* windows; const float* divisor; long long plane, nwin; int C, Hs, Ws, H, W, S, nW;      // H = W = P
  struct Img { long long oy, ox; };
  __device__ __forceinline__ bool image(int b, Img& im) const {
    const long long w = windows[b];
    const bool valid = w >= 0 && w < nwin;
    const long long wi = valid ? w / nW : 0, wj = valid ? w - wi * nW : 0;
    im.oy = wi * S; im.ox = wj * S;
    return valid;
  }
  __device__ __forceinline__ bool locate(const Img& im, long long sy, long long sx, int flip, long long& off) const {
    if constexpr (!CROP_SCENE) { if (sy < 0 || sy >= H || sx < 0 || sx >= W) return false; }
    if (flip) sx = W - 1 - sx;
    const long long gy = im.oy + sy, gx = im.ox + sx;         // the origin is added to integers only
    if constexpr (CROP_SCENE) { if (gy < 0 || gy >= Hs || gx < 0 || gx >= Ws) return false; }
    off = gy * Ws + gx;
    return true;
  }
  __device__ __forceinline__ T at(long long off, int c) const { return src[off + c * plane]; }
  __device__ __forceinline__ float div(int c) const { return divisor[c]; }
};

// ---------------------------------------------------------------------------------------------------------------- draws
// The per-image draws are ten CALLS of four words each: 0 = (flip, top, left, rot), 1 = (a, b, g, -), 2 + k = the gains of bands
// 4k .. 4k + 3, 6 + k = their offsets.  A call is a pure function of (b, seed, step, policy), so it gives the same words whether every
// thread makes it or one thread of the workgroup does and leaves them in LDS.
constexpr int AUG_CALLS = 10, AUG_LDS_IMGS = 2;      // a workgroup's 256 consecutive pixels span at most two images of >= 256 pixels
constexpr float AUG_DEG = 0.017453292519943295f;     // fl32(pi / 180)

// (a kernel built with EAE_NO_PK inlines only what is marked __forceinline__: the target attribute differs from the headers' inline
//  functions, and a real call spills the kernel's argument structs to scratch -- so the bit casts and the barrier are spelled here)
__device__ __forceinline__ uint32_t aug_bits(float f) { return __builtin_bit_cast(uint32_t, f); }
__device__ __forceinline__ float aug_float(uint32_t u) { return __builtin_bit_cast(float, u); }
__device__ __forceinline__ void aug_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

__device__ __forceinline__ EAE_NO_PK void aug_call(const StageAug& A, int C, int b, int call, unsigned long long seed, unsigned long long step,
                                                   uint32_t* w) {
  if (call == 0) {
    // (a stride-3 table and the fixed state come from plain calls and train = 0, which launch the PLAIN instantiation only: in the
    //  others these two tests are never taken)
    int flip = 0, top = 4, left = 4, rot = 0;
    if (A.geom) {
      const int* g = A.geom + (long long)b * A.geom_stride;
      flip = g[0]; top = g[1]; left = g[2];
      if (A.geom_stride == 4) rot = g[3] & 3;
    } else if (!A.fixed) { stage_draw_geom(b, seed, step, flip, top, left, rot); if (!A.dihedral) rot = 0; }
    w[0] = (uint32_t)flip; w[1] = (uint32_t)top; w[2] = (uint32_t)left; w[3] = (uint32_t)rot;
  } else if (call == 1) {
    float a = 1.f, bb = 0.f, g = 1.f;
    const bool draw_ab = A.affine_on && !A.affine, draw_g = A.radio_on && !A.radio && A.g_w != 0.f;
    uint32_t o[4] = {0, 0, 0, 0};
    if (draw_ab || draw_g) stage_aug_words(b, AUG_TAG_IMAGE, 0, seed, step, o);
    if (A.affine) { a = A.affine[b * 2]; bb = A.affine[b * 2 + 1]; }
    else if (draw_ab) {
      const float th = __fmul_rn(stage_uniform(o[0], A.rot_lo, A.rot_w), AUG_DEG), sg = stage_uniform(o[1], A.sc_lo, A.sc_w);
      float sn, cs;
      sincosf(th, &sn, &cs);
      a = __fdiv_rn(cs, sg); bb = __fdiv_rn(sn, sg);
    }
    if (draw_g) g = stage_uniform(o[2], A.g_lo, A.g_w);
    w[0] = aug_bits(a); w[1] = aug_bits(bb); w[2] = aug_bits(g); w[3] = 0u;
  } else {
    const bool gains = call < 6;
    const int c0 = (gains ? call - 2 : call - 6) * 4;
    const float lo = gains ? A.bg_lo : A.of_lo, wd = gains ? A.bg_w : A.of_w, none = gains ? 1.f : 0.f;
    float v[4] = {none, none, none, none};
    if (A.radio) {
#pragma unroll
      for (int j = 0; j < 4; ++j) if (c0 + j < C) v[j] = A.radio[((long long)b * C + c0 + j) * 2 + (gains ? 0 : 1)];
    } else if (A.radio_on && wd != 0.f && c0 < C) {
      uint32_t o[4];
      stage_aug_words(b, gains ? AUG_TAG_GAIN : AUG_TAG_OFFSET, c0, seed, step, o);
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = stage_uniform(o[j], lo, wd);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) w[j] = aug_bits(v[j]);
  }
}

// the integer path's source of output position (xo, yo), any integers: doubled centred coordinates, quarter turns, crop shift
template <typename SRC>
__device__ __forceinline__ bool aug_locate(const SRC& s, const typename SRC::Img& im, bool valid, int rot, int flip, int top, int left,
                                           long long xo, long long yo, long long& off) {
  long long U = 2 * xo - (s.W - 1), V = 2 * yo - (s.H - 1);
  if (rot & 1) { const long long t = U; U = -V; V = t; }
  if (rot & 2) { U = -U; V = -V; }
  const long long sx = ((U + (s.W - 1)) >> 1) + left - 4, sy = ((V + (s.H - 1)) >> 1) + top - 4;      // even sums (H == W when turned)
  return valid && s.locate(im, sy, sx, flip, off);
}

// a / d for 0 <= a < lim and 0 < d <= lim: in 32 bits when lim allows it (uniform; a 64-bit division is some hundred instructions)
__device__ __forceinline__ long long aug_div(long long a, long long d, long long lim) {
  return lim <= 0xffffffffLL ? (long long)((unsigned)a / (unsigned)d) : a / d;
}
__device__ __forceinline__ float aug_lerp(float p, float q, float t) { return fmaf(t, __fsub_rn(q, p), p); }

// ---------------------------------------------------------------------------------------------------------------- the kernel
// One thread per output pixel, all bands; p is the flat index over [B][H][W], which stage_draw_noise4(p, c0) draws the noise for.
// AFFINE: the bilinear path (four taps); else the integer path (one).  Loads are unconditional -- a tap that reads 0 loads element 0 of
// the source and drops it -- so the bands' loads of a thread are all in flight together.
// PLAIN: the launch has no quarter turn, no radiometric step and no bilinear path (a plain call, a policy with nothing on, train = 0):
// rot = 0 and the radiometric branch are folded away and every thread makes the one geometric draw itself, no prologue
// (without the flag the plain calls ran 6 % slower than the kernels this body replaced).
// SRC::BANDS: the band count when the source fixes it (else 0: nbands).
template <typename SRC, bool LDS, bool AFFINE, bool PLAIN>
__global__ EAE_NO_PK __launch_bounds__(256) void stage_kernel(SRC s, int nbands, int B, float* __restrict__ out, float std,
                                                              unsigned long long seed, unsigned long long step, StageAug A,
                                                              const float* __restrict__ noise) {
  const int H = s.H, W = s.W, C = SRC::BANDS ? SRC::BANDS : nbands;
  const long long plane = (long long)H * W, tot = plane * B;
  const long long p0 = (long long)blockIdx.x * 256, p = p0 + threadIdx.x;
  const bool radio = !PLAIN && (A.radio_on || A.radio != nullptr);
  __shared__ uint32_t draws[LDS ? AUG_LDS_IMGS : 1][AUG_CALLS][4];
  const int b_first = (int)aug_div(p0, plane, tot);
  if constexpr (LDS) {
    const int t = threadIdx.x, i = t / AUG_CALLS, call = t - i * AUG_CALLS;
    if (i < AUG_LDS_IMGS && b_first + i < B) aug_call(A, C, b_first + i, call, seed, step, draws[i][call]);
    aug_barrier();
  }
  if (p >= tot) return;
  const int b = (int)aug_div(p, plane, tot);
  const long long r = p - b * plane;
  const int y = (int)aug_div(r, W, plane), x = (int)(r - (long long)y * W);
  uint32_t wg[4], wi[4];
  if constexpr (LDS) {
#pragma unroll
    for (int j = 0; j < 4; ++j) { wg[j] = draws[b - b_first][0][j]; wi[j] = draws[b - b_first][1][j]; }
  } else {
    aug_call(A, C, b, 0, seed, step, wg);
    if (AFFINE || radio) aug_call(A, C, b, 1, seed, step, wi); else { wi[0] = aug_bits(1.f); wi[1] = 0u; wi[2] = wi[0]; wi[3] = 0u; }
  }
  const int flip = (int)wg[0], top = (int)wg[1], left = (int)wg[2], rot = PLAIN ? 0 : (int)wg[3];
  const float ca = aug_float(wi[0]), cb = aug_float(wi[1]), g = aug_float(wi[2]);
  typename SRC::Img im;
  const bool valid = s.image(b, im);

  constexpr int TAPS = AFFINE ? 4 : 1;
  long long off[TAPS];
  bool in[TAPS];
  float fx = 0.f, fy = 0.f;
  if constexpr (AFFINE) {
    const float cx = 0.5f * (float)(W - 1), cy = 0.5f * (float)(H - 1);
    const float u = (float)x - cx, v = (float)y - cy;                               // exact
    float X = __fadd_rn(fmaf(ca, u, -__fmul_rn(cb, v)), cx), Y = __fadd_rn(fmaf(cb, u, __fmul_rn(ca, v)), cy);
    X = fminf(fmaxf(X, -1.0e9f), 1.0e9f); Y = fminf(fmaxf(Y, -1.0e9f), 1.0e9f);      // explicit (a, b) of any size; NaN -> -1e9
    const float Xf = floorf(X), Yf = floorf(Y);
    fx = __fsub_rn(X, Xf); fy = __fsub_rn(Y, Yf);                                   // exact
    const long long xi = (long long)Xf, yi = (long long)Yf;
#pragma unroll
    for (int k = 0; k < 4; ++k) in[k] = aug_locate(s, im, valid, rot, flip, top, left, xi + (k & 1), yi + (k >> 1), off[k]);
  } else {
    in[0] = aug_locate(s, im, valid, rot, flip, top, left, x, y, off[0]);
  }
#pragma unroll
  for (int k = 0; k < TAPS; ++k) if (!in[k]) off[k] = 0;

  for (int c0 = 0; c0 < C; c0 += 4) {
    float z[4] = {0.f, 0.f, 0.f, 0.f};
    if (std != 0.f && !noise) stage_draw_noise4(p, c0, seed, step, z);
    uint32_t wgain[4], woff[4];
    if (radio) {
      if constexpr (LDS) {
#pragma unroll
        for (int j = 0; j < 4; ++j) { wgain[j] = draws[b - b_first][2 + (c0 >> 2)][j]; woff[j] = draws[b - b_first][6 + (c0 >> 2)][j]; }
      } else {
        aug_call(A, C, b, 2 + (c0 >> 2), seed, step, wgain);
        aug_call(A, C, b, 6 + (c0 >> 2), seed, step, woff);
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = c0 + j;
      if (c >= C) break;
      const float d = s.div(c);
      float v;
      if constexpr (AFFINE) {
        float t[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) { const float raw = (float)s.at(off[k], c); t[k] = in[k] ? raw : 0.f; }
        v = aug_lerp(aug_lerp(t[0], t[1], fx), aug_lerp(t[2], t[3], fx), fy) / d;
      } else {
        const float q = scene_val(s.at(off[0], c), d);
        v = in[0] ? q : 0.f;
      }
      if (!valid) v = __builtin_nanf("");
      if (radio) v = fmaf(v, __fmul_rn(g, aug_float(wgain[j])), aug_float(woff[j]));
      if (std != 0.f) v = fmaf(std, noise ? noise[((long long)b * C + c) * plane + r] : z[j], v);
      out[((long long)b * C + c) * plane + r] = v;
    }
  }
}

// train = 0: the fixed state in place of `policy` -- nothing is drawn, neither through LDS nor by a thread, and no noise is added
template <typename SRC>
int launch_aug(hipStream_t st, const SRC& s, int C, int B, float* out, int train, float std, unsigned long long seed,
               unsigned long long step, const StageAug& policy, const float* noise, const char* too_large) {
  const long long nblk = ((long long)B * s.H * s.W + 255) / 256;
  if (nblk > 0x7fffffffLL) return eae_set_error(EAE_ERR_ARG, too_large);
  EAE_NO_GROUP("stage_kernel");
  StageAug aug = policy;
  if (!train) { aug = StageAug(); aug.fixed = 1; std = 0.f; }
  const bool affine = aug.affine_on || aug.affine != nullptr;
  const bool plain = !affine && !aug.radio_on && !aug.radio && !aug.dihedral && !(aug.geom && aug.geom_stride == 4);
  const std::true_type yes;
  const std::false_type no;
  auto launch = [&](auto lds, auto aff, auto pl) {
    hipLaunchKernelGGL((stage_kernel<SRC, decltype(lds)::value, decltype(aff)::value, decltype(pl)::value>), dim3((unsigned)nblk), dim3(256),
                       0, st, s, C, B, out, std, seed, step, aug, noise);
  };
  if (plain) launch(no, no, yes);                      // whatever aug.lds says: a PLAIN launch draws per thread
  else if (aug.lds) { if (affine) launch(yes, yes, no); else launch(yes, no, no); }
  else { if (affine) launch(no, yes, no); else launch(no, no, no); }
  EAE_LAUNCH_CHECK();
  return 0;
}

bool range_ok(float v, float below) { return std::isfinite(v) && v >= 0.f && v < below; }

}  // namespace

int eae_stage_aug_prepare(const eae_aug* aug, const int* geom, const float* affine, const float* radio, int H, int W, const char* who,
                          StageAug* out) {
  StageAug a = StageAug();
  char msg[160];
  auto fail = [&](const char* what) { snprintf(msg, sizeof msg, "%s: %s", who, what); return eae_set_error(EAE_ERR_ARG, msg); };
  int mode = 0;
  if (aug) {
    if (!range_ok(aug->rotate, 180.0000001f)) return fail("augment: rotate must be in 0..180 degrees");
    if (!range_ok(aug->scale, 1.f)) return fail("augment: scale must be in [0, 1)");
    if (!range_ok(aug->gain, 1.f)) return fail("augment: gain must be in [0, 1)");
    if (!range_ok(aug->band_gain, 1.f)) return fail("augment: band_gain must be in [0, 1)");
    if (!range_ok(aug->offset, INFINITY)) return fail("augment: offset must not be negative");
    if (aug->draw_mode < 0 || aug->draw_mode > 2) return fail("augment: draw_mode must be 0, 1 or 2");
    mode = aug->draw_mode;
    a.dihedral = aug->dihedral != 0;
    a.affine_on = aug->rotate != 0.f || aug->scale != 0.f;
    a.radio_on = aug->gain != 0.f || aug->band_gain != 0.f || aug->offset != 0.f;
    a.rot_lo = -aug->rotate; a.rot_w = 2.f * aug->rotate;
    a.sc_lo = 1.f - aug->scale; a.sc_w = 2.f * aug->scale;
    a.g_lo = 1.f - aug->gain; a.g_w = 2.f * aug->gain;
    a.bg_lo = 1.f - aug->band_gain; a.bg_w = 2.f * aug->band_gain;
    a.of_lo = -aug->offset; a.of_w = 2.f * aug->offset;
  }
  a.geom = geom; a.geom_stride = 4; a.affine = affine; a.radio = radio;
  if ((a.dihedral || geom) && H != W) return fail("augment: quarter turns (dihedral, geom) need square images, H == W");
  const long long plane = (long long)H * W;
  if (mode == 2 && plane < 256) return fail("augment: draw_mode 2 needs images of at least 256 pixels");
  // the draws of an image: by every thread, or once per workgroup through LDS ("Augmentation policy").  Read by launches
  // with something of the policy on; one with nothing on (PLAIN) draws per thread under every draw_mode, 2 included.
  a.lds = mode == 2 || (mode == 0 && plane >= 256);
  *out = a;
  return 0;
}

StageAug eae_stage_plain(const int* params) {
  StageAug a = StageAug();
  a.geom = params; a.geom_stride = 3;
  return a;
}

// the checks and the launch of eae_augment[_aug]
static int stage_hwc(hipStream_t st, const void* in_u8, float* out, int B, int H, int W, int train, float std, unsigned long long seed,
                     unsigned long long step, const StageAug& aug, const float* noise) {
  if (!in_u8 || !out || B <= 0 || H <= 0 || W <= 0) return eae_set_error(EAE_ERR_ARG, "augment: bad argument");
  const AugSrcHwc s = {(const uint8_t*)in_u8, H, W};
  return launch_aug(st, s, 3, B, out, train, std, seed, step, aug, noise, "augment: batch too large");
}

// the checks and the launch of eae_stage_bands[_aug]
static int stage_bands(hipStream_t st, const void* src, int elem_bytes, long long N, int C, int H, int W, const long long* index, int B,
                       const float* divisor, float* out, int train, float std, unsigned long long seed, unsigned long long step,
                       const StageAug& aug, const float* noise) {
  if (!src || !divisor || !out || N <= 0 || B <= 0 || H <= 0 || W <= 0) return eae_set_error(EAE_ERR_ARG, "stage_bands: bad argument");
  if (C < 1 || C > 16) return eae_set_error(EAE_ERR_ARG, "stage_bands: in_channels must be in 1..16");
  if (elem_bytes != 1 && elem_bytes != 2) return eae_set_error(EAE_ERR_ARG, "stage_bands: source must be uint8 or uint16 (elem_bytes 1 or 2)");
  if (!index && B > N) return eae_set_error(EAE_ERR_ARG, "stage_bands: without an index the batch is the first B images (B <= N)");
  if (elem_bytes == 1) {
    const AugSrcBands<uint8_t> s = {(const uint8_t*)src, index, divisor, N, C, H, W};
    return launch_aug(st, s, C, B, out, train, std, seed, step, aug, noise, "stage_bands: batch too large");
  }
  const AugSrcBands<uint16_t> s = {(const uint16_t*)src, index, divisor, N, C, H, W};
  return launch_aug(st, s, C, B, out, train, std, seed, step, aug, noise, "stage_bands: batch too large");
}

int eae_launch_augment(hipStream_t st, const void* in_u8, float* out, int B, int H, int W, int train, float std, unsigned long long seed,
                       unsigned long long step, const int* params, const float* noise) {
  return stage_hwc(st, in_u8, out, B, H, W, train, std, seed, step, eae_stage_plain(params), noise);
}

int eae_launch_stage_bands(hipStream_t st, const void* src, int elem_bytes, long long N, int C, int H, int W, const long long* index, int B,
                           const float* divisor, float* out, int train, float std, unsigned long long seed, unsigned long long step,
                           const int* params, const float* noise) {
  return stage_bands(st, src, elem_bytes, N, C, H, W, index, B, divisor, out, train, std, seed, step, eae_stage_plain(params), noise);
}

template <typename T, bool CROP_SCENE>
static int launch_scene(hipStream_t st, const eae_scene* sc, long long nW, long long nwin, const long long* windows, int B, float* out,
                        int train, float std, unsigned long long seed, unsigned long long step, const StageAug& aug, const float* noise) {
  const AugSrcScene<T, CROP_SCENE> s = {(const T*)sc->data, windows, sc->divisor, (long long)sc->H * sc->W, nwin, sc->C, sc->H, sc->W,
                                        sc->patch, sc->patch, sc->stride, (int)nW};
  return launch_aug(st, s, sc->C, B, out, train, std, seed, step, aug, noise, "scene_stage_windows: batch too large");
}
int eae_launch_scene_stage(hipStream_t st, const eae_scene* s, long long nW, long long nwin, const long long* windows, int B, float* out,
                           int train, float std, unsigned long long seed, unsigned long long step, const StageAug& aug, const float* noise,
                           int crop) {
  const bool sc = crop == EAE_CROP_SCENE;
  switch (s->dtype) {
    case EAE_SCENE_U8:
      return sc ? launch_scene<uint8_t, true>(st, s, nW, nwin, windows, B, out, train, std, seed, step, aug, noise)
                : launch_scene<uint8_t, false>(st, s, nW, nwin, windows, B, out, train, std, seed, step, aug, noise);
    case EAE_SCENE_U16:
      return sc ? launch_scene<uint16_t, true>(st, s, nW, nwin, windows, B, out, train, std, seed, step, aug, noise)
                : launch_scene<uint16_t, false>(st, s, nW, nwin, windows, B, out, train, std, seed, step, aug, noise);
    default:
      return sc ? launch_scene<float, true>(st, s, nW, nwin, windows, B, out, train, std, seed, step, aug, noise)
                : launch_scene<float, false>(st, s, nW, nwin, windows, B, out, train, std, seed, step, aug, noise);
  }
}

// The plain scene call alone keeps a kernel of its own: stage_kernel's PLAIN instantiation over AugSrcScene computes the same values
// (tests/test_gpu_augment.py::test_no_policy_is_the_plain_call) but ran the loader epochs 1 - 2 % slower, for a cause that was not
// found.  The transform is the head comment's with src_b = window windows[b], origin (oy, ox); one thread per
// output pixel, all bands, p the flat index over [B][P][P]; the draws are stage_kernel's calls (eae_stage.h), so equal (b, p, c0, seed,
// step) give equal values.  CROP_SCENE = false: (sy, unflipped sx) outside [0, P) reads 0; true: the read is bounds-checked against
// the scene instead.  An id outside [0, nwin) gives NaN and reads nothing.
template <typename T, bool CROP_SCENE>
__global__ EAE_NO_PK __launch_bounds__(256) void scene_stage_windows_kernel(const T* __restrict__ src, const float* __restrict__ divisor,
                                                                        int C, long long plane, int Hs, int Ws, int P, int S, int nW,
                                                                        long long nwin, const long long* __restrict__ windows, int B,
                                                                        float* __restrict__ out, int train, float std,
                                                                        unsigned long long seed, unsigned long long step,
                                                                        const int* __restrict__ params, const float* __restrict__ noise) {
  const long long pp = (long long)P * P;
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= pp * B) return;
  const int b = (int)(p / pp);
  const long long r = p - b * pp;
  const int y = (int)(r / P), x = (int)(r - (long long)y * P);
  const long long w = windows[b];
  const bool valid = w >= 0 && w < nwin;
  int flip = 0, top = 4, left = 4, rot = 0;
  if (train) {
    if (params) { flip = params[b * 3]; top = params[b * 3 + 1]; left = params[b * 3 + 2]; }
    else stage_draw_geom(b, seed, step, flip, top, left, rot);
  }
  const long long sy = (long long)y + top - 4;
  long long sx = (long long)x + left - 4;
  bool inside = valid;
  if constexpr (!CROP_SCENE) inside = inside && sy >= 0 && sy < P && sx >= 0 && sx < P;
  if (flip) sx = P - 1 - sx;
  const long long wi = valid ? w / nW : 0, wj = valid ? w - wi * nW : 0;
  const long long gy = wi * S + sy, gx = wj * S + sx;                  // scene pixel
  if constexpr (CROP_SCENE) inside = inside && gy >= 0 && gy < Hs && gx >= 0 && gx < Ws;
  const T* q = src + (inside ? gy * Ws + gx : 0);
  for (int c0 = 0; c0 < C; c0 += 4) {
    float z[4] = {0.f, 0.f, 0.f, 0.f};
    if (train && std != 0.f && !noise) stage_draw_noise4(p, c0, seed, step, z);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = c0 + j;
      if (c >= C) break;
      float v = inside ? scene_val(q[c * plane], divisor[c]) : 0.f;
      if (!valid) v = __builtin_nanf("");
      if (train && std != 0.f) v = fmaf(std, noise ? noise[((long long)b * C + c) * pp + r] : z[j], v);
      out[((long long)b * C + c) * pp + r] = v;
    }
  }
}
int eae_launch_scene_stage_plain(hipStream_t st, const eae_scene* s, long long nW, long long nwin, const long long* windows, int B,
                                 float* out, int train, float std, unsigned long long seed, unsigned long long step, const int* params,
                                 const float* noise, int crop) {
  const long long plane = (long long)s->H * s->W, nblk = ((long long)B * s->patch * s->patch + 255) / 256;
  if (nblk > 0x7fffffffLL) return eae_set_error(EAE_ERR_ARG, "scene_stage_windows: batch too large");
  EAE_NO_GROUP("scene_stage_windows_kernel");
  auto launch = [&](auto* t, auto scene_crop) {
    using T = std::remove_cv_t<std::remove_pointer_t<decltype(t)>>;
    hipLaunchKernelGGL((scene_stage_windows_kernel<T, decltype(scene_crop)::value>), dim3((unsigned)nblk), dim3(256), 0, st,
                       (const T*)s->data, s->divisor, s->C, plane, s->H, s->W, s->patch, s->stride, (int)nW, nwin, windows, B, out, train,
                       std, seed, step, params, noise);
  };
  auto by_crop = [&](auto* t) { if (crop == EAE_CROP_SCENE) launch(t, std::true_type()); else launch(t, std::false_type()); };
  switch (s->dtype) {
    case EAE_SCENE_U8: by_crop((const uint8_t*)nullptr); break;
    case EAE_SCENE_U16: by_crop((const uint16_t*)nullptr); break;
    default: by_crop((const float*)nullptr);
  }
  EAE_LAUNCH_CHECK();
  return 0;
}

extern "C" int eae_augment_aug(void* stream, const void* in_u8, float* out, int B, int H, int W, int train, float noise_std,
                               unsigned long long seed, unsigned long long step, const eae_aug* aug, const int* geom,
                               const float* affine, const float* radio, const float* noise) {
  StageAug a;
  if (int rc = eae_stage_aug_prepare(aug, geom, affine, radio, H, W, "augment", &a)) return rc;
  return stage_hwc((hipStream_t)stream, in_u8, out, B, H, W, train, noise_std, seed, step, a, noise);
}

extern "C" int eae_stage_bands_aug(void* stream, const void* src, int elem_bytes, long long N, int C, int H, int W, const long long* index,
                                   int B, const float* divisor, float* out, int train, float noise_std, unsigned long long seed,
                                   unsigned long long step, const eae_aug* aug, const int* geom, const float* affine,
                                   const float* radio, const float* noise) {
  StageAug a;
  if (int rc = eae_stage_aug_prepare(aug, geom, affine, radio, H, W, "stage_bands", &a)) return rc;
  return stage_bands((hipStream_t)stream, src, elem_bytes, N, C, H, W, index, B, divisor, out, train, noise_std, seed, step, a, noise);
}
