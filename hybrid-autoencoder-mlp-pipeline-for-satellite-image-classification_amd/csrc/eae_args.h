// Plain-data launch arguments and constants of the kernels: what host code fills in and the kernel headers (*.hip.h) read.
// No device code here, so a host unit that builds argument blocks includes this file and compiles no kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "eae_bn_acc.h"    // bn_acc_limit

typedef uint16_t bf16_t;

// activation "sources": how a logical NHWC activation tensor is materialised when it is loaded
enum { SRC_RAW = 0,      // bf16 tensor as stored
       SRC_BNRELU = 1,   // max(0, s[c]*y + t[c])            (BatchNorm apply + ReLU fused into the consumer's load)
       SRC_BNBWD = 2,    // A[c]*g + B[c]*y + C[c]           (BatchNorm backward apply fused into the consumer's load)
       SRC_F32 = 3,      // fp32 tensor, converted to bf16 on load
       SRC_RAWG = 4 };   // bf16 GRADIENT tensor as stored (the BatchNorm-backward-applied dy a backward-data kernel wrote while it staged
                         // its patch, ConvArgs::dy_out): loads like SRC_RAW; the fp8 variants convert it to e5m2 like SRC_BNBWD

// epilogues of the conv-like kernels
enum { EPI_FWD = 0,      // + bias, store raw bf16, per-channel sum / sum-of-squares partials (BatchNorm batch statistics)
       EPI_MASK = 1,     // ReLU mask from the previous layer's BN output, store masked grad, sum g / sum g*xhat partials
       EPI_PLAIN = 2 };  // store bf16

struct SrcDesc {
  const bf16_t* p0;    // RAW: tensor; BNRELU: raw pre-BN tensor y; BNBWD: masked gradient g
  const bf16_t* p1;    // BNBWD: raw pre-BN tensor y
  const float* coef;   // BNRELU: [4][C] = s, t, mean, invstd ; BNBWD: [3][C] = A, B, C
};

// ---- folded BatchNorm finalize (eae_common.hip.h has the scheme and the device side)
struct BnAcc {
  unsigned long long* acc;   // [copies][2][C]; zero before the producer runs; nullptr: per-tile partials + finalize kernel
  int copies;                // power of two
  float scale;               // fixed-point scale
  unsigned long long* flag;  // [C] sticky "a partial of this channel was not finite or too large" words (cleared with the accumulators)
  float limit;               // |v * scale| of one contribution stays below this, or it raises the flag (set by the launcher, below)
  int world;                 // SyncBN replicas whose accumulators are summed before the consumer reads them (0 or 1: none)
};
// the launcher's part: it knows how many workgroups contribute to one channel (ConvArgs::ntiles)
inline void bn_acc_set_limit(BnAcc& b, int contributions) { b.limit = bn_acc_limit(contributions, b.world); }
struct BnFold {
  const unsigned long long* acc;   // nullptr: the coefficients come from SrcDesc::coef
  int copies;
  float inv_scale, count, momentum, eps;
  const float* gamma; const float* beta;
  float* rm; float* rv; long long* nbt;
  float* coef_out;           // [4][C]: s, t, mean, invstd
  const unsigned long long* flag;  // [C] the layer's non-finite flags (BnAcc::flag)
  unsigned* poison;          // step-wide sticky word (cleared with the accumulators): the writer workgroup sets it when a channel is flagged
};
// copies <= BN_FOLD_K * (256 / C)  (at most BN_FOLD_K accumulator sets per thread of the consumer's prologue)
constexpr int BN_FOLD_K = 4;
constexpr int BN_FOLD_KB = 2;      // backward tables: the consumers hold two source tensors' raw pieces in registers meanwhile
struct BnBwdFold {
  const unsigned long long* acc;   // nullptr: the coefficients come from SrcDesc::coef (bn_bwd_finalize_kernel wrote them)
  int copies;
  float inv_scale, count;
  const float* gamma; const float* coef_fwd;       // [C], [4][C]
  float* dgamma; float* dbeta; float* coef_out;    // [C], [C], [3][C]: written by the `writer` workgroup (each may be nullptr)
  float* dbias;              // eval-mode backward only: gradient of the bias in FRONT of this BatchNorm, A[c] * sum g (train mode: zero)
  const unsigned long long* flag;  // [C] the layer's non-finite flags (BnAcc::flag of the backward accumulators)
  unsigned* poison;          // step-wide sticky word, as in BnFold
};

// ---- 3x3 stride-2 convolution family (eae_igemm.hip.h)
enum { KIND_CONV = 0, KIND_DECONV = 1 };
struct ConvArgs {
  SrcDesc src;
  const bf16_t* wpack;     // [COUT][9][CIN] bf16 (tap = ky*3+kx)
  const float* bias;       // [COUT] (EPI_FWD) or nullptr
  bf16_t* out;             // NHWC bf16
  float* stat_part;        // [2][COUT][ntiles] (channel-major: the finalize kernels read one channel contiguously) or nullptr
  int ntiles;              // number of statistics partials per channel = workgroups along grid.x (set by the launcher)
  const bf16_t* yprev;     // EPI_MASK: raw pre-BN tensor at the output positions
  const float* prev_coef;  // EPI_MASK: [4][COUT] s,t,mean,invstd of that BN
  int B, Hin, Win;         // input spatial size (conv: out = Hin/2; deconv: out = 2*Hin)
  // Progress word of the caller's stream: the first thread of the grid stores `sig_val` there when the kernel STARTS (i.e. after
  // everything enqueued before it on its stream has completed).  Gate kernels on the engine's side streams poll that word, so a
  // hand-over to a side stream needs no event record on the dependency chain (each one cost it ~5 us of bubble).
  unsigned* sig;
  unsigned sig_val;
  BnAcc bacc;              // statistics go to fixed-point accumulators instead of stat_part (finalize folded into the consumer)
  BnFold fold;             // SRC_BNRELU: build the source layer's coefficient table from its accumulators
  BnBwdFold bfold;         // SRC_BNBWD: build the source layer's backward coefficient table from its accumulators
  // fp8 variant (igemm8_s2_kernel, BASELINE config 5): wpack = e4m3 bytes [COUT][9][CIN];  qs[0] = 1 / (scale of the pixel
  // operand) -- the fragments are converted bf16 -> e4m3 (activations) / e5m2 (gradients) with v_cvt_scalef32_pk_*_bf16, which
  // DIVIDES by its scale operand --, qs[1] = 1 / (pixel scale * weight scale), applied to the accumulators;  amax: the largest
  // |staged value| (bf16 bits << 16, atomicMax) for the next step's scale (delayed scaling, eae_fp8.hip)
  const float* qs;
  unsigned* amax;
  int amax_mask;          // amax is an array of amax_mask + 1 slots (a power of two): workgroup t reports into slot t & amax_mask
  int amax_stride;        // words between two slots (the engine: 32 = one 128-byte line per slot; per-op calls: 0 slots -> unused)
  // SRC_BNBWD only: the BatchNorm-backward-applied gradient dy = A*g + B*y + C, exactly as staged (bf16, the source tensor's NHWC
  // layout), is ALSO stored here by channel block 0 of every tile, so that the layer's weight-gradient kernel reads ONE plain
  // tensor instead of transforming g and y again (SRC_RAWG, eae_wgrad.hip.h).  nullptr: off
  bf16_t* dy_out;
#ifdef EAE_STAMPS
  unsigned long long* dbg; // diagnostic build only: s_memtime stamps of workgroup `dbg_block`, wave 0
  int dbg_block;
#endif
};

// ---- the two C-band edge layers (eae_edge.hip.h)
enum { SRC3_NCHW_F32 = 0,     // fp32 planar image (the loader contract)
       SRC3_NHWCP_BF16 = 1,   // bf16 pixels padded to CP channels (gradient of the pre-sigmoid output)
       SRC3_SCENE_U8 = 2,     // P x P windows of a planar uint8 / uint16 / fp32 scene [C][Hs][Ws], value / divisor[c] (eae_scene)
       SRC3_SCENE_U16 = 3,
       SRC3_SCENE_F32 = 4 };

// Scene source of conv1 (eval-mode forward only): image n of the launch is window w = first + n of the grid of P x P windows at
// stride S (nW per row), whose origin is scene pixel (w / nW * S, w % nW * S).  Offsets are 64-bit: scenes exceed 2^31 elements.
// Index-driven form (the IDX template flag of the scene kernels): image n is window index[first + n] instead; an id outside
// [0, nwin) reads as an all-zero window (defence in depth: the callers reject such ids before any launch).
// (SceneSrcCore is the part every scene kernel takes; SceneSrc adds the border fields behind it.  Kernels with arguments after the
// scene take the two parts apart, the border last, so that the argument block of the borderless forms stays as it was.)
struct SceneSrcCore {
  const void* data = nullptr;        // [C][Hs][Ws]
  const float* div = nullptr;        // [C]
  long long first = 0, plane = 0;    // first window of the launch; Hs * Ws
  int Ws = 0, S = 0, nW = 0;
  const long long* index = nullptr;  // window ids (IDX kernels only)
  long long nwin = 0;                // nH * nW
};
// border (BORDER kernels only; eae.h, "Border modes"): the grid lies over the virtual scene, window (i, j) starts at virtual pixel
// (i * S, j * S) = scene pixel (i * S - pt, j * S - pl), and a pixel outside the Hs x Ws scene is resolved when it is loaded
struct SceneBorder {
  int mode = 0, pt = 0, pl = 0, Hs = 0, Ws = 0;
  float fill = 0.f;
};
struct SceneSrc : SceneSrcCore { SceneBorder b; };

// Band counts: C (1..16, a run-time argument) image bands are staged as CP = 4, 8 or 16 (the trailing template argument of every
// edge kernel).  CP = 4 is the RGB form: C = 3 is a compile-time constant there (edge_bands), so it compiles to the registers,
// arithmetic and summation order of the 3-band kernels.  Generic forms with a run-time C measured 3-5 % slower on the RGB step
// (DESIGN.md section 10).  C = 1, 2 and 4..8 -> CP = 8, C = 9..16 -> CP = 16.
constexpr int edge_cp(int C) { return C == 3 ? 4 : C <= 8 ? 8 : 16; }
// loss partial row of deconv4 / sigmoid backward: {sum diff^2, sum g(c) for c < C}, padded to whole float4s (4 floats for C = 3)
__host__ __device__ constexpr int edge_lp_stride(int C) { return (C + 4) / 4 * 4; }

// out[m][32] = im2col(src)[m][9C] . Wp[32][9C]^T      (conv1 forward; backward-data of deconv4)
struct EdgeArgs {
  const void* src3;        // fp32 NCHW [B,C,H,W] or bf16 NHWC-CP [B,H,W,CP]
  int B, H, W;             // spatial size of the C-band tensor
  ConvArgs c;              // wpack [32][KP] (k = tap*CP + c, zero where c >= C or k >= 9*CP), bias, out [B,H/2,W/2,32], stat_part, yprev, prev_coef
  int C = 3;               // bands (1..16; edge_cp(C) == CP)
};
// deconv4 forward (all four phases jointly) + sigmoid + MSE loss + its gradient
struct Deconv4Args {
  SrcDesc src;             // a3 = BNRELU(u3)  [B,Hin,Win,32]
  const bf16_t* wjoint;    // [16*NT][128]  n = phase*C+co, k = nb*32+ci
  const float* bias;       // [C]
  const float* x;          // target fp32 NCHW [B,C,2Hin,2Win] or nullptr (forward only)
  float* x_hat;            // fp32 NCHW or nullptr
  bf16_t* g4;              // bf16 NHWC-CP [B,2Hin,2Win,CP] or nullptr
  float* loss_part;        // [ntiles][edge_lp_stride(C)]: sum diff^2, sum g (co = 0..C-1), zero padding   or nullptr
  float gscale;
  int B, Hin, Win;
  BnFold fold;             // BNRELU source: coefficient table of deconv3's BatchNorm from its accumulators
  int C = 3;               // bands (1..16; edge_cp(C) == CP)
};
// deconv4 + sigmoid against windows of a scene
struct Deconv4SceneArgs {
  float* part;             // [ntiles][edge_bp_stride(C)]
  float* recon;            // STITCH: fp32 [C][Hg][Wg]; BORDER: [C][Hs][Ws], the real scene
  float* residual;         // STITCH: fp32 [Hg][Wg] or nullptr; BORDER: [Hs][Ws]
  long long gplane = 0;    // Hg * Wg; BORDER: Hs * Ws
  int Wg = 0, nH = 0, m = 0;   // width of the stitched raster (BORDER: Ws), window rows of the grid, (P - S) / 2
};

// ---- weight gradient of the 3x3 stride-2 layers (eae_wgrad.hip.h)
struct WgradArgs {
  SrcDesc small, big;
  float* part;            // [nslices][CS][CB][9]
  int B, Hs, Ws;          // small-map spatial size (big map = 2Hs x 2Ws)
  int tiles_per_block, ntiles, nslices;
  BnBwdFold bfold;        // the SRC_BNBWD operand's coefficient table from the layer's backward accumulators (eae_common.hip.h)
  const float* qs;        // fp8 variant (wgrad8_s2_kernel): 1/scale of the small operand, 1/scale of the big operand, 1/(product)
};

// ---- latent projections (eae_fc.hip.h)
enum { FCE_PARTIAL = 0,    // fp32 partial [kslice][M][N]       (split-K)
       FCE_BIAS_BF16 = 1,  // bf16(acc + bias[n]) -> [M][N]
       FCE_MASK = 2 };     // ReLU mask of the BN output at the same position + BN-backward partial sums
struct FcNtArgs {
  SrcDesc a;               // A [M][K]; SRC_F32: p0 is a float*; BNRELU: channel = k % 256
  const bf16_t* w;         // [N][K]
  int M, N, K;
  int klen;                // K-range per grid.z slice (multiple of 64)
  float* part;             // FCE_PARTIAL
  ConvArgs c;              // FCE_BIAS_BF16 / FCE_MASK: out, bias ([N]), stat_part, yprev, prev_coef ([4][256]);
                           // c.fold: BNRELU source -- coefficient table of the 256-channel source layer from its accumulators
                           // (no field of its own: eight of these blocks must fit one grouped launch, eae_group.h)
};
// R[i][j] = sum_b P[b][i] * Q[b][j]  (eae_fc.hip.h, fc_tn_kernel, has the output permutations)
struct FcTnArgs {
  SrcDesc p, q;            // P [Bt][I], Q [Bt][J]   (F32: p0 is float*; BNRELU: channel = col % 256)
  int Bt, I, J;
  float* out;              // reference-layout weight gradient
  float* colsum;           // bias gradient (reference order) or nullptr
  int out_mode, Pn;        // Pn = pixels per image of the flattened map
};
