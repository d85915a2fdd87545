// Host-side dispatch of the C-band edge-layer kernels (enc.conv1, dec.deconv4): the band count C (1..16) picks the padded width
// CP = edge_cp(C), the last template argument of every edge kernel.
#include "eae_internal.h"
#include <cstdlib>
#include "eae_edge.hip.h"
#include "eae_wgrad.hip.h"
#include "eae_wgrad_plan.h"

static_assert(EDGE_TILE_ROWS == 2 * E_TH && EDGE_TILE_COLS == 2 * E_TW, "the plan's tiles are the edge kernels'");

static int check_edge_shape(int B, int H, int W) {
  if (B <= 0 || H % 8 || W % 64) return eae_set_error(-2, "edge layer: image height must be a multiple of 8 and width of 64");
  return 0;
}
static int check_bands(int C) {
  if (C < 1 || C > 16) return eae_set_error(-2, "edge layer: in_channels must be in 1..16");
  return 0;
}

int eae_launch_edge_conv(hipStream_t st, int src3_kind, int epi, const EdgeArgs& a0) {
  if (int rc = check_edge_shape(a0.B, a0.H, a0.W)) return rc;
  if (int rc = check_bands(a0.C)) return rc;
  EdgeArgs a = a0;
  const int cp = edge_cp(a.C);
  dim3 grid(a.B * (a.H / 2 / E_TH) * (a.W / 2 / E_TW));
  a.c.ntiles = (int)grid.x;
  bn_acc_set_limit(a.c.bacc, a.c.ntiles);
#define CASE1(S, E, P) if (src3_kind == S && epi == E && cp == P) { eae_launch(edge_conv_kernel<S, E, P>, edge_conv_kernel_g<S, E, P>, grid, dim3(256), 0, st, a); EAE_LAUNCH_CHECK(); return 0; }
#define CASE(S, E) CASE1(S, E, 4) CASE1(S, E, 8) CASE1(S, E, 16)
  CASE(SRC3_NCHW_F32, EPI_FWD)
  CASE(SRC3_NHWCP_BF16, EPI_MASK)
  CASE(SRC3_NHWCP_BF16, EPI_PLAIN)
  CASE(SRC3_NCHW_F32, EPI_PLAIN)
#undef CASE
#undef CASE1
  return eae_set_error(-2, "edge_conv: combination not instantiated");
}

// conv1 over windows of a scene (eval-mode forward): the window gather is the kernel's patch load, no staged [B,C,P,P] batch;
// windows first + n, or index[first + n] when s.index is set; the BORDER forms when s.b.mode is
int eae_launch_edge_conv_scene(hipStream_t st, int src3_kind, const EdgeArgs& a0, const SceneSrc& s) {
  if (int rc = check_edge_shape(a0.B, a0.H, a0.W)) return rc;
  if (int rc = check_bands(a0.C)) return rc;
  EdgeArgs a = a0;
  const int cp = edge_cp(a.C);
  dim3 grid(a.B * (a.H / 2 / E_TH) * (a.W / 2 / E_TW));
  a.c.ntiles = (int)grid.x;
  EAE_NO_GROUP("edge_conv_scene_kernel");
#define CASE1(S, P) if (src3_kind == S && cp == P) { \
    if (s.b.mode) { \
      if (s.index) hipLaunchKernelGGL((edge_conv_scene_kernel<S, P, true, true>), grid, dim3(256), 0, st, a, s); \
      else hipLaunchKernelGGL((edge_conv_scene_kernel<S, P, false, true>), grid, dim3(256), 0, st, a, s); \
    } else if (s.index) hipLaunchKernelGGL((edge_conv_scene_kernel<S, P, true>), grid, dim3(256), 0, st, a, s); \
    else hipLaunchKernelGGL((edge_conv_scene_kernel<S, P>), grid, dim3(256), 0, st, a, s); \
    EAE_LAUNCH_CHECK(); return 0; }
#define CASE(S) CASE1(S, 4) CASE1(S, 8) CASE1(S, 16)
  CASE(SRC3_SCENE_U8)
  CASE(SRC3_SCENE_U16)
  CASE(SRC3_SCENE_F32)
#undef CASE
#undef CASE1
  return eae_set_error(-2, "edge_conv_scene: source kind not instantiated");
}

int eae_edge_tiles(int B, int H, int W) { return B * (H / 2 / E_TH) * (W / 2 / E_TW); }

// dw [32][C][3][3] = reduce over blocks of the per-block partials. scratch must hold nblocks*288*C floats.
int eae_launch_edge_wgrad(hipStream_t st, int src3_kind, const void* src3, int B, int H, int W, const SrcDesc& side, int smode,
                          float* scratch, long long scratch_floats, float* dw, const EaeProfHook* hook, const BnBwdFold* bfold,
                          unsigned* sig, unsigned sig_val, int (*mid)(void*, GateArgs*), void* mid_user, int C) {
  if (int rc = check_edge_shape(B, H, W)) return rc;
  if (int rc = check_bands(C)) return rc;
  const int cp = edge_cp(C), slice = (int)eae_edge_wgrad_slice_floats(C);
  // the kernel addresses both operands through buffer descriptors with 32-bit byte offsets below OOB_OFF
  if ((long long)B * H * W * 16 >= 0x7fffff00LL) return eae_set_error(-2, "edge_wgrad: batch too large for one launch (2 GB per operand)");
  EdgeWgradArgs a;
  a.bfold = bfold ? *bfold : BnBwdFold();
  a.sig = sig; a.sig_val = sig_val;
  a.src3 = src3; a.B = B; a.H = H; a.W = W; a.side = side; a.part = scratch; a.C = C;
  // the plan (eae_wgrad_plan.h) under this process's caps
  static const int cap = getenv("EAE_EDGE_WGRAD_BLOCKS") ? atoi(getenv("EAE_EDGE_WGRAD_BLOCKS")) : 512;
  static const int cap_side = getenv("EAE_EDGE_WGRAD_SIDE_BLOCKS") ? atoi(getenv("EAE_EDGE_WGRAD_SIDE_BLOCKS")) : 256;
  EdgeWgPlan p;
  if (!eae_edge_wgrad_plan(p, src3_kind == SRC3_NHWCP_BF16, C, B, H, W, scratch_floats, cap, cap_side, eae_geo_mult))
    return eae_set_error(-2, "edge_wgrad: scratch too small");
  a.ntiles = p.ntiles;
  a.tiles_per_block = p.tiles_per_block;
  const int nblocks = p.blocks;
#define CASE1(S, M, P) if (src3_kind == S && smode == M && cp == P) { if (hook) hook->begin(hook->user, st); eae_launch(edge_wgrad_kernel<S, M, P>, edge_wgrad_kernel_g<S, M, P>, dim3(nblocks), dim3(256), 0, st, a); if (hook) hook->end(hook->user, st); EAE_LAUNCH_CHECK(); goto reduce; }
#define CASE(S, M) CASE1(S, M, 4) CASE1(S, M, 8) CASE1(S, M, 16)
  CASE(SRC3_NCHW_F32, SRC_BNBWD)
  CASE(SRC3_NHWCP_BF16, SRC_BNRELU)
  CASE(SRC3_NCHW_F32, SRC_RAW)
#undef CASE
#undef CASE1
  return eae_set_error(-2, "edge_wgrad: combination not instantiated");
reduce:
  GateArgs tail = GateArgs();      // mid(): the caller's work between the two launches; a gate it returns is waited for in the reduction's tail
  if (mid) { if (int rc = mid(mid_user, &tail)) return rc; }
  {
    const ReduceTallArgs ra = {scratch, nblocks, (long)(slice / 4), dw, tail};
    eae_launch(reduce_slices_tall_kernel, reduce_slices_tall_kernel_g, dim3((slice / 4 + 3) / 4), dim3(256), 0, st, ra);
  }
  EAE_LAUNCH_CHECK();
  return 0;
}

int eae_launch_deconv4_loss(hipStream_t st, int smode, const Deconv4Args& a) {
  if (a.B <= 0 || a.Hin % E_TH || a.Win % E_TW) return eae_set_error(-2, "deconv4: input must be a multiple of 4 x 32");
  if (int rc = check_bands(a.C)) return rc;
  dim3 grid(a.B * (a.Hin / E_TH) * (a.Win / E_TW));
  const int cp = edge_cp(a.C);
#define CASE(M, P) if (smode == M && cp == P) { eae_launch(deconv4_loss_kernel<M, P>, deconv4_loss_kernel_g<M, P>, grid, dim3(256), 0, st, a); EAE_LAUNCH_CHECK(); return 0; }
  CASE(SRC_BNRELU, 4) CASE(SRC_BNRELU, 8) CASE(SRC_BNRELU, 16)
  CASE(SRC_RAW, 4) CASE(SRC_RAW, 8) CASE(SRC_RAW, 16)
#undef CASE
  return eae_set_error(-2, "deconv4: source mode not instantiated");
}

int eae_launch_deconv4_scene(hipStream_t st, int src3_kind, const Deconv4Args& a, const SceneSrc& s, const Deconv4SceneArgs& r) {
  if (a.B <= 0 || a.Hin % E_TH || a.Win % E_TW) return eae_set_error(-2, "deconv4: input must be a multiple of 4 x 32");
  if (a.Hin != a.Win) return eae_set_error(-2, "deconv4_scene: windows are square");
  if (int rc = check_bands(a.C)) return rc;
  if (!r.part) return eae_set_error(-2, "deconv4_scene: NULL partials");
  dim3 grid(a.B * (a.Hin / E_TH) * (a.Win / E_TW));
  const int cp = edge_cp(a.C);
  EAE_NO_GROUP("deconv4_scene_kernel");
#define CASE3(S, P, I, T, D) { hipLaunchKernelGGL((deconv4_scene_kernel<S, P, I, T, D>), grid, dim3(256), 0, st, a, (const SceneSrcCore&)s, r, s.b); EAE_LAUNCH_CHECK(); return 0; }
#define CASE2(S, P, I, T) { if (s.b.mode) CASE3(S, P, I, T, true) else CASE3(S, P, I, T, false) }
#define CASE1(S, P) if (src3_kind == S && cp == P) { \
    if (s.index) { if (r.recon) CASE2(S, P, true, true) else CASE2(S, P, true, false) } \
    else { if (r.recon) CASE2(S, P, false, true) else CASE2(S, P, false, false) } }
#define CASE(S) CASE1(S, 4) CASE1(S, 8) CASE1(S, 16)
  CASE(SRC3_SCENE_U8)
  CASE(SRC3_SCENE_U16)
  CASE(SRC3_SCENE_F32)
#undef CASE
#undef CASE1
#undef CASE2
#undef CASE3
  return eae_set_error(-2, "deconv4_scene: source kind not instantiated");
}

// One (window, band) per thread, 16 lanes per window: the thread of band c adds the window's tiles in ascending order; the band sums
// are then added in ascending order (every lane of the group walks them, lane 0 writes) and divided by C * P * P.  The result depends
// on the window alone, never on the batch it ran in.
__global__ EAE_NO_PK __launch_bounds__(256) void scene_err_finalize_kernel(const float* __restrict__ part, int B, int tiles, int C, int bps,
                                                                       float npix, long long first, const long long* __restrict__ index,
                                                                       long long nwin, float* __restrict__ err,
                                                                       float* __restrict__ band_err) {
  const int t = blockIdx.x * 256 + threadIdx.x, n = t >> 4, c = t & 15;
  const bool live = n < B;
  float s = 0.f;
  if (live && c < C) {
    const float* q = part + (size_t)n * tiles * bps + c;
    for (int k = 0; k < tiles; ++k) s += q[(size_t)k * bps];
  }
  const int base = threadIdx.x & 48;          // first lane of this window's group inside the wave
  float tot = 0.f;
  for (int k = 0; k < C; ++k) tot += __shfl(s, base + k);
  if (!live) return;
  long long w = first + n;
  if (index) w = index[w];
  if (w < 0 || w >= nwin) return;
  if (band_err && c < C) band_err[c * nwin + w] = s / npix;
  if (c == 0) err[w] = tot / (npix * (float)C);
}

int eae_launch_scene_err_finalize(hipStream_t st, const float* part, int B, int P, int C, long long first, const long long* index,
                                  long long nwin, float* err, float* band_err) {
  if (int rc = check_bands(C)) return rc;
  if (!part || !err || B <= 0) return eae_set_error(-2, "scene_err_finalize: NULL argument");
  EAE_NO_GROUP("scene_err_finalize_kernel");
  const int tiles = (P / 2 / E_TH) * (P / 2 / E_TW);
  hipLaunchKernelGGL(scene_err_finalize_kernel, dim3((unsigned)((B * 16 + 255) / 256)), dim3(256), 0, st, part, B, tiles, C,
                     edge_bp_stride(C), (float)P * (float)P, first, index, nwin, err, band_err);
  EAE_LAUNCH_CHECK();
  return 0;
}

// g4[n,oy,ox,c] = bf16(dx_hat * x_hat * (1 - x_hat))   (backward of nn.Sigmoid, R.md:383, for an externally supplied dL/dx_hat)
// fp32 NCHW [B,C,H,W] in, bf16 NHWC-CP out; part[block][edge_lp_stride(C)] = {0, sum g(c) for c < C, zero padding} (bias gradient of
// deconv4)
template <int CP>
__global__ EAE_NO_PK __launch_bounds__(256) void sigmoid_bwd_kernel(const float* __restrict__ xh, const float* __restrict__ dxh, bf16_t* __restrict__ g4,
                                                           float* __restrict__ part, long npix_total, long plane, int C_) {
  const int C = edge_bands<CP>(C_);
  constexpr int CMAX = EdgeK<CP>::CMAX;
  __shared__ float red[4][1 + CMAX];
  const int LPS = edge_lp_stride(C);
  const long p = (long)blockIdx.x * 256 + threadIdx.x;      // pixel index n*H*W + oy*W + ox
  float g[CMAX];
#pragma unroll
  for (int c = 0; c < CMAX; ++c) g[c] = 0.f;
  if (p < npix_total) {
    const long n = p / plane, r = p % plane;
    uint32_t w[CP];
#pragma unroll
    for (int c = 0; c < CP; ++c) w[c] = 0u;
#pragma unroll
    for (int c = 0; c < CMAX; ++c) {
      if (c < C) {
        float x = xh[(n * C + c) * plane + r];
        w[c] = f2bf(dxh[(n * C + c) * plane + r] * x * (1.0f - x));
        g[c] = bf2f(w[c]);
      }
    }
    if constexpr (CP == 4) {
      *reinterpret_cast<uint2*>(g4 + p * 4) = make_uint2(w[0] | (w[1] << 16), w[2] | (w[3] << 16));
    } else {
#pragma unroll
      for (int q = 0; q < CP / 8; ++q)
        reinterpret_cast<uint4*>(g4 + p * CP)[q] = make_uint4(w[8 * q] | (w[8 * q + 1] << 16), w[8 * q + 2] | (w[8 * q + 3] << 16),
                                                              w[8 * q + 4] | (w[8 * q + 5] << 16), w[8 * q + 6] | (w[8 * q + 7] << 16));
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int c = 0; c < CMAX; ++c) {
    if (c < C) {
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) g[c] += __shfl_xor(g[c], o);
      if (lane == 0) red[wave][c + 1] = g[c];
    }
  }
  __syncthreads();
  if ((int)threadIdx.x < LPS)
    part[(size_t)blockIdx.x * LPS + threadIdx.x] = (threadIdx.x == 0 || (int)threadIdx.x > C) ? 0.f
        : red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
}

int eae_launch_sigmoid_bwd(hipStream_t st, const float* x_hat, const float* dx_hat, void* g4, float* part, int B, int H, int W, int C) {
  if (int rc = check_bands(C)) return rc;
  const long plane = (long)H * W, tot = plane * B;
  EAE_NO_GROUP("sigmoid_bwd");
  const dim3 grid((unsigned)((tot + 255) / 256));
  const int cp = edge_cp(C);
  if (cp == 4) hipLaunchKernelGGL(sigmoid_bwd_kernel<4>, grid, dim3(256), 0, st, x_hat, dx_hat, (bf16_t*)g4, part, tot, plane, C);
  else if (cp == 8) hipLaunchKernelGGL(sigmoid_bwd_kernel<8>, grid, dim3(256), 0, st, x_hat, dx_hat, (bf16_t*)g4, part, tot, plane, C);
  else hipLaunchKernelGGL(sigmoid_bwd_kernel<16>, grid, dim3(256), 0, st, x_hat, dx_hat, (bf16_t*)g4, part, tot, plane, C);
  EAE_LAUNCH_CHECK();
  return 0;
}

#ifdef EAE_STAMPS
extern "C" int eae_debug_set_edge(void* p, int block) {
  unsigned long long* q = static_cast<unsigned long long*>(p);
  EAE_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_edge_dbg), &q, sizeof(q)));
  EAE_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_edge_dbg_block), &block, sizeof(block)));
  return 0;
}
#endif
