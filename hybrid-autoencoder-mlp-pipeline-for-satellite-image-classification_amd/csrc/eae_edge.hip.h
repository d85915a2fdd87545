// Kernels for the two C-band "edge" layers (C = 1..16 image bands, 3 for RGB), which carry the most bytes and the least math
// (hard parts):
//   enc.conv1  (R.md:292)  x fp32 NCHW [B,C,H,W]            -> y1 [B,H/2,W/2,32]
//   dec.deconv4 (R.md:382) a3 [B,H/2,W/2,32] -> sigmoid -> x_hat [B,C,H,W], fused with MSE loss and its gradient
// The bands are padded to CP = 4 / 8 / 16 in LDS and in deconv4's bf16 output gradient only: K = 9*CP is padded to 64 / 96 / 160
// (2 / 3 / 5 v_mfma_f32_16x16x32_bf16 K-steps), and N = C is handled by computing the four sub-pixel phases jointly (N = 4 phases x C
// bands in 1, 2 or 4 MFMA column tiles: 12 of 16 columns for RGB), never by padding the fp32 image in HBM.
#pragma once
#include "eae_common.hip.h"
#include "eae_igemm.hip.h"
// (argument blocks EdgeArgs / Deconv4Args / Deconv4SceneArgs / SceneSrc, the SRC3_* kinds, edge_cp and edge_lp_stride: eae_args.h)

#ifdef EAE_STAMPS          // diagnostic build: s_memtime stamps of one workgroup of the edge kernels (tools/kstamp3.py)
__device__ unsigned long long* g_edge_dbg = nullptr;
__device__ int g_edge_dbg_block = 0;
#define EDGE_STAMP(i) do { if (g_edge_dbg && (int)blockIdx.x == g_edge_dbg_block && threadIdx.x == 0) { \
    unsigned long long t__; asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t__) :: "memory"); g_edge_dbg[i] = t__; } } while (0)
#else
#define EDGE_STAMP(i) do {} while (0)
#endif

template <int SRC3> constexpr bool src3_planar() { return SRC3 != SRC3_NHWCP_BF16; }

template <typename T> __device__ __forceinline__ float scene_val(T v, float d) { return (float)v / d; }
// The one border resolver: source index on an axis of length n of virtual coordinate v behind a leading pad p, or -1 for a constant
// pixel (whose stored value is fill).  s = v - p inside [0, n) is the pixel itself; EDGE clamps; REFLECT mirrors about the edge pixel
// without repeating it (one reflection: the pads are at most n - 1, eae_scene_check).
__device__ __forceinline__ int scene_resolve(int v, int p, int n, int mode) {
  const int s = v - p;
  if ((unsigned)s < (unsigned)n) return s;
  if (mode == EAE_BORDER_EDGE) return s < 0 ? 0 : n - 1;
  if (mode == EAE_BORDER_REFLECT) return s < 0 ? -s : 2 * (n - 1) - s;
  return -1;
}
// value of virtual pixel (vy, vx) of band plane x, as conv1 and deconv4's target both read it
template <typename T> __device__ __forceinline__ float scene_border_val(const T* x, const SceneBorder& b, int vy, int vx, float d) {
  const int sy = scene_resolve(vy, b.pt, b.Hs, b.mode), sx = scene_resolve(vx, b.pl, b.Ws, b.mode);
  return scene_val(sy < 0 || sx < 0 ? (T)b.fill : x[(long long)sy * b.Ws + sx], d);
}
// 4 consecutive scene pixels of one band: one vector load where the address allows it (window origins x are not aligned for most
// strides and scene widths), else 4 element loads
template <typename T> __device__ __forceinline__ float4 scene_load4(const T* p, float d) {
  T e[4];
  if ((reinterpret_cast<uintptr_t>(p) & (4 * sizeof(T) - 1)) == 0) {
    if constexpr (sizeof(T) == 1) { const uchar4 v = *reinterpret_cast<const uchar4*>(p); e[0] = v.x; e[1] = v.y; e[2] = v.z; e[3] = v.w; }
    else if constexpr (sizeof(T) == 2) { const ushort4 v = *reinterpret_cast<const ushort4*>(p); e[0] = v.x; e[1] = v.y; e[2] = v.z; e[3] = v.w; }
    else { const float4 v = *reinterpret_cast<const float4*>(p); e[0] = v.x; e[1] = v.y; e[2] = v.z; e[3] = v.w; }
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) e[i] = p[i];
  }
  return make_float4(scene_val(e[0], d), scene_val(e[1], d), scene_val(e[2], d), scene_val(e[3], d));
}
template <int SRC3> struct SceneElem { using T = float; };
template <> struct SceneElem<SRC3_SCENE_U8> { using T = uint8_t; };
template <> struct SceneElem<SRC3_SCENE_U16> { using T = uint16_t; };

template <int CP> __device__ __forceinline__ int edge_bands(int C) { return CP == 4 ? 3 : C; }
template <int CP> struct EdgeK {
  static constexpr int CMAX = CP == 4 ? 3 : CP;       // most bands a CP form takes
  static constexpr int KP = (9 * CP + 31) / 32 * 32;  // packed conv K (k = tap*CP + c): 64, 96, 160
  static constexpr int KS = KP / 32;                  // v_mfma_f32_16x16x32_bf16 k-steps: 2, 3, 5
  static constexpr int KC = (9 * CMAX + 31) / 32;     // 32-wide im2col chunks of the weight gradient (k = tap*C + c): at most 1, 3, 5
  static constexpr int NT = CP / 4;                   // deconv4: 16-column MFMA tiles of the 4 phases x C outputs
};

constexpr int E_TH = 4, E_TW = 32;                 // 128 output pixels (conv view) / 128 input positions (deconv view)
constexpr int E_PH = 2 * E_TH + 1, E_PW = 2 * E_TW + 1;   // 9 x 65 patch of the C-band tensor
template <int CP> constexpr int e_patch() { return E_PH * E_PW * CP; }     // bf16 elements ([row][col][CP])
constexpr int E_AT = 128 * PIX_STRIDE;             // im2col tile [128][32 + pad]

// Stage the C-band patch (rows iy0.., cols ix0..) as bf16 [E_PH][E_PW][CP] with zero padding outside the image and in bands >= C.
// Every pixel of the patch is written exactly once, as whole CP-band pixels: a thread takes 4 consecutive pixels of a row -- for the
// planar fp32 source one float4 per band -- and writes them with 8-byte (CP = 4) or 16-byte stores (the patch starts one pixel
// left of a 16-byte boundary: the halo column).  Round 2 cleared the patch, synchronised, and scattered 2-byte elements plane by
// plane (12 ds_write_b16 per float4 triple): by the stamps 4.8-8.5 K of conv1's 9.5-14.6 K workgroup cycles.  One barrier, at the end.
// (split into a load and a write half so that a loop over tiles can keep the NEXT tile's raw values in flight: edge_wgrad_kernel)
template <int CP> constexpr int e_pieces_row() { return 8 * CP; }                 // 16-byte pieces of a row's 64 interior pixels
template <int CP> constexpr int e_halo_row() { return CP == 4 ? 1 : CP / 8; }     // pieces of the halo pixel (CP = 4: half a piece)
template <int CP> constexpr int e_nld() { return (E_PH * (e_pieces_row<CP>() + e_halo_row<CP>()) + 255) / 256; }
template <int SRC3, int CP> struct Patch3Regs { float4 v[EdgeK<CP>::CMAX]; };     // planar fp32: one float4 per band (halo threads: .x only)
template <int CP> struct Patch3Regs<SRC3_NHWCP_BF16, CP> { uint4 v[e_nld<CP>()]; };   // bf16 NHWC-CP: 16-byte pieces
template <int SRC3, int CP, bool IDX = false, bool BORDER = false>
__device__ __forceinline__ void patch3_load(const void* src, int C, int n, int H, int W, int iy0, int ix0, Patch3Regs<SRC3, CP>& r,
                                            const SceneSrc* sc = nullptr) {
  const int tid = threadIdx.x;
  if constexpr (SRC3 >= SRC3_SCENE_U8) {
    // window-local coordinates: the conv padding outside the window stays zero, even where the scene has pixels there
    using T = typename SceneElem<SRC3>::T;
    const T* x = static_cast<const T*>(sc->data);
    constexpr int CMAX = EdgeK<CP>::CMAX;
    long long w = sc->first + n;
    if constexpr (IDX) w = sc->index[w];                 // one uniform load per workgroup
    const long long wi = w / sc->nW, wj = w - wi * sc->nW;
    const long long org = wi * sc->S * (long long)sc->Ws + wj * sc->S;
#pragma unroll
    for (int c = 0; c < CMAX; ++c) r.v[c] = make_float4(0.f, 0.f, 0.f, 0.f);
    if constexpr (IDX)
      if (w < 0 || w >= sc->nwin) return;
    if constexpr (BORDER) {
      // virtual coordinates (vy, vx) of the window's pixels.  The row resolves once per thread; a thread whose four virtual columns are
      // real ones takes the vector path of the borderless form, else four resolved element loads (or the fill): only the workgroups
      // of windows at the border diverge.
      const int vy0 = (int)wi * sc->S, vx0 = (int)wj * sc->S;
      if (tid < E_PH * 16) {
        const int c4 = tid & 15, rr = tid >> 4;
        const int iy = iy0 + rr, ix = ix0 + 1 + c4 * 4;
        if (iy >= 0 && iy < H) {
          const int sy = scene_resolve(vy0 + iy, sc->b.pt, sc->b.Hs, sc->b.mode), sx0 = vx0 + ix - sc->b.pl;
          if (sy >= 0 && sx0 >= 0 && sx0 + 3 < sc->Ws) {
            const T* p = x + (long long)sy * sc->Ws + sx0;
#pragma unroll
            for (int c = 0; c < CMAX; ++c)
              if (c < C) r.v[c] = scene_load4<T>(p + c * sc->plane, sc->div[c]);
          } else {
            int sx[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) sx[e] = sy < 0 ? -1 : scene_resolve(vx0 + ix + e, sc->b.pl, sc->Ws, sc->b.mode);
            const T* p = x + (long long)(sy < 0 ? 0 : sy) * sc->Ws;
#pragma unroll
            for (int c = 0; c < CMAX; ++c)
              if (c < C) {
                const T* q = p + c * sc->plane;
                const float d = sc->div[c];
                const T f = (T)sc->b.fill;
                r.v[c] = make_float4(scene_val(sx[0] < 0 ? f : q[sx[0]], d), scene_val(sx[1] < 0 ? f : q[sx[1]], d),
                                     scene_val(sx[2] < 0 ? f : q[sx[2]], d), scene_val(sx[3] < 0 ? f : q[sx[3]], d));
              }
          }
        }
      } else if (tid < E_PH * 16 + E_PH) {
        const int iy = iy0 + tid - E_PH * 16;
        if (ix0 >= 0 && iy >= 0 && iy < H) {
#pragma unroll
          for (int c = 0; c < CMAX; ++c)
            if (c < C) r.v[c].x = scene_border_val<T>(x + c * sc->plane, sc->b, vy0 + iy, vx0 + ix0, sc->div[c]);
        }
      }
      return;
    }
    if (tid < E_PH * 16) {
      const int c4 = tid & 15, rr = tid >> 4;
      const int iy = iy0 + rr, ix = ix0 + 1 + c4 * 4;
      if (iy >= 0 && iy < H) {
        const T* p = x + org + (long long)iy * sc->Ws + ix;
#pragma unroll
        for (int c = 0; c < CMAX; ++c)
          if (c < C) r.v[c] = scene_load4<T>(p + c * sc->plane, sc->div[c]);
      }
    } else if (tid < E_PH * 16 + E_PH) {
      const int iy = iy0 + tid - E_PH * 16;
      if (ix0 >= 0 && iy >= 0 && iy < H) {
        const T* p = x + org + (long long)iy * sc->Ws + ix0;
#pragma unroll
        for (int c = 0; c < CMAX; ++c)
          if (c < C) r.v[c].x = scene_val(p[c * sc->plane], sc->div[c]);
      }
    }
  } else if constexpr (SRC3 == SRC3_NCHW_F32) {
    const float* x = static_cast<const float*>(src);
    constexpr int CMAX = EdgeK<CP>::CMAX;
#pragma unroll
    for (int c = 0; c < CMAX; ++c) r.v[c] = make_float4(0.f, 0.f, 0.f, 0.f);
    // interior columns ix0+1 .. ix0+64 are image columns (ix0 = 2*tx0-1, tx0 multiple of 32 -> 16-byte aligned rows)
    if (tid < E_PH * 16) {
      const int c4 = tid & 15, rr = tid >> 4;
      const int iy = iy0 + rr, ix = ix0 + 1 + c4 * 4;
      if (iy >= 0 && iy < H) {
#pragma unroll
        for (int c = 0; c < CMAX; ++c)
          if (c < C) r.v[c] = *reinterpret_cast<const float4*>(x + (((size_t)n * C + c) * H + iy) * W + ix);
      }
    } else if (tid < E_PH * 16 + E_PH) {          // left halo column: a real pixel for tiles not at the image edge, else zero padding
      const int iy = iy0 + tid - E_PH * 16;
      if (ix0 >= 0 && iy >= 0 && iy < H) {
#pragma unroll
        for (int c = 0; c < CMAX; ++c)
          if (c < C) r.v[c].x = x[(((size_t)n * C + c) * H + iy) * W + ix0];
      }
    }
  } else {
    const bf16_t* g = static_cast<const bf16_t*>(src);
    constexpr int IPR = e_pieces_row<CP>(), HPR = e_halo_row<CP>();
#pragma unroll
    for (int k = 0; k < e_nld<CP>(); ++k) {
      const int i = tid + k * 256;
      r.v[k] = make_uint4(0, 0, 0, 0);
      if (i < E_PH * IPR) {                       // 16-byte pieces of the interior pixels
        const int pc = i % IPR, rr = i / IPR;
        const int iy = iy0 + rr;
        if (iy >= 0 && iy < H) r.v[k] = *reinterpret_cast<const uint4*>(g + (((size_t)n * H + iy) * W + ix0 + 1) * CP + pc * 8);
      } else if (i < E_PH * (IPR + HPR)) {        // the halo column
        const int j = i - E_PH * IPR, rr = j / HPR, hp = j % HPR;
        const int iy = iy0 + rr;
        if (ix0 >= 0 && iy >= 0 && iy < H) {
          if constexpr (CP == 4) {
            const uint2 h = *reinterpret_cast<const uint2*>(g + (((size_t)n * H + iy) * W + ix0) * CP);
            r.v[k].x = h.x; r.v[k].y = h.y;
          } else {
            r.v[k] = *reinterpret_cast<const uint4*>(g + (((size_t)n * H + iy) * W + ix0) * CP + hp * 8);
          }
        }
      }
    }
  }
}
template <int SRC3, int CP>
__device__ __forceinline__ void patch3_write(bf16_t* p3, const Patch3Regs<SRC3, CP>& r) {
  const int tid = threadIdx.x;
  if constexpr (src3_planar<SRC3>()) {
    constexpr int CMAX = EdgeK<CP>::CMAX;
    auto put = [&](bf16_t* d, int e) __attribute__((always_inline)) {
      uint32_t w[CP / 2];
#pragma unroll
      for (int c = 0; c < CP; c += 2) {
        const float lo = c >= CMAX ? 0.f : e == 0 ? r.v[c].x : e == 1 ? r.v[c].y : e == 2 ? r.v[c].z : r.v[c].w;
        const float hi = c + 1 >= CMAX ? 0.f : e == 0 ? r.v[c + 1].x : e == 1 ? r.v[c + 1].y : e == 2 ? r.v[c + 1].z : r.v[c + 1].w;
        w[c / 2] = c >= CMAX ? 0u : c + 1 >= CMAX ? f2bf(lo) : pack2(lo, hi);
      }
      if constexpr (CP == 4) {
        *reinterpret_cast<uint2*>(d) = make_uint2(w[0], w[1]);
      } else {
#pragma unroll
        for (int q = 0; q < CP / 8; ++q) reinterpret_cast<uint4*>(d)[q] = make_uint4(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]);
      }
    };
    if (tid < E_PH * 16) {
      const int c4 = tid & 15, rr = tid >> 4;
      bf16_t* d = p3 + (rr * E_PW + 1 + c4 * 4) * CP;
      put(d, 0); put(d + CP, 1); put(d + 2 * CP, 2); put(d + 3 * CP, 3);
    } else if (tid < E_PH * 16 + E_PH) {
      put(p3 + ((tid - E_PH * 16) * E_PW) * CP, 0);
    }
  } else {
    constexpr int IPR = e_pieces_row<CP>(), HPR = e_halo_row<CP>();
#pragma unroll
    for (int k = 0; k < e_nld<CP>(); ++k) {
      const int i = tid + k * 256;
      if (i < E_PH * IPR) {
        const int pc = i % IPR, rr = i / IPR;
        bf16_t* d = p3 + (rr * E_PW + 1) * CP + pc * 8;
        if constexpr (CP == 4) {         // 8-byte aligned only (the interior starts one 8-byte pixel into the row)
          reinterpret_cast<uint2*>(d)[0] = make_uint2(r.v[k].x, r.v[k].y);
          reinterpret_cast<uint2*>(d)[1] = make_uint2(r.v[k].z, r.v[k].w);
        } else {
          *reinterpret_cast<uint4*>(d) = r.v[k];
        }
      } else if (i < E_PH * (IPR + HPR)) {
        const int j = i - E_PH * IPR, rr = j / HPR, hp = j % HPR;
        if constexpr (CP == 4) *reinterpret_cast<uint2*>(p3 + (rr * E_PW) * CP) = make_uint2(r.v[k].x, r.v[k].y);
        else *reinterpret_cast<uint4*>(p3 + (rr * E_PW) * CP + hp * 8) = r.v[k];
      }
    }
  }
}
template <int SRC3, int CP, bool IDX = false, bool BORDER = false>
__device__ __forceinline__ void stage_patch3(const void* src, int C, bf16_t* p3, int n, int H, int W, int iy0, int ix0,
                                             const SceneSrc* sc = nullptr) {
  Patch3Regs<SRC3, CP> r;
  patch3_load<SRC3, CP, IDX, BORDER>(src, C, n, H, W, iy0, ix0, r, sc);
  patch3_write<SRC3, CP>(p3, r);
  __syncthreads();
}

// im2col of the weight gradient: k = tap*C + c (K = 9C, zero for k >= 9C), in 32-wide chunks.  A thread fills the same 8 k of
// every tile (kg = tid & 3): their patch offsets (or -1) are computed once, before the tile loop.
template <int CP>
__device__ __forceinline__ void im2col_offsets(int C, int kc, int (&off)[8]) {
  const int kg = threadIdx.x & 3;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int k = kc * 32 + kg * 8 + j;
    const int tap = k / C, c = k % C;
    off[j] = (k < 9 * C) ? ((tap / 3) * E_PW + tap % 3) * CP + c : -1;
  }
}
// Build the im2col tile [128 pixels][32 k] of one chunk from the staged patch.
template <int CP>
__device__ __forceinline__ void build_im2col(const bf16_t* p3, bf16_t* at, const int (&off)[8]) {
  const int tid = threadIdx.x;
  if constexpr (CP == 4) {          // RGB: k = tap*3 + c (zero for k >= 27), as the 3-band kernel had it
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      int q = tid + i * 256;
      int m = q >> 2, kg = q & 3;
      int ty = m / E_TW, tx = m % E_TW;
      uint32_t w[4];
#pragma unroll
      for (int j = 0; j < 8; j += 2) {
        uint32_t e[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          int k = kg * 8 + j + u;
          int tap = k / 3, c = k % 3;
          int ky = tap / 3, kx = tap % 3;
          e[u] = (k < 27) ? (uint32_t)p3[((2 * ty + ky) * E_PW + 2 * tx + kx) * 4 + c] : 0u;
        }
        w[j >> 1] = e[0] | (e[1] << 16);
      }
      *reinterpret_cast<uint4*>(at + m * PIX_STRIDE + kg * 8) = make_uint4(w[0], w[1], w[2], w[3]);
    }
    return;
  }
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    int q = tid + i * 256;
    int m = q >> 2, kg = q & 3;
    int ty = m / E_TW, tx = m % E_TW;
    const bf16_t* pb = p3 + ((2 * ty) * E_PW + 2 * tx) * CP;
    uint32_t w[4];
#pragma unroll
    for (int j = 0; j < 8; j += 2) {
      uint32_t e[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) e[u] = off[j + u] >= 0 ? (uint32_t)pb[off[j + u]] : 0u;
      w[j >> 1] = e[0] | (e[1] << 16);
    }
    *reinterpret_cast<uint4*>(at + m * PIX_STRIDE + kg * 8) = make_uint4(w[0], w[1], w[2], w[3]);
  }
}

// ---------------------------------------------------------------------------------------------------------------
// out[m][32] = im2col(src)[m][9C] . Wp[32][9C]^T      (conv1 forward; backward-data of deconv4)
// ---------------------------------------------------------------------------------------------------------------

// No im2col tile: with k = tap*CP + c (bands >= C and k >= 9*CP are zero in the weights: K = KP, 2 / 3 / 5 MFMA k-steps) a lane's 8
// consecutive k are whole pixel pieces of the staged [row][col][CP] patch (two pixels for CP = 4, one for 8, half a pixel for 16), so
// the pixel operand is read straight from the patch.  The weights are the MFMA A operand: an accumulator lane holds 4 consecutive
// output channels of one pixel (8-byte tile writes instead of 16 two-byte ones).
template <int SRC3, int EPI, int CP, bool IDX = false, bool BORDER = false>
__device__ __forceinline__ void edge_conv_body(const EdgeArgs& a, const SceneSrc* sc = nullptr) {
  constexpr int KP = EdgeK<CP>::KP, KS = EdgeK<CP>::KS;
  __shared__ __attribute__((aligned(16))) bf16_t p3[e_patch<CP>()];
  // output tile [128][40] (10 KB); the statistics reduction scratch [2][64][32] floats (16 KB) reuses the same memory: TileEpilogue::end()
  // starts with a barrier behind the last read of the tile (31.3 -> 20.7 KB of LDS per block: 7 instead of 5 blocks per CU)
  __shared__ __attribute__((aligned(16))) float red[2 * 64 * 32];
  static_assert(sizeof(float) * 2 * 64 * 32 >= sizeof(bf16_t) * E_AT, "the tile must fit the reduction scratch");
  bf16_t* const at = reinterpret_cast<bf16_t*>(red);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int Hout = a.H >> 1, Wout = a.W >> 1;
  const int tiles_x = Wout / E_TW, tiles_y = Hout / E_TH;
  int t = blockIdx.x;
  const int txb = t % tiles_x; t /= tiles_x;
  const int tyb = t % tiles_y; t /= tiles_y;
  const int n = t;
  const int kgl = lane >> 4;
  eae_signal(a.c.sig, a.c.sig_val);
  // weight fragments first (independent of the patch): A[channel][k], 2 m-tiles x KS k-steps
  bf16x8 wf[2][KS];
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
      wf[mt][ks] = *reinterpret_cast<const bf16x8*>(a.c.wpack + (mt * 16 + (lane & 15)) * KP + ks * 32 + kgl * 8);
  EDGE_STAMP(16);
  stage_patch3<SRC3, CP, IDX, BORDER>(a.src3, edge_bands<CP>(a.C), p3, n, a.H, a.W, 2 * tyb * E_TH - 1, 2 * txb * E_TW - 1, sc);  // ends with a barrier
  EDGE_STAMP(17);
  f32x4 acc[2][2];
#pragma unroll
  for (int nt = 0; nt < 2; ++nt) {
    const int m = (wave * 2 + nt) * 16 + (lane & 15);                // this lane's pixel of the n-tile
    const int ty = m / E_TW, tx = m % E_TW;
    const bf16_t* pb = p3 + ((2 * ty) * E_PW + 2 * tx) * CP;
    if constexpr (CP == 4) {
      // RGB, as the 3-band kernel: k-step 0 = taps 2*kgl and 2*kgl+1; k-step 1 = tap 8 (lane group 0 only), everything else
      // multiplies zero weights
      const int t0 = 2 * kgl, t1 = 2 * kgl + 1;
      union { bf16x8 v; uint2 h[2]; } f0, f1;
      f0.h[0] = *reinterpret_cast<const uint2*>(pb + ((t0 / 3) * E_PW + (t0 % 3)) * 4);
      f0.h[1] = *reinterpret_cast<const uint2*>(pb + ((t1 / 3) * E_PW + (t1 % 3)) * 4);
      f1.h[0] = (kgl == 0) ? *reinterpret_cast<const uint2*>(pb + (2 * E_PW + 2) * 4) : make_uint2(0, 0);
      f1.h[1] = make_uint2(0, 0);
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) {
        acc[mt][nt] = mfma16(wf[mt][0], f0.v, (f32x4){0.f, 0.f, 0.f, 0.f});
        acc[mt][nt] = mfma16(wf[mt][1], f1.v, acc[mt][nt]);
      }
    } else {
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        // this lane's k = ks*32 + kgl*8 .. +7 = half (CP = 16) or all (CP = 8) of one tap's pixel; taps >= 9 multiply zero weights
        const int k0 = ks * 32 + kgl * 8;
        const int tap = k0 / CP, c0 = k0 % CP;
        union { bf16x8 v; uint4 q; } f;
        f.q = tap < 9 ? *reinterpret_cast<const uint4*>(pb + ((tap / 3) * E_PW + (tap % 3)) * CP + c0) : make_uint4(0, 0, 0, 0);
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) acc[mt][nt] = mfma16(wf[mt][ks], f.v, ks == 0 ? (f32x4){0.f, 0.f, 0.f, 0.f} : acc[mt][nt]);
      }
    }
  }
  // D[channel][pixel]: col = lane & 15 = pixel, rows (lane >> 4) * 4 + r = 4 consecutive channels
#pragma unroll
  for (int mt = 0; mt < 2; ++mt) {
    const int ch = mt * 16 + (lane >> 4) * 4;
    float4 bv = make_float4(0.f, 0.f, 0.f, 0.f);
    if (EPI == EPI_FWD) bv = *reinterpret_cast<const float4*>(a.c.bias + ch);
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
      const int m = (wave * 2 + nt) * 16 + (lane & 15);
      uint2 w2;
      w2.x = pk2((f32x2){acc[mt][nt][0] + bv.x, acc[mt][nt][1] + bv.y});
      w2.y = pk2((f32x2){acc[mt][nt][2] + bv.z, acc[mt][nt][3] + bv.w});
      *reinterpret_cast<uint2*>(at + m * 40 + ch) = w2;
    }
  }
  EDGE_STAMP(18);
  __syncthreads();
  // output window: the tile's E_TH output rows of image n
  auto rowmap = [=](int row) -> long {
    int ty = row / E_TW, tx = row % E_TW;
    return (ty * Wout + (txb * E_TW + tx)) * 32;
  };
  tile_epilogue<32, 32, EPI>(a.c, at, red, 0, blockIdx.x, 128, ((long)n * Hout + tyb * E_TH) * Wout * 32, (long)E_TH * Wout * 32, rowmap);
  EDGE_STAMP(19);
}
template <int SRC3, int EPI, int CP>
__global__ __launch_bounds__(256) void edge_conv_kernel(EdgeArgs a) { edge_conv_body<SRC3, EPI, CP>(a); }
template <int SRC3, int EPI, int CP>
__global__ __launch_bounds__(256) void edge_conv_kernel_g(GroupPack<EdgeArgs> p, int gz) { edge_conv_body<SRC3, EPI, CP>(group_args<EdgeArgs>(gz)); }
// conv1 reading P x P windows of a device-resident scene (eae_scene_encode / eae_scene_classify; eval-mode forward); IDX: the windows
// of the launch come from s.index (eae_scene_encode_windows / eae_scene_classify_windows); BORDER: the grid lies over the virtual
// padded scene (s.border and the fields behind it).  The flag keeps the borderless instantiations the code they were.
template <int SRC3, int CP, bool IDX = false, bool BORDER = false>
__global__ __launch_bounds__(256) void edge_conv_scene_kernel(EdgeArgs a, SceneSrc s) { edge_conv_body<SRC3, EPI_FWD, CP, IDX, BORDER>(a, &s); }

// ---------------------------------------------------------------------------------------------------------------
// R[k][c] = sum_m im2col(src)[m][k] * T(side)[m][c]     (weight gradient of conv1 and of deconv4)
// Each block sweeps `tiles_per_block` 128-pixel tiles and writes one fp32 partial in the REFERENCE layout
// [c][C][3][3] (index c*9C + cx*9 + tap with k = tap*C + cx), summed later by reduce_slices (deterministic).
// ---------------------------------------------------------------------------------------------------------------
struct EdgeWgradArgs {
  const void* src3;
  int B, H, W;
  SrcDesc side;           // [B,H/2,W/2,32] tensor with its load transform
  float* part;            // [nblocks][32*9C]
  int tiles_per_block, ntiles;
  BnBwdFold bfold;        // SRC_BNBWD side: coefficient table from the layer's backward accumulators (eae_common.hip.h)
  unsigned* sig;          // progress word of the caller's stream, published when the kernel starts (ConvArgs::sig); nullptr: none
  unsigned sig_val;
  int C;                  // bands (1..16; edge_cp(C) == CP)
};

template <int SRC3, int SMODE, int CP>
__device__ __forceinline__ void edge_wgrad_body(const EdgeWgradArgs& a) {
  constexpr int KC = EdgeK<CP>::KC;
  eae_signal(a.sig, a.sig_val);
  __shared__ __attribute__((aligned(16))) bf16_t p3[e_patch<CP>()];
  // the two operand tiles (im2col chunk, side); the cross-wave reduction image of the epilogue (16 KB) reuses them (41.9 -> 26 KB of
  // LDS per block: 6 instead of 3 blocks per CU).  More than one 32-wide k chunk (C > 3) goes through the im2col tile in turn.
  static_assert(2 * E_AT * sizeof(bf16_t) >= 4 * 2 * 2 * 64 * 4 * sizeof(float), "reduction image must fit the operand tiles");
  __shared__ __attribute__((aligned(16))) bf16_t tiles[2 * E_AT];
  bf16_t* const at = tiles;
  bf16_t* const st = tiles + E_AT;
  float (*racc)[2][2][64 * 4] = reinterpret_cast<float (*)[2][2][64 * 4]>(tiles);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int C = edge_bands<CP>(a.C), nkc = (9 * C + 31) / 32;
  const int Hout = a.H >> 1, Wout = a.W >> 1;
  const int tiles_x = Wout / E_TW, tiles_y = Hout / E_TH;
  const int kgs = tid & 3;
  ChanCoef<SMODE> cc;
  {
    __shared__ float coef_tab[SMODE == SRC_BNBWD ? 3 * 32 : 4];
    const float* coefp = a.side.coef;
    if (SMODE == SRC_BNBWD && a.bfold.acc != nullptr) {      // folded BatchNorm-backward finalize (this kernel is the layer's only consumer)
      BnFoldRegsB fr;
      bn_fold_bwd_load<32>(a.bfold, fr);
      bn_fold_bwd_finish<32>(a.bfold, fr, coef_tab, reinterpret_cast<long long*>(&racc[0][0][0][0]), blockIdx.x == 0);
      coefp = coef_tab;
    }
    cc.load(coefp, 32, kgs * 8);
  }
  int off[KC][8];
  if constexpr (CP != 4) {
#pragma unroll
    for (int kc = 0; kc < KC; ++kc) im2col_offsets<CP>(C, kc, off[kc]);
  }
  f32x4 acc[KC][2][2];
#pragma unroll
  for (int kc = 0; kc < KC; ++kc)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[kc][i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const int g = lane >> 4, q = (lane & 15) >> 2, p = lane & 3;
  // Tile loop with the NEXT tile's raw values (side pieces + C-band patch) requested before this tile is multiplied: round 2
  // loaded, staged and multiplied one tile after the other, every tile exposing a memory round trip (conv1's weight gradient is the
  // last kernel of the backward: 32 us on the critical path).
  const int t_begin = blockIdx.x * a.tiles_per_block;
  int t_end = t_begin + a.tiles_per_block;
  if (t_end > a.ntiles) t_end = a.ntiles;
  RawPiece<SMODE> raw[2];
  Patch3Regs<SRC3, CP> pr;
  auto request = [&](int t) __attribute__((always_inline)) {
    const int txb = t % tiles_x; t /= tiles_x;
    const int tyb = t % tiles_y; t /= tiles_y;
    const int n = t;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      int m = (tid + i * 256) >> 2;
      int ty = m / E_TW, tx = m % E_TW;
      size_t off = ((((size_t)n * Hout + tyb * E_TH + ty) * Wout) + txb * E_TW + tx) * 32 + kgs * 8;
      load_piece<SMODE>(a.side, off, true, raw[i]);
    }
    patch3_load<SRC3, CP>(a.src3, C, n, a.H, a.W, 2 * tyb * E_TH - 1, 2 * txb * E_TW - 1, pr);
  };
  if (t_begin < t_end) request(t_begin);
  for (int t = t_begin; t < t_end; ++t) {
    __syncthreads();                 // the previous tile's fragment reads (at, st) and im2col reads (p3) are done
    patch3_write<SRC3, CP>(p3, pr);
    uint4 sv[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) sv[i] = transform_piece<SMODE>(raw[i], true, cc);
    if (t + 1 < t_end) request(t + 1);
    __syncthreads();                 // the C-band patch is complete
    build_im2col<CP>(p3, at, off[0]);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      int m = (tid + i * 256) >> 2;
      *reinterpret_cast<uint4*>(st + m * PIX_STRIDE + kgs * 8) = sv[i];
    }
    __syncthreads();
    // wave w reduces pixels 32w .. 32w+31
    const int r_lo = wave * 32 + 8 * g + q, r_hi = r_lo + 4;
    bf16x8 ka[2], sb[2];
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      ka[it] = tr_frag(at + r_lo * PIX_STRIDE + it * 16 + 4 * p, at + r_hi * PIX_STRIDE + it * 16 + 4 * p);
      sb[it] = tr_frag(st + r_lo * PIX_STRIDE + it * 16 + 4 * p, st + r_hi * PIX_STRIDE + it * 16 + 4 * p);
    }
#pragma unroll
    for (int it = 0; it < 2; ++it)
#pragma unroll
      for (int jt = 0; jt < 2; ++jt) acc[0][it][jt] = mfma16(ka[it], sb[jt], acc[0][it][jt]);
#pragma unroll
    for (int kc = 1; kc < KC; ++kc) {          // further k chunks (C > 3): rebuild the im2col tile
      if (kc < nkc) {
        __syncthreads();
        build_im2col<CP>(p3, at, off[kc]);
        __syncthreads();
#pragma unroll
        for (int it = 0; it < 2; ++it) ka[it] = tr_frag(at + r_lo * PIX_STRIDE + it * 16 + 4 * p, at + r_hi * PIX_STRIDE + it * 16 + 4 * p);
#pragma unroll
        for (int it = 0; it < 2; ++it)
#pragma unroll
          for (int jt = 0; jt < 2; ++jt) acc[kc][it][jt] = mfma16(ka[it], sb[jt], acc[kc][it][jt]);
      }
    }
  }
  // cross-wave reduction (fixed order) and store in reference layout, one 32-wide k chunk at a time
  OutRsrc po;      // window: this block's partial
  po.init(a.part + (size_t)blockIdx.x * (32 * 9 * C), (long)(32 * 9 * C) * 4);
#pragma unroll
  for (int kc = 0; kc < KC; ++kc) {
    if (kc >= nkc) break;
    __syncthreads();            // every wave has read its fragments of the last tile / the previous chunk's image: the image may overwrite the tiles
#pragma unroll
    for (int it = 0; it < 2; ++it)
#pragma unroll
      for (int jt = 0; jt < 2; ++jt)
#pragma unroll
        for (int r = 0; r < 4; ++r) racc[wave][it][jt][lane * 4 + r] = acc[kc][it][jt][r];
    __syncthreads();
    // 4 (it,jt) tiles x 256 values = 1024 outputs; thread handles 4
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      int e = tid + i * 256;
      int tile = e >> 8, idx = e & 255;
      int it = tile >> 1, jt = tile & 1;
      float v = racc[0][it][jt][idx] + racc[1][it][jt][idx] + racc[2][it][jt][idx] + racc[3][it][jt][idx];
      int l = idx >> 2, r = idx & 3;
      int k = kc * 32 + it * 16 + (l >> 4) * 4 + r;     // D row  = k index (im2col side)
      int c = jt * 16 + (l & 15);                        // D col  = side channel
      if (k < 9 * C) {
        int tap = k / C, cx = k % C;
        po.st4<EAE_WT_EDGE>((uint32_t)(c * 9 * C + cx * 9 + tap) * 4u, v);
      }
    }
  }
}
template <int SRC3, int SMODE, int CP>
__global__ __launch_bounds__(256) void edge_wgrad_kernel(EdgeWgradArgs a) { edge_wgrad_body<SRC3, SMODE, CP>(a); }
template <int SRC3, int SMODE, int CP>
__global__ __launch_bounds__(256) void edge_wgrad_kernel_g(GroupPack<EdgeWgradArgs> p, int gz) { edge_wgrad_body<SRC3, SMODE, CP>(group_args<EdgeWgradArgs>(gz)); }

// ---------------------------------------------------------------------------------------------------------------
// deconv4 forward (all four phases jointly) + sigmoid + MSE loss + its gradient      (R.md:382-383, 622, 649)
//   s[n,oy,ox,co] = b[co] + sum over the 2x2 input neighbourhood ;  x_hat = sigmoid(s)
//   loss partial  = sum (x_hat - x)^2 ;  g = gscale * (x_hat - x) * x_hat * (1 - x_hat)   (gscale = alpha*2/numel)
// ---------------------------------------------------------------------------------------------------------------

template <int SRC, int CP>
__device__ __forceinline__ void deconv4_loss_body(const Deconv4Args& a) {
  constexpr int PH = E_TH + 1, PW = E_TW + 1, NPIX = PH * PW;       // 5 x 33 input pixels
  constexpr int NPA = (NPIX * 4 + 255) / 256;
  constexpr int NT = EdgeK<CP>::NT, SLW = 16 * NT + 1;              // pre-sigmoid tile [128][16*NT + 1] floats
  constexpr int PATCH_B = (int)sizeof(bf16_t) * NPIX * PIX_STRIDE, SL_B = (int)sizeof(float) * 128 * SLW;
  // the pre-sigmoid tile `sl` (8.7 KB for CP = 4) reuses the patch (13.2 KB) once every wave has read its fragments: 8 blocks per CU
  __shared__ __attribute__((aligned(16))) bf16_t patch[(PATCH_B > SL_B ? PATCH_B : SL_B) / 2];
  float* const sl = reinterpret_cast<float*>(patch);
  __shared__ float redl[4][1 + EdgeK<CP>::CMAX];
  const int C = edge_bands<CP>(a.C), LPS = edge_lp_stride(C);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int Hout = a.Hin * 2, Wout = a.Win * 2;
  const int tiles_x = a.Win / E_TW, tiles_y = a.Hin / E_TH;
  int t = blockIdx.x;
  const int txb = t % tiles_x; t /= tiles_x;
  const int tyb = t % tiles_y; t /= tiles_y;
  const int n = t;
  const int iy0 = tyb * E_TH, ix0 = txb * E_TW;
  const int kgs = tid & 3, kgl = lane >> 4;
  ChanCoef<SRC> cc;
  BnFoldRegs fr;
  const bool folded = SRC == SRC_BNRELU && a.fold.acc != nullptr;
  EDGE_STAMP(0);
  if (folded) bn_fold_load<32>(a.fold, fr);       // before the patch loads: results return in issue order
  RawPiece<SRC> raw[NPA];
  bool val[NPA];
#pragma unroll
  for (int i = 0; i < NPA; ++i) {
    int qq = tid + i * 256;
    int pix = qq >> 2;
    int pr = pix / PW, pc = pix % PW;
    int iy = iy0 + pr, ix = ix0 + pc;
    val[i] = (pix < NPIX) && (iy < a.Hin) && (ix < a.Win);
    size_t off = (((size_t)n * a.Hin + iy) * a.Win + ix) * 32 + kgs * 8;
    load_piece<SRC>(a.src, off, val[i], raw[i]);
  }
  {   // coefficient table of the 32-channel source layer (folded BatchNorm finalize) while the loads are in flight
    __shared__ float coef_tab[4 * 32];
    const float* coefp = a.src.coef;
    if (folded) {
      bn_fold_fwd_finish<32>(a.fold, fr, coef_tab, reinterpret_cast<long long*>(sl), blockIdx.x == 0);
      coefp = coef_tab;
    }
    cc.load(coefp, 32, kgs * 8);
  }
  EDGE_STAMP(1);
#pragma unroll
  for (int i = 0; i < NPA; ++i) {
    int qq = tid + i * 256;
    if (qq < NPIX * 4)
      *reinterpret_cast<uint4*>(patch + (qq >> 2) * PIX_STRIDE + kgs * 8) = transform_piece<SRC>(raw[i], val[i], cc);
  }
  EDGE_STAMP(2);
  __syncthreads();
  EDGE_STAMP(3);
  f32x4 acc[NT][2];
#pragma unroll
  for (int j = 0; j < NT; ++j) acc[j][0] = acc[j][1] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int nb = 0; nb < 4; ++nb) {
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      bf16x8 bfr = *reinterpret_cast<const bf16x8*>(a.wjoint + (j * 16 + (lane & 15)) * 128 + nb * 32 + kgl * 8);
#pragma unroll
      for (int mi = 0; mi < 2; ++mi) {
        int pos = (wave * 2 + mi) * 16 + (lane & 15);
        int ty = pos / E_TW, tx = pos % E_TW;
        bf16x8 af = *reinterpret_cast<const bf16x8*>(patch + ((ty + (nb >> 1)) * PW + tx + (nb & 1)) * PIX_STRIDE + kgl * 8);
        acc[j][mi] = mfma16(af, bfr, acc[j][mi]);
      }
    }
  }
  EDGE_STAMP(4);
  __syncthreads();                 // every wave has read its patch fragments: the tiles below overwrite the patch
#pragma unroll
  for (int j = 0; j < NT; ++j)
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int r = 0; r < 4; ++r) sl[((wave * 2 + mi) * 16 + (lane >> 4) * 4 + r) * SLW + j * 16 + (lane & 15)] = acc[j][mi][r];
  __syncthreads();
  EDGE_STAMP(5);
  // Elementwise pass, one thread per OUTPUT PIXEL (2 pixels per thread: oy = tid / 64 + 4 i, ox = tid % 64), all C bands: the
  // target / x_hat accesses stay coalesced per plane (a wave = one 64-pixel row segment of a plane), and the gradient pixel
  // [g0 .. g(C-1), 0 ..] leaves as whole CP-band stores (8 bytes for CP = 4).  (Round 2 went element by element in NCHW order -- 6
  // elements per thread, each with its own 64-bit address arithmetic -- and staged the gradient tile through LDS with 2-byte scatter
  // writes, a clear and two more barriers: by the stamps this phase was 7.7-12 K of a workgroup's 23-38 K cycles, all of it VALU
  // issue at 8 workgroups per CU.)
  constexpr int CMAX = EdgeK<CP>::CMAX;
  float lsum = 0.f, gsum[CMAX];
  float bb[CMAX];
#pragma unroll
  for (int co = 0; co < CMAX; ++co) { gsum[co] = 0.f; bb[co] = co < C ? a.bias[co] : 0.f; }
  const size_t plane = (size_t)Hout * Wout;
  const int ox = tid & 63;
  // output windows: the tile's 2 * E_TH output rows of image n -- of the gradient tensor [n][oy][ox][CP], and (x_hat, per band) of a plane
  const size_t row0 = (size_t)(2 * iy0) * Wout;
  OutRsrc og;
  og.init(a.g4 ? a.g4 + ((size_t)n * plane + row0) * CP : (bf16_t*)nullptr, a.g4 ? (long)(2 * E_TH) * Wout * CP * 2 : 0);
  float xt[2][CMAX];                 // the target values of this thread, requested together (the stores below may not be reordered against loads)
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int co = 0; co < CMAX; ++co)
      xt[i][co] = (a.x && co < C) ? a.x[((size_t)n * C + co) * plane + (size_t)(2 * iy0 + (tid >> 6) + 4 * i) * Wout + 2 * ix0 + ox] : 0.f;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int oy = (tid >> 6) + 4 * i;
    const int pos = (oy >> 1) * E_TW + (ox >> 1), ph = (oy & 1) * 2 + (ox & 1);
    const float* sp = sl + pos * SLW + ph * C;
    uint32_t gb[CP];
#pragma unroll
    for (int co = 0; co < CP; ++co) gb[co] = 0u;
#pragma unroll
    for (int co = 0; co < CMAX; ++co) {
      if (co < C) {
        const float s = sp[co] + bb[co];
        const float xh = 1.0f / (1.0f + __expf(-s));
        if (a.x_hat) {
          OutRsrc oh;
          oh.init(a.x_hat + ((size_t)n * C + co) * plane + row0, (long)(2 * E_TH) * Wout * 4);
          oh.st4<EAE_WT_EDGE>((uint32_t)(oy * Wout + 2 * ix0 + ox) * 4u, xh);
        }
        if (a.x) {
          const float d = xh - xt[i][co];
          lsum = fmaf(d, d, lsum);
          if (a.g4) {
            gb[co] = f2bf(a.gscale * d * xh * (1.0f - xh));
            gsum[co] += bf2f(gb[co]);
          }
        }
      }
    }
    if (a.g4) {
      const uint32_t go = (uint32_t)((oy * Wout + 2 * ix0 + ox) * CP) * 2u;
      if constexpr (CP == 4) {
        og.st8<EAE_WT_EDGE>(go, (u32x2){gb[0] | (gb[1] << 16), gb[2] | (gb[3] << 16)});
      } else {
#pragma unroll
        for (int q = 0; q < CP / 8; ++q)
          og.st16<EAE_WT_EDGE>(go + 16u * q, make_uint4(gb[8 * q] | (gb[8 * q + 1] << 16), gb[8 * q + 2] | (gb[8 * q + 3] << 16),
                                                       gb[8 * q + 4] | (gb[8 * q + 5] << 16), gb[8 * q + 6] | (gb[8 * q + 7] << 16)));
      }
    }
  }
  EDGE_STAMP(6);
  if (a.loss_part) {
    float v[1 + CMAX];
    v[0] = lsum;
#pragma unroll
    for (int k = 0; k < CMAX; ++k) v[1 + k] = gsum[k];
#pragma unroll
    for (int k = 0; k < 1 + CMAX; ++k) {
      if (k <= C) {
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) v[k] += __shfl_xor(v[k], o);
        if (lane == 0) redl[wave][k] = v[k];
      }
    }
    __syncthreads();
    OutRsrc ol;      // window: this block's row of the loss partials
    ol.init(a.loss_part + (size_t)blockIdx.x * LPS, (long)LPS * 4);
    if (tid < LPS) ol.st4<EAE_WT_EDGE>((uint32_t)tid * 4u, tid <= C ? redl[0][tid] + redl[1][tid] + redl[2][tid] + redl[3][tid] : 0.f);
  }
  EDGE_STAMP(7);
}
template <int SRC, int CP>
__global__ __launch_bounds__(256) void deconv4_loss_kernel(Deconv4Args a) { deconv4_loss_body<SRC, CP>(a); }
template <int SRC, int CP>
__global__ __launch_bounds__(256) void deconv4_loss_kernel_g(GroupPack<Deconv4Args> p, int gz) { deconv4_loss_body<SRC, CP>(group_args<Deconv4Args>(gz)); }

// ---------------------------------------------------------------------------------------------------------------
// deconv4 forward + sigmoid against the SCENE (eae_scene_recon_error / eae_scene_reconstruct; eval mode)
//   image n of the launch is a window of the scene (SceneSrc, as conv1's scene source: first + n, or index[first + n]); the MSE target
//   is the scene pixel itself, scene_val(v, divisor[c]) -- the expression conv1's patch load uses, so the target is bit-identical to
//   what the encoder saw.  No [B,C,P,P] x_hat batch and no gradient are written:
//   part[tile][c] = sum over the tile's 8 x 64 pixels of (x_hat - x)^2 of band c (zero in the padding columns of the row), and with
//   STITCH x_hat (and optionally the band-mean squared residual of the pixel) goes to a stitched raster, for the pixels the window
//   OWNS only: with m = (P - S) / 2 window row i owns scene rows [i*S + m, i*S + m + S), extended to 0 for i = 0 and to Hg for
//   i = nH - 1; columns alike (scene.py owned_span).  Every pixel of the extent has exactly one owner: plain stores, no accumulation.
//   Summation order of a partial: each thread chains its 2 pixels (fmaf), 6 xor-shuffle levels over the wave, then the four waves in
//   ascending order; scene_err_finalize_kernel adds a window's tiles, then its bands, in ascending order.  No atomics anywhere.
// ---------------------------------------------------------------------------------------------------------------
__host__ __device__ constexpr int edge_bp_stride(int C) { return (C + 3) / 4 * 4; }      // floats of a partial row: C bands, whole float4s

// The MFMA part of deconv4_loss_body, line for line: stages the 5 x 33 input patch of this workgroup's tile (image n, input rows iy0..,
// columns ix0..), multiplies the four phases jointly and leaves the pre-sigmoid tile sl[128][16*NT + 1] (without the bias) in LDS,
// behind a barrier.  Returns sl.  (Kept beside deconv4_loss_body instead of shared with it: routing the training kernel through this
// helper changed its instruction schedule, and that kernel's code is tuned and measured as it stands.)
template <int SRC, int CP>
__device__ __forceinline__ float* deconv4_presigmoid_tile(const Deconv4Args& a, int& n, int& iy0, int& ix0) {
  constexpr int PH = E_TH + 1, PW = E_TW + 1, NPIX = PH * PW;       // 5 x 33 input pixels
  constexpr int NPA = (NPIX * 4 + 255) / 256;
  constexpr int NT = EdgeK<CP>::NT, SLW = 16 * NT + 1;              // pre-sigmoid tile [128][16*NT + 1] floats
  constexpr int PATCH_B = (int)sizeof(bf16_t) * NPIX * PIX_STRIDE, SL_B = (int)sizeof(float) * 128 * SLW;
  // the pre-sigmoid tile `sl` (8.7 KB for CP = 4) reuses the patch (13.2 KB) once every wave has read its fragments: 8 blocks per CU
  __shared__ __attribute__((aligned(16))) bf16_t patch[(PATCH_B > SL_B ? PATCH_B : SL_B) / 2];
  float* const sl = reinterpret_cast<float*>(patch);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tiles_x = a.Win / E_TW, tiles_y = a.Hin / E_TH;
  int t = blockIdx.x;
  const int txb = t % tiles_x; t /= tiles_x;
  const int tyb = t % tiles_y; t /= tiles_y;
  n = t;
  iy0 = tyb * E_TH; ix0 = txb * E_TW;
  const int kgs = tid & 3, kgl = lane >> 4;
  ChanCoef<SRC> cc;
  BnFoldRegs fr;
  const bool folded = SRC == SRC_BNRELU && a.fold.acc != nullptr;
  EDGE_STAMP(0);
  if (folded) bn_fold_load<32>(a.fold, fr);       // before the patch loads: results return in issue order
  RawPiece<SRC> raw[NPA];
  bool val[NPA];
#pragma unroll
  for (int i = 0; i < NPA; ++i) {
    int qq = tid + i * 256;
    int pix = qq >> 2;
    int pr = pix / PW, pc = pix % PW;
    int iy = iy0 + pr, ix = ix0 + pc;
    val[i] = (pix < NPIX) && (iy < a.Hin) && (ix < a.Win);
    size_t off = (((size_t)n * a.Hin + iy) * a.Win + ix) * 32 + kgs * 8;
    load_piece<SRC>(a.src, off, val[i], raw[i]);
  }
  {   // coefficient table of the 32-channel source layer (folded BatchNorm finalize) while the loads are in flight
    __shared__ float coef_tab[4 * 32];
    const float* coefp = a.src.coef;
    if (folded) {
      bn_fold_fwd_finish<32>(a.fold, fr, coef_tab, reinterpret_cast<long long*>(sl), blockIdx.x == 0);
      coefp = coef_tab;
    }
    cc.load(coefp, 32, kgs * 8);
  }
  EDGE_STAMP(1);
#pragma unroll
  for (int i = 0; i < NPA; ++i) {
    int qq = tid + i * 256;
    if (qq < NPIX * 4)
      *reinterpret_cast<uint4*>(patch + (qq >> 2) * PIX_STRIDE + kgs * 8) = transform_piece<SRC>(raw[i], val[i], cc);
  }
  EDGE_STAMP(2);
  __syncthreads();
  EDGE_STAMP(3);
  f32x4 acc[NT][2];
#pragma unroll
  for (int j = 0; j < NT; ++j) acc[j][0] = acc[j][1] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int nb = 0; nb < 4; ++nb) {
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      bf16x8 bfr = *reinterpret_cast<const bf16x8*>(a.wjoint + (j * 16 + (lane & 15)) * 128 + nb * 32 + kgl * 8);
#pragma unroll
      for (int mi = 0; mi < 2; ++mi) {
        int pos = (wave * 2 + mi) * 16 + (lane & 15);
        int ty = pos / E_TW, tx = pos % E_TW;
        bf16x8 af = *reinterpret_cast<const bf16x8*>(patch + ((ty + (nb >> 1)) * PW + tx + (nb & 1)) * PIX_STRIDE + kgl * 8);
        acc[j][mi] = mfma16(af, bfr, acc[j][mi]);
      }
    }
  }
  EDGE_STAMP(4);
  __syncthreads();                 // every wave has read its patch fragments: the tiles below overwrite the patch
#pragma unroll
  for (int j = 0; j < NT; ++j)
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int r = 0; r < 4; ++r) sl[((wave * 2 + mi) * 16 + (lane >> 4) * 4 + r) * SLW + j * 16 + (lane & 15)] = acc[j][mi][r];
  __syncthreads();
  EDGE_STAMP(5);
  return sl;
}

template <int SRC3, int CP, bool IDX, bool STITCH, bool BORDER = false>
__device__ __forceinline__ void deconv4_scene_body(const Deconv4Args& a, const SceneSrcCore& sc, const Deconv4SceneArgs& r,
                                                   const SceneBorder& sb) {
  using T = typename SceneElem<SRC3>::T;
  constexpr int NT = EdgeK<CP>::NT, SLW = 16 * NT + 1, CMAX = EdgeK<CP>::CMAX;
  __shared__ float redb[4][CMAX];
  const int C = edge_bands<CP>(a.C), BPS = edge_bp_stride(C);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int n, iy0, ix0;
  const float* const sl = deconv4_presigmoid_tile<SRC_BNRELU, CP>(a, n, iy0, ix0);
  const int P = a.Win * 2;                          // square windows (scene_ctx_checks)
  long long w = sc.first + n;
  if constexpr (IDX) w = sc.index[w];               // one uniform load per workgroup
  bool inside = true;
  if constexpr (IDX) inside = w >= 0 && w < sc.nwin;   // an id outside the grid: target zero, nothing written for it
  const long long wi = inside ? w / sc.nW : 0, wj = inside ? w - wi * sc.nW : 0;
  const long long org = wi * sc.S * (long long)sc.Ws + wj * sc.S;
  const T* const x = static_cast<const T*>(sc.data);
  float bsum[CMAX], bb[CMAX], dv[CMAX];
#pragma unroll
  for (int co = 0; co < CMAX; ++co) {
    bsum[co] = 0.f;
    bb[co] = co < C ? a.bias[co] : 0.f;
    dv[co] = co < C ? sc.div[co] : 1.f;
  }
  const int ox = tid & 63, lx = 2 * ix0 + ox;       // window-local column of this thread's pixels
  float xt[2][CMAX];               // the target values of this thread, requested together ahead of the stores (as deconv4_loss_body)
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    if constexpr (BORDER) {          // the resolver conv1's patch load used: target and input stay bit-identical
      const int vy = (int)wi * sc.S + 2 * iy0 + (tid >> 6) + 4 * i, vx = (int)wj * sc.S + lx;
#pragma unroll
      for (int co = 0; co < CMAX; ++co)
        xt[i][co] = (inside && co < C) ? scene_border_val<T>(x + co * sc.plane, sb, vy, vx, dv[co]) : 0.f;
    } else {
      const T* p = x + org + (long long)(2 * iy0 + (tid >> 6) + 4 * i) * sc.Ws + lx;
#pragma unroll
      for (int co = 0; co < CMAX; ++co) xt[i][co] = (inside && co < C) ? scene_val(p[co * sc.plane], dv[co]) : 0.f;
    }
  }
  // owned span of the window, window-local (STITCH)
  int oy_lo = 0, oy_hi = 0, ox_lo = 0, ox_hi = 0;
  if constexpr (STITCH) {
    oy_lo = wi == 0 ? 0 : r.m; oy_hi = wi == r.nH - 1 ? P : r.m + sc.S;
    ox_lo = wj == 0 ? 0 : r.m; ox_hi = wj == sc.nW - 1 ? P : r.m + sc.S;
  }
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int oy = (tid >> 6) + 4 * i, ly = 2 * iy0 + oy;
    const int pos = (oy >> 1) * E_TW + (ox >> 1), ph = (oy & 1) * 2 + (ox & 1);
    const float* sp = sl + pos * SLW + ph * C;
    bool own = false;
    long long gp = 0;
    if constexpr (STITCH) {
      own = inside && ly >= oy_lo && ly < oy_hi && lx >= ox_lo && lx < ox_hi;
      if constexpr (BORDER) {        // spans in virtual coordinates; a store lands only where the virtual pixel is a real one
        const long long ry = wi * sc.S + ly - sb.pt, rx = wj * sc.S + lx - sb.pl;
        own = own && ry >= 0 && ry < sb.Hs && rx >= 0 && rx < sb.Ws;
        gp = ry * r.Wg + rx;
      } else {
        gp = (wi * sc.S + ly) * (long long)r.Wg + wj * sc.S + lx;
      }
    }
    float rs = 0.f;
#pragma unroll
    for (int co = 0; co < CMAX; ++co) {
      if (co < C) {
        const float s = sp[co] + bb[co];
        const float xh = 1.0f / (1.0f + __expf(-s));
        const float d = xh - xt[i][co];
        bsum[co] = fmaf(d, d, bsum[co]);
        if constexpr (STITCH) {
          rs = fmaf(d, d, rs);
          if (own) r.recon[co * r.gplane + gp] = xh;
        }
      }
    }
    if constexpr (STITCH)
      if (own && r.residual) r.residual[gp] = rs / (float)C;
  }
#pragma unroll
  for (int k = 0; k < CMAX; ++k) {
    if (k < C) {
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) bsum[k] += __shfl_xor(bsum[k], o);
      if (lane == 0) redb[wave][k] = bsum[k];
    }
  }
  __syncthreads();
  if (tid < BPS) r.part[(size_t)blockIdx.x * BPS + tid] = tid < C ? ((redb[0][tid] + redb[1][tid]) + redb[2][tid]) + redb[3][tid] : 0.f;
}
template <int SRC3, int CP, bool IDX, bool STITCH, bool BORDER = false>
__global__ __launch_bounds__(256) void deconv4_scene_kernel(Deconv4Args a, SceneSrcCore s, Deconv4SceneArgs r, SceneBorder sb) {
  deconv4_scene_body<SRC3, CP, IDX, STITCH, BORDER>(a, s, r, sb);
}
