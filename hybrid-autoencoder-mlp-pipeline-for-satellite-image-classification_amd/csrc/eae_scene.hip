// Scene classification helpers (include/eae.h, "scene classification"): the window gather (the public way to get patches, and the
// reference the fused conv1 scene source is tested against), the cell blends of window probabilities, and the nodata / mask path:
// per-window invalid-pixel counts and the compaction of the valid window ids; and training from a scene (include/eae.h, "training from
// a scene"): window batches (the kernel is eae_stage.hip's) and a label for every window from a label raster; and the confusion counts
// of a class map against a label raster (include/eae.h, "accuracy assessment").  None uses matrix instructions, so all are built with
// packed FP32 disabled (EAE_NO_PK, tests/test_isa_guard.py).
#include "eae_internal.h"
#include "eae_ctx.h"
#include "eae_common.hip.h"
#include "eae_edge.hip.h"
#include "eae_stage.h"

namespace {

// out[b][c][y][x] = scene[c][oy + y][ox + x] / divisor[c] for window first + b; one thread per output pixel, all bands
// BORDER: (oy + y, ox + x) is a virtual pixel, resolved by scene_border_val (bs: the border fields of the scene; read by BORDER only)
template <typename T, bool BORDER>
__global__ EAE_NO_PK __launch_bounds__(256) void scene_windows_kernel(const T* __restrict__ src, const float* __restrict__ divisor, int C,
                                                                  long long plane, int Ws, int P, int S, int nW, long long first, int B,
                                                                  float* __restrict__ out, SceneBorder bs) {
  const long long pp = (long long)P * P;
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= pp * B) return;
  const long long b = p / pp, r = p - b * pp;
  const int y = (int)(r / P), x = (int)(r - (long long)y * P);
  const long long w = first + b, wi = w / nW, wj = w - wi * nW;
  if constexpr (BORDER) {
    for (int c = 0; c < C; ++c)
      out[(b * C + c) * pp + r] = scene_border_val<T>(src + c * plane, bs, (int)wi * S + y, (int)wj * S + x, divisor[c]);
    return;
  }
  const T* q = src + (wi * S + y) * (long long)Ws + wj * S + x;
  for (int c = 0; c < C; ++c) out[(b * C + c) * pp + r] = scene_val(q[c * plane], divisor[c]);
}

// cell (ci, cj) of the [nH + k - 1][nW + k - 1] map: mean over windows i in [ci - k + 1, ci] x j in [cj - k + 1, cj] inside the grid.
// VALID: over the valid ones of them only (labels >= 0): the same (i, then j) summation order, divided by the float count of valid
// covering windows; a cell without one gets probabilities 0 and label -1.  (labels is the last argument, read by VALID only: the plain
// form keeps the argument block it had as a kernel of its own.)
// Worked: a 2 x 2 grid, k = 2, two classes, probs[0] = {{.5, .25}, {.75, 1}}, probs[1] = 1 - probs[0]; 3 x 3 cells.  Cell (0, 0) has
// window (0, 0) alone: .5 / .5, a tie, label 0 (the lowest class).  Cell (0, 1): (.5 + .25) / 2 = .375 against .625, label 1.  Cell
// (1, 1): (.5 + .25 + .75 + 1) / 4 = .625, label 0.  VALID with window (0, 1) invalid: cell (0, 2), covered by that window alone, is
// 0 / 0 with label -1; cell (0, 1) is window (0, 0)'s .5 / .5, label 0; cell (1, 1) is (.5 + .75 + 1) / 3 = .75 against .25, label 0.
template <bool VALID>
__global__ EAE_NO_PK __launch_bounds__(256) void scene_blend_kernel(const float* __restrict__ probs, int K, int nH, int nW, int k,
                                                                float* __restrict__ cell, long long* __restrict__ cell_labels,
                                                                const long long* __restrict__ labels) {
  const int cH = nH + k - 1, cW = nW + k - 1;
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= (long long)cH * cW) return;
  const int ci = (int)(p / cW), cj = (int)(p - (long long)ci * cW);
  const int i0 = ci - k + 1 > 0 ? ci - k + 1 : 0, i1 = ci < nH - 1 ? ci : nH - 1;
  const int j0 = cj - k + 1 > 0 ? cj - k + 1 : 0, j1 = cj < nW - 1 ? cj : nW - 1;
  const long long wplane = (long long)nH * nW, cplane = (long long)cH * cW;
  int nv = (i1 - i0 + 1) * (j1 - j0 + 1);
  if constexpr (VALID) {
    nv = 0;
    for (int i = i0; i <= i1; ++i)
      for (int j = j0; j <= j1; ++j) nv += labels[(long long)i * nW + j] >= 0;
    if (nv == 0) {
      for (int c = 0; c < K; ++c) cell[c * cplane + p] = 0.f;
      cell_labels[p] = -1;
      return;
    }
  }
  const float cnt = (float)nv;
  float mx = 0.f;
  int am = 0;
  for (int c = 0; c < K; ++c) {
    const float* q = probs + c * wplane;
    float s = 0.f;
    for (int i = i0; i <= i1; ++i)
      for (int j = j0; j <= j1; ++j) {
        if constexpr (VALID) {
          if (labels[(long long)i * nW + j] < 0) continue;
        }
        s += q[(long long)i * nW + j];
      }
    const float v = s / cnt;
    cell[c * cplane + p] = v;
    if (c == 0 || v > mx) { mx = v; am = c; }
  }
  cell_labels[p] = am;
}

// ---------------------------------------------------------------------------------------------------------------- invalid-pixel counts
// Separable count of the invalid pixels of every window, reading each scene element (and mask byte) inside the grid's extent once:
//   pass 1 (scene_invalid_rows_kernel): one workgroup per (pixel row y, chunk of window columns).  Each thread tests groups of V pixels
//     (one 16-byte load per band where aligned, else element loads) across the bands in registers and writes one flag byte per pixel
//     to LDS; a block prefix sum over the chunk's pixels gives every window column its horizontal run sum in O(1) (also for S < P):
//     rows[y][j] = number of invalid pixels in scene row y, columns j*S .. j*S + P - 1.
//   pass 2 (scene_invalid_windows_kernel): counts[i][j] = sum of rows[i*S + r][j], r < P (one thread per window, coalesced along j).
// BORDER (the grid over the virtual padded scene; the mapping virtual -> source pixel is separable, so the split stays): y and the
//   columns of pass 1 are virtual coordinates, rows[] holds the virtual rows and pass 2 is unchanged.  The workgroup of virtual row y
//   reads the row's source row; a group of V whose virtual columns are all real takes the vector path, any other group loads resolved
//   elements, a constant pixel being the fill value itself (so it is invalid exactly when the fill matches nodata; its mask byte is 0).
//   Reads: a real element is read once for every virtual pixel inside the extent that resolves to it.  Per axis that is 1 for constant,
//   at most 3 for reflect (itself, a leading and a trailing mirror image) and, for edge, 1 except the first and the last row / column,
//   which are read 1 + their pad (<= P) times: at most 9 reads of an element under reflect, P * P of a corner pixel under edge, and
//   over the scene at most (H + pad_top + pad_bottom) x (W + pad_left + pad_right) element reads per band.
constexpr int INV_NT = 256;               // threads of pass 1
constexpr int INV_SPAN = INV_NT * 16;     // pixels per pass-1 workgroup (16 per thread), including the alignment shift

__device__ __forceinline__ int wave_incl_scan(int v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int u = __shfl_up(v, d, 64);
    if (lane >= d) v += u;
  }
  return v;
}
// exclusive prefix of v over the NT threads of the block (NT a multiple of 64); *total = the block's sum.  sh: NT / 64 ints of LDS.
template <int NT>
__device__ __forceinline__ int block_excl_scan(int v, int* sh, int* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int incl = wave_incl_scan(v);
  if (lane == 63) sh[wave] = incl;
  __syncthreads();
  int base = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < NT / 64; ++w) {
    const int x = sh[w];
    base += w < wave ? x : 0;
    tot += x;
  }
  __syncthreads();                        // sh is reused by the next call
  *total = tot;
  return base + incl - v;
}

template <typename T> __device__ __forceinline__ bool inv_match(T v, int mode, T ref, float fref) {
  if constexpr (sizeof(T) == 4) return mode == EAE_NODATA_NAN ? v != v : v == fref;
  else return v == ref;
}

template <typename T, bool BORDER>
__global__ EAE_NO_PK __launch_bounds__(INV_NT) void scene_invalid_rows_kernel(const T* __restrict__ src, long long plane, int C, int Ws,
                                                                           int P, int S, int nW, int J, int nchunk, int mode, float nodata,
                                                                           int rule_any, const unsigned char* __restrict__ mask,
                                                                           int* __restrict__ rows, SceneBorder bs) {
  constexpr int V = 16 / (int)sizeof(T), G = (int)sizeof(T);   // pixels per 16-byte group, groups per thread (G * V = 16)
  __shared__ unsigned char fl[INV_SPAN];
  __shared__ int pre[INV_SPAN + 1];
  __shared__ int sh[INV_NT / 64];
  const int tid = threadIdx.x;
  const long long y = blockIdx.x / nchunk;
  const int chunk = (int)(blockIdx.x - y * nchunk);
  const int j0 = chunk * J, jn = nW - j0 < J ? nW - j0 : J;
  const long long x0 = (long long)j0 * S, x1 = (long long)(j0 + jn - 1) * S + P;     // pixels [x0, x1) of this workgroup
  // BORDER: y, x0, x1, gx, lo, hi are virtual coordinates; virtual column v of this row is element rowoff + v of a band when real
  const int pl = BORDER ? bs.pl : 0;
  const int sy = BORDER ? scene_resolve((int)y, bs.pt, bs.Hs, bs.mode) : 0;     // source row; -1: a row of constant pixels
  const long long rowoff = (BORDER ? (long long)(sy < 0 ? 0 : sy) : y) * Ws - pl;
  // groups start at a 16-byte boundary of band 0: xa = x0 - m
  const int m = (int)(((reinterpret_cast<uintptr_t>(src) + (uintptr_t)((rowoff + x0) * (long long)sizeof(T))) & 15) / sizeof(T));
  const long long xa = x0 - m;
  const T ref = (T)(mode == EAE_NODATA_VALUE && sizeof(T) < 4 ? nodata : 0.f);
#pragma unroll
  for (int g = 0; g < G; ++g) {
    const int q = g * INV_NT + tid;
    const long long gx = xa + (long long)q * V;
    const long long lo = gx > x0 ? gx : x0, hi = gx + V < x1 ? gx + V : x1;
    bool inv[V];
    const bool any_rule = rule_any != 0;
#pragma unroll
    for (int v = 0; v < V; ++v) inv[v] = false;
    int sx[V];                          // BORDER: source columns of the group's virtual ones, -1 = a constant pixel
    if constexpr (BORDER) {
#pragma unroll
      for (int v = 0; v < V; ++v) sx[v] = sy < 0 ? -1 : scene_resolve((int)gx + v, pl, Ws, bs.mode);
    }
    if (lo < hi) {
      const bool full = lo == gx && hi == gx + V && (!BORDER || (sy >= 0 && gx >= pl && gx + V <= pl + Ws));
      if (mode != EAE_NODATA_NONE) {
#pragma unroll
        for (int v = 0; v < V; ++v) inv[v] = !any_rule;
#pragma unroll 4
        for (int c = 0; c < C; ++c) {
          const T* p = src + c * plane + rowoff + gx;
          T e[V];
          if (full && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
            const uint4 u = *reinterpret_cast<const uint4*>(p);
            __builtin_memcpy(e, &u, 16);
          } else if constexpr (BORDER) {
            const T* pr = src + c * plane + rowoff + pl;      // the real row
#pragma unroll
            for (int v = 0; v < V; ++v) e[v] = (gx + v >= lo && gx + v < hi) ? (sx[v] < 0 ? (T)bs.fill : pr[sx[v]]) : (T)0;
          } else {
#pragma unroll
            for (int v = 0; v < V; ++v) e[v] = (gx + v >= lo && gx + v < hi) ? p[v] : (T)0;
          }
#pragma unroll
          for (int v = 0; v < V; ++v) {
            const bool mt = inv_match<T>(e[v], mode, ref, nodata);
            inv[v] = any_rule ? (inv[v] || mt) : (inv[v] && mt);
          }
        }
      }
      if (mask) {
        const unsigned char* p = mask + rowoff + gx;
        unsigned char e[V];
        if (full && (reinterpret_cast<uintptr_t>(p) & (V - 1)) == 0) {
          if constexpr (V == 16) { const uint4 u = *reinterpret_cast<const uint4*>(p); __builtin_memcpy(e, &u, 16); }
          else if constexpr (V == 8) { const uint2 u = *reinterpret_cast<const uint2*>(p); __builtin_memcpy(e, &u, 8); }
          else { const unsigned u = *reinterpret_cast<const unsigned*>(p); __builtin_memcpy(e, &u, 4); }
        } else if constexpr (BORDER) {
          const unsigned char* pr = mask + rowoff + pl;
#pragma unroll
          for (int v = 0; v < V; ++v) e[v] = (gx + v >= lo && gx + v < hi && sx[v] >= 0) ? pr[sx[v]] : (unsigned char)0;
        } else {
#pragma unroll
          for (int v = 0; v < V; ++v) e[v] = (gx + v >= lo && gx + v < hi) ? p[v] : (unsigned char)0;
        }
#pragma unroll
        for (int v = 0; v < V; ++v) inv[v] = inv[v] || e[v] != 0;
      }
#pragma unroll
      for (int v = 0; v < V; ++v) inv[v] = inv[v] && gx + v >= lo && gx + v < hi;
    }
#pragma unroll
    for (int v = 0; v < V; ++v) fl[q * V + v] = inv[v] ? 1 : 0;
  }
  __syncthreads();
  // pre[k] = invalid pixels among [xa, xa + k): thread tid owns pixels tid*16 .. tid*16 + 15
  int loc = 0;
#pragma unroll
  for (int v = 0; v < 16; ++v) loc += fl[tid * 16 + v];
  int tot = 0;
  int run = block_excl_scan<INV_NT>(loc, sh, &tot);
  if (tid == 0) pre[0] = 0;
#pragma unroll
  for (int v = 0; v < 16; ++v) {
    run += fl[tid * 16 + v];
    pre[tid * 16 + v + 1] = run;
  }
  __syncthreads();
  for (int jj = tid; jj < jn; jj += INV_NT) {
    const int s0 = m + jj * S;
    rows[y * nW + j0 + jj] = pre[s0 + P] - pre[s0];
  }
}

__global__ EAE_NO_PK __launch_bounds__(256) void scene_invalid_windows_kernel(const int* __restrict__ rows, int nH, int nW, int P, int S,
                                                                          int* __restrict__ counts) {
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= (long long)nH * nW) return;
  const long long i = p / nW, j = p - i * nW;
  const int* r = rows + i * S * nW + j;
  int s = 0;
  for (int y = 0; y < P; ++y) s += r[(long long)y * nW];
  counts[p] = s;
}

// Stable compaction in one workgroup: ids of the windows with counts <= t, ascending, and their number.  Each pass takes 8 consecutive
// windows per thread (8192 per pass); the output offsets come from a block prefix sum, so the order never depends on scheduling.
constexpr int SEL_NT = 1024, SEL_PER = 8;
__global__ EAE_NO_PK __launch_bounds__(SEL_NT) void scene_select_kernel(const int* __restrict__ counts, long long n, int t,
                                                                    long long* __restrict__ ids, long long* __restrict__ count_out) {
  __shared__ int sh[SEL_NT / 64];
  const int tid = threadIdx.x;
  long long base = 0;
  for (long long c0 = 0; c0 < n; c0 += (long long)SEL_NT * SEL_PER) {
    const long long k0 = c0 + (long long)tid * SEL_PER;
    unsigned ok = 0;
    int loc = 0;
#pragma unroll
    for (int v = 0; v < SEL_PER; ++v)
      if (k0 + v < n && counts[k0 + v] <= t) { ok |= 1u << v; ++loc; }
    int tot = 0;
    long long o = base + block_excl_scan<SEL_NT>(loc, sh, &tot);
#pragma unroll
    for (int v = 0; v < SEL_PER; ++v)
      if (ok & (1u << v)) ids[o++] = k0 + v;
    base += tot;
  }
  if (tid == 0) *count_out = base;
}


// ---------------------------------------------------------------------------------------------------------------- training from a scene
// One workgroup per window: every wave counts the labelled pixels (values in [0, K)) it reads into its own K-bin LDS histogram, a
// thread adding a run of equal classes with one atomic (land-cover windows are mostly one class: a run is usually the thread's whole
// share); wave 0 then sums the waves' bins in wave order, lane = class, and reduces (count, class) to the largest count, the lowest
// class on a tie.  Integer counts: exact and identical from run to run.
constexpr int LBL_NT = 256;
template <typename T>
__global__ EAE_NO_PK __launch_bounds__(LBL_NT) void scene_window_labels_kernel(const T* __restrict__ raster, int W, int P, int S, int nW,
                                                                            int K, long long* __restrict__ label,
                                                                            int* __restrict__ count, int* __restrict__ labelled) {
  __shared__ int hist[LBL_NT / 64][64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long n = blockIdx.x, wi = n / nW, wj = n - wi * nW;
  hist[wave][lane] = 0;
  __syncthreads();
  const T* q = raster + wi * S * (long long)W + wj * S;
  int cur = -1, run = 0;
  for (int i = tid; i < P * P; i += LBL_NT) {
    const int y = i / P, x = i - y * P;
    const long long v = (long long)q[(long long)y * W + x];
    const int k = v >= 0 && v < K ? (int)v : -1;
    if (k != cur) {
      if (cur >= 0) atomicAdd(&hist[wave][cur], run);
      cur = k;
      run = 0;
    }
    ++run;
  }
  if (cur >= 0) atomicAdd(&hist[wave][cur], run);
  __syncthreads();
  if (wave != 0) return;
  int best = 0;
#pragma unroll
  for (int w = 0; w < LBL_NT / 64; ++w) best += hist[w][lane];       // lanes K .. 63 hold 0
  int tot = best, cls = lane;
#pragma unroll
  for (int d = 32; d; d >>= 1) {
    tot += __shfl_xor(tot, d, 64);
    const int ob = __shfl_xor(best, d, 64), oc = __shfl_xor(cls, d, 64);
    if (ob > best || (ob == best && oc < cls)) { best = ob; cls = oc; }
  }
  if (lane == 0) {
    label[n] = tot ? cls : -1;
    if (count) count[n] = tot ? best : 0;
    if (labelled) labelled[n] = tot;
  }
}

// ---------------------------------------------------------------------------------------------------------------- accuracy assessment
// Confusion counts of a cell map against a label raster (include/eae.h, "accuracy assessment").  The unit of work is a RUN: 16
// consecutive pixels of one row, starting at a 16-element boundary of the raster's memory (run g of row y covers columns
// [16 g - m, 16 g - m + 16), m = the element misalignment of the row's first pixel), so a whole run is one 16-byte load of a uint8
// raster (four of an int32 one) and one of the mask, and the clipped first and last runs of a row load element by element.  Rows
// have G = ceil((W + 15) / 16) run slots (the last may be empty for a small m); a tile is CONF_NT consecutive slots of the flattened
// [H][G] list, so narrow rasters fill a workgroup with several rows, and the workgroups take tiles grid-strided.  Divisions: one 64-bit
// one per tile (uniform), then per run one 32-bit one for the row, one for the cell row and one for the first cell column; the cell
// column is stepped from there and pred is re-read only when the cell changes.  (r, c) pairs go to a (K+1)^2 int table in LDS, a run
// of equal pairs as one atomic (the label kernel's scheme); the non-zero bins are flushed with 64-bit integer atomics.  Integers
// only: exact, and identical from run to run.  The launch keeps a workgroup's share below 2^31 pixels (the table is 32-bit).
constexpr int CONF_NT = 256, CONF_RUN = 16;
// the table column of cell x of a map row: its class in [0, K), else K (rowin: the row lies inside the map; prow is read only then)
__device__ __forceinline__ int conf_cell_class(const long long* __restrict__ prow, bool rowin, unsigned cW, unsigned x, int K) {
  if (!rowin || x >= cW) return K;
  const long long v = prow[x];
  return v >= 0 && v < K ? (int)v : K;
}
template <typename T>
__global__ EAE_NO_PK __launch_bounds__(CONF_NT) void scene_confusion_kernel(const T* __restrict__ truth, int H, int W,
                                                                         const long long* __restrict__ pred, int cH, int cW,
                                                                         unsigned cell, unsigned oy, unsigned ox,
                                                                         const unsigned char* __restrict__ mask, int K, unsigned G,
                                                                         long long ntiles, unsigned long long* __restrict__ counts) {
  extern __shared__ int conf_tab[];                         // [(K+1)][(K+1)]
  constexpr int V = CONF_RUN;
  const int tid = threadIdx.x, K1 = K + 1, nbin = K1 * K1;
  for (int i = tid; i < nbin; i += CONF_NT) conf_tab[i] = 0;
  __syncthreads();
  const unsigned long long base_el = reinterpret_cast<uintptr_t>(truth) / sizeof(T);      // element address of pixel (0, 0)
  for (long long t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const long long u0 = t * CONF_NT, y0 = u0 / G;
    const unsigned q = (unsigned)(u0 - y0 * G) + (unsigned)tid, dy = q / G, g = q - dy * G;      // q < G + CONF_NT
    const long long y = y0 + dy;
    if (y >= H) continue;                                   // the last tile's tail (no barrier inside the loop)
    const long long row = y * W;
    const int m = (int)((base_el + (unsigned long long)row) & (V - 1));
    const long long gx = (long long)g * V - m;              // first column of the run; < 0 for a clipped first run
    const int lo = gx > 0 ? (int)gx : 0, hi = gx + V < W ? (int)(gx + V) : W;
    if (lo >= hi) continue;                                 // the empty last slot of a row
    const bool full = hi - lo == V;
    const T* p = truth + row + gx;                          // dereferenced at [lo - gx, hi - gx) only
    int tv[V], mk[V];                                       // truth values and mask bytes of the run (statically indexed: registers)
    if (full) {                                             // 16 elements from a 16-element boundary
      const uint4* p4 = reinterpret_cast<const uint4*>(p);
      if constexpr (sizeof(T) == 1) {
        const uint4 w = p4[0];
        const unsigned ww[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
        for (int v = 0; v < V; ++v) tv[v] = (int)((ww[v >> 2] >> ((v & 3) * 8)) & 255u);
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const uint4 w = p4[i];
          tv[4 * i] = (int)w.x; tv[4 * i + 1] = (int)w.y; tv[4 * i + 2] = (int)w.z; tv[4 * i + 3] = (int)w.w;
        }
      }
    } else {
#pragma unroll
      for (int v = 0; v < V; ++v) tv[v] = (gx + v >= lo && gx + v < hi) ? (int)p[v] : 0;
    }
#pragma unroll
    for (int v = 0; v < V; ++v) mk[v] = 0;
    if (mask) {
      const unsigned char* pm = mask + row + gx;
      if (full && (reinterpret_cast<uintptr_t>(pm) & 15) == 0) {
        const uint4 w = *reinterpret_cast<const uint4*>(pm);
        const unsigned ww[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
        for (int v = 0; v < V; ++v) mk[v] = (int)((ww[v >> 2] >> ((v & 3) * 8)) & 255u);
      } else {
#pragma unroll
        for (int v = 0; v < V; ++v) mk[v] = (gx + v >= lo && gx + v < hi) ? (int)pm[v] : 0;
      }
    }
    // the cell of pixel (y, lo), stepped along the row; pc = its column in the table (K: not classified)
    const unsigned cy = ((unsigned)y + oy) / cell;
    unsigned cx = ((unsigned)lo + ox) / cell, rem = ((unsigned)lo + ox) - cx * cell;
    const bool rowin = cy < (unsigned)cH;
    const long long* prow = pred + (long long)cy * cW;      // read only when rowin
    int pc = conf_cell_class(prow, rowin, (unsigned)cW, cx, K);
    int cur = -1, run = 0;
#pragma unroll
    for (int v = 0; v < V; ++v) {
      const bool in = gx + v >= lo && gx + v < hi;
      int bin = -1;
      if (in) {
        const int r = tv[v] >= 0 && tv[v] < K ? tv[v] : K;
        if (mk[v] == 0) bin = r * K1 + pc;
        if (++rem == cell) { rem = 0; ++cx; pc = conf_cell_class(prow, rowin, (unsigned)cW, cx, K); }
      }
      if (bin != cur) {
        if (cur >= 0) atomicAdd(&conf_tab[cur], run);
        cur = bin;
        run = 0;
      }
      ++run;
    }
    if (cur >= 0) atomicAdd(&conf_tab[cur], run);
  }
  __syncthreads();
  for (int i = tid; i < nbin; i += CONF_NT) {
    const int n = conf_tab[i];
    if (n) atomicAdd(&counts[i], (unsigned long long)n);
  }
}

}  // namespace

long long eae_scene_extent(long long n, int patch, int stride) { return (n - 1) * stride + patch; }

// model: the windows feed the model, whose image size is a multiple of 64; the model-free calls (eae_scene_windows, training from a
// scene) take any patch size
static int scene_check(const eae_scene* s, long long* nH, long long* nW, bool model) {
  if (!s) return eae_set_error(EAE_ERR_ARG, "scene: NULL scene");
  if (!s->data) return eae_set_error(EAE_ERR_ARG, "scene: NULL data");
  if (!s->divisor) return eae_set_error(EAE_ERR_ARG, "scene: NULL divisor");
  if (s->dtype != EAE_SCENE_U8 && s->dtype != EAE_SCENE_U16 && s->dtype != EAE_SCENE_F32)
    return eae_set_error(EAE_ERR_ARG, "scene: dtype must be EAE_SCENE_U8, EAE_SCENE_U16 or EAE_SCENE_F32");
  if (s->C < 1 || s->C > 16) return eae_set_error(EAE_ERR_ARG, "scene: in_channels must be in 1..16");
  if (s->patch <= 0 || (model && s->patch % 64))
    return eae_set_error(EAE_ERR_ARG, model ? "scene: the patch size must be a positive multiple of 64" : "scene: the patch size must be positive");
  if (s->border < EAE_BORDER_NONE || s->border > EAE_BORDER_REFLECT) return eae_set_error(EAE_ERR_ARG, "scene: unknown border mode");
  const int pads[4] = {s->pad_top, s->pad_bottom, s->pad_left, s->pad_right};
  for (int p : pads) {
    if (s->border == EAE_BORDER_NONE && p != 0) return eae_set_error(EAE_ERR_ARG, "scene: pads need a border mode");
    if (p < 0 || p >= s->patch) return eae_set_error(EAE_ERR_ARG, "scene: every pad must be in 0..patch - 1");
  }
  if (s->border != EAE_BORDER_NONE && (s->H < 1 || s->W < 1)) return eae_set_error(EAE_ERR_ARG, "scene: empty scene");
  if (s->border == EAE_BORDER_REFLECT &&
      (s->pad_top > s->H - 1 || s->pad_bottom > s->H - 1 || s->pad_left > s->W - 1 || s->pad_right > s->W - 1))
    return eae_set_error(EAE_ERR_ARG, "scene: a reflect pad must be smaller than the scene (one reflection)");
  if (s->border == EAE_BORDER_CONSTANT && s->dtype != EAE_SCENE_F32) {
    const float hi = s->dtype == EAE_SCENE_U8 ? 255.f : 65535.f;
    if (!(s->fill >= 0.f && s->fill <= hi) || s->fill != (float)(int)s->fill)
      return eae_set_error(EAE_ERR_ARG, "scene: fill must be an integer in the scene dtype's range");
  }
  // the grid lies over the virtual scene (border = NONE: the scene itself, every pad being 0)
  const long long Hv = (long long)s->H + s->pad_top + s->pad_bottom, Wv = (long long)s->W + s->pad_left + s->pad_right;
  if (Hv < s->patch || Wv < s->patch) return eae_set_error(EAE_ERR_ARG, "scene: smaller than one window");
  if (s->stride < 1 || s->stride > s->patch) return eae_set_error(EAE_ERR_ARG, "scene: stride must be in 1..patch");
  *nH = (Hv - s->patch) / s->stride + 1;
  *nW = (Wv - s->patch) / s->stride + 1;
  return 0;
}
int eae_scene_check(const eae_scene* s, long long* nH, long long* nW) { return scene_check(s, nH, nW, true); }

int eae_scene_src3_kind(const eae_scene* s) {
  return s->dtype == EAE_SCENE_U8 ? SRC3_SCENE_U8 : s->dtype == EAE_SCENE_U16 ? SRC3_SCENE_U16 : SRC3_SCENE_F32;
}

void eae_scene_fill_src(const eae_scene* s, long long nW, long long first, SceneSrc* out) {
  out->data = s->data; out->div = s->divisor; out->first = first; out->plane = (long long)s->H * s->W;
  out->Ws = s->W; out->S = s->stride; out->nW = (int)nW;
  out->b.mode = s->border; out->b.pt = s->pad_top; out->b.pl = s->pad_left; out->b.Hs = s->H; out->b.Ws = s->W; out->b.fill = s->fill;
}

// the one u8 / u16 / f32 x borderless / border dispatch: f(tag, border) with tag a null pointer of the scene's element type and
// border a std::bool_constant
template <typename F> void scene_dtype_dispatch(const eae_scene* s, F f) {
  auto g = [&](auto border) {
    if (s->dtype == EAE_SCENE_U8) f((const uint8_t*)nullptr, border);
    else if (s->dtype == EAE_SCENE_U16) f((const uint16_t*)nullptr, border);
    else f((const float*)nullptr, border);
  };
  if (s->border) g(std::true_type()); else g(std::false_type());
}

extern "C" int eae_scene_windows(void* stream, const eae_scene* s, long long first, int B, float* out) {
  long long nH = 0, nW = 0;
  if (int rc = scene_check(s, &nH, &nW, false)) return rc;
  if (!out) return eae_set_error(EAE_ERR_ARG, "scene_windows: NULL output");
  if (B <= 0 || first < 0 || first + B > nH * nW) return eae_set_error(EAE_ERR_ARG, "scene_windows: windows outside the grid");
  EAE_NO_GROUP("scene_windows_kernel");
  const hipStream_t st = (hipStream_t)stream;
  const long long plane = (long long)s->H * s->W, tot = (long long)B * s->patch * s->patch;
  const dim3 grid((unsigned)((tot + 255) / 256));
  SceneSrc bs;
  eae_scene_fill_src(s, nW, first, &bs);
  scene_dtype_dispatch(s, [&](auto* t, auto border) {
    using T = std::remove_cv_t<std::remove_pointer_t<decltype(t)>>;
    hipLaunchKernelGGL((scene_windows_kernel<T, decltype(border)::value>), grid, dim3(256), 0, st, (const T*)s->data, s->divisor, s->C,
                       plane, s->W, s->patch, s->stride, (int)nW, first, B, out, bs.b);
  });
  EAE_LAUNCH_CHECK();
  return 0;
}

// both blends: the plain one passes labels = NULL, which its kernel never reads
template <bool VALID>
static int scene_blend(void* stream, const float* probs, const long long* labels, int K, int nH, int nW, int k, float* cell,
                       long long* cell_labels) {
  if (!probs || (VALID && !labels) || !cell || !cell_labels) return eae_set_error(EAE_ERR_ARG, "scene_blend: NULL argument");
  if (K < 1 || nH < 1 || nW < 1 || k < 1) return eae_set_error(EAE_ERR_ARG, "scene_blend: bad shape");
  EAE_NO_GROUP("scene_blend_kernel");
  const long long tot = (long long)(nH + k - 1) * (nW + k - 1);
  hipLaunchKernelGGL(scene_blend_kernel<VALID>, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, probs, K, nH, nW, k, cell, cell_labels, labels);
  EAE_LAUNCH_CHECK();
  return 0;
}
extern "C" int eae_scene_blend(void* stream, const float* probs, int K, int nH, int nW, int k, float* cell, long long* cell_labels) {
  return scene_blend<false>(stream, probs, nullptr, K, nH, nW, k, cell, cell_labels);
}
extern "C" int eae_scene_blend_valid(void* stream, const float* probs, const long long* labels, int K, int nH, int nW, int k, float* cell,
                                     long long* cell_labels) {
  return scene_blend<true>(stream, probs, labels, K, nH, nW, k, cell, cell_labels);
}

extern "C" int eae_scene_invalid_counts(void* stream, const eae_scene* s, int nodata_mode, float nodata, int rule,
                                        const unsigned char* mask, int* rows, int* counts) {
  long long nH = 0, nW = 0;
  if (int rc = eae_scene_check(s, &nH, &nW)) return rc;
  if (!rows || !counts) return eae_set_error(EAE_ERR_ARG, "scene_invalid_counts: NULL rows or counts");
  if (nodata_mode != EAE_NODATA_NONE && nodata_mode != EAE_NODATA_VALUE && nodata_mode != EAE_NODATA_NAN)
    return eae_set_error(EAE_ERR_ARG, "scene_invalid_counts: unknown nodata mode");
  if (rule != EAE_INVALID_ALL && rule != EAE_INVALID_ANY) return eae_set_error(EAE_ERR_ARG, "scene_invalid_counts: unknown rule");
  if (s->dtype != EAE_SCENE_F32 && nodata_mode == EAE_NODATA_NAN)
    return eae_set_error(EAE_ERR_ARG, "scene_invalid_counts: a NaN nodata needs an fp32 scene");
  if (s->dtype != EAE_SCENE_F32 && nodata_mode == EAE_NODATA_VALUE) {
    const float hi = s->dtype == EAE_SCENE_U8 ? 255.f : 65535.f;
    if (!(nodata >= 0.f && nodata <= hi) || nodata != (float)(int)nodata)
      return eae_set_error(EAE_ERR_ARG, "scene_invalid_counts: nodata must be an integer in the scene dtype's range");
  }
  if (s->patch > INV_SPAN - 16) return eae_set_error(EAE_ERR_ARG, "scene_invalid_counts: the patch size must be at most 4080");
  EAE_NO_GROUP("scene_invalid_rows_kernel");
  const hipStream_t st = (hipStream_t)stream;
  const long long plane = (long long)s->H * s->W, Hg = eae_scene_extent(nH, s->patch, s->stride);
  const int J = (INV_SPAN - 15 - s->patch) / s->stride + 1;        // window columns per workgroup: (J - 1) S + P + shift <= INV_SPAN
  const int nchunk = (int)((nW + J - 1) / J);
  const long long nblk = Hg * nchunk;
  if (nblk * INV_NT > 0xffffffffLL) return eae_set_error(EAE_ERR_ARG, "scene_invalid_counts: scene too large");
  const int rany = rule == EAE_INVALID_ANY;
  SceneSrc bs;
  eae_scene_fill_src(s, nW, 0, &bs);
  scene_dtype_dispatch(s, [&](auto* t, auto border) {
    using T = std::remove_cv_t<std::remove_pointer_t<decltype(t)>>;
    hipLaunchKernelGGL((scene_invalid_rows_kernel<T, decltype(border)::value>), dim3((unsigned)nblk), dim3(INV_NT), 0, st,
                       (const T*)s->data, plane, s->C, s->W, s->patch, s->stride, (int)nW, J, nchunk, nodata_mode, nodata, rany, mask,
                       rows, bs.b);
  });
  EAE_LAUNCH_CHECK();
  const long long nwin = nH * nW;
  hipLaunchKernelGGL(scene_invalid_windows_kernel, dim3((unsigned)((nwin + 255) / 256)), dim3(256), 0, st, rows, (int)nH, (int)nW,
                     s->patch, s->stride, counts);
  EAE_LAUNCH_CHECK();
  return 0;
}

extern "C" int eae_scene_select(void* stream, const int* counts, long long n, int threshold, long long* windows, long long* count) {
  if (!counts || !windows || !count) return eae_set_error(EAE_ERR_ARG, "scene_select: NULL argument");
  if (n < 1) return eae_set_error(EAE_ERR_ARG, "scene_select: empty grid");
  EAE_NO_GROUP("scene_select_kernel");
  hipLaunchKernelGGL(scene_select_kernel, dim3(1), dim3(SEL_NT), 0, (hipStream_t)stream, counts, n, threshold, windows, count);
  EAE_LAUNCH_CHECK();
  return 0;
}

// the checks of eae_scene_stage_windows[_aug] (the kernel and its launcher are eae_stage.hip's); nH, nW: the grid
static int scene_stage_check(const eae_scene* s, const long long* windows, int B, const float* out, int crop, long long* nH, long long* nW) {
  if (int rc = scene_check(s, nH, nW, false)) return rc;
  if (s->border != EAE_BORDER_NONE) return eae_set_error(EAE_ERR_ARG, "scene_stage_windows: border modes are not supported");
  if (!windows || !out) return eae_set_error(EAE_ERR_ARG, "scene_stage_windows: NULL windows or output");
  if (B <= 0) return eae_set_error(EAE_ERR_ARG, "scene_stage_windows: B must be positive");
  if (crop != EAE_CROP_WINDOW && crop != EAE_CROP_SCENE) return eae_set_error(EAE_ERR_ARG, "scene_stage_windows: unknown crop mode");
  return 0;
}

extern "C" int eae_scene_stage_windows(void* stream, const eae_scene* s, const long long* windows, int B, float* out, int train,
                                       float noise_std, unsigned long long seed, unsigned long long step, const int* params,
                                       const float* noise, int crop) {
  long long nH = 0, nW = 0;
  if (int rc = scene_stage_check(s, windows, B, out, crop, &nH, &nW)) return rc;
  return eae_launch_scene_stage_plain((hipStream_t)stream, s, nW, nH * nW, windows, B, out, train, noise_std, seed, step, params, noise,
                                      crop);
}

// with an augmentation policy (include/eae.h, "augmentation policy")
extern "C" int eae_scene_stage_windows_aug(void* stream, const eae_scene* s, const long long* windows, int B, float* out, int train,
                                           float noise_std, unsigned long long seed, unsigned long long step, const eae_aug* aug,
                                           const int* geom, const float* affine, const float* radio, const float* noise, int crop) {
  long long nH = 0, nW = 0;
  if (int rc = scene_stage_check(s, windows, B, out, crop, &nH, &nW)) return rc;
  StageAug a;
  if (int rc = eae_stage_aug_prepare(aug, geom, affine, radio, s->patch, s->patch, "scene_stage_windows", &a)) return rc;
  return eae_launch_scene_stage((hipStream_t)stream, s, nW, nH * nW, windows, B, out, train, noise_std, seed, step, a, noise, crop);
}

extern "C" int eae_scene_window_labels(void* stream, const void* raster, int elem_bytes, int H, int W, int patch, int stride, int K,
                                       long long* label, int* count, int* labelled) {
  if (!raster || !label) return eae_set_error(EAE_ERR_ARG, "scene_window_labels: NULL raster or label");
  if (elem_bytes != 1 && elem_bytes != 4) return eae_set_error(EAE_ERR_ARG, "scene_window_labels: raster must be uint8 or int32 (elem_bytes 1 or 4)");
  if (K < 1 || K > 64) return eae_set_error(EAE_ERR_ARG, "scene_window_labels: the number of classes must be in 1..64");
  if (patch < 1 || patch > INV_SPAN - 16) return eae_set_error(EAE_ERR_ARG, "scene_window_labels: the patch size must be in 1..4080");
  if (stride < 1 || stride > patch) return eae_set_error(EAE_ERR_ARG, "scene_window_labels: stride must be in 1..patch");
  if (H < patch || W < patch) return eae_set_error(EAE_ERR_ARG, "scene_window_labels: raster smaller than one window");
  const long long nH = (H - patch) / stride + 1, nW = (W - patch) / stride + 1;
  if (nH * nW > 0x7fffffffLL) return eae_set_error(EAE_ERR_ARG, "scene_window_labels: raster too large");
  EAE_NO_GROUP("scene_window_labels_kernel");
  const hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)(nH * nW));
  if (elem_bytes == 1)
    hipLaunchKernelGGL(scene_window_labels_kernel<uint8_t>, grid, dim3(LBL_NT), 0, st, (const uint8_t*)raster, W, patch, stride, (int)nW, K,
                       label, count, labelled);
  else
    hipLaunchKernelGGL(scene_window_labels_kernel<int32_t>, grid, dim3(LBL_NT), 0, st, (const int32_t*)raster, W, patch, stride, (int)nW, K,
                       label, count, labelled);
  EAE_LAUNCH_CHECK();
  return 0;
}

extern "C" int eae_scene_confusion(void* stream, const void* truth, int elem_bytes, int H, int W, const long long* pred, int cH, int cW,
                                   int cell, int oy, int ox, const unsigned char* mask, int K, int accumulate, long long* counts) {
  if (!truth || !pred || !counts) return eae_set_error(EAE_ERR_ARG, "scene_confusion: NULL truth, pred or counts");
  if (elem_bytes != 1 && elem_bytes != 4) return eae_set_error(EAE_ERR_ARG, "scene_confusion: truth must be uint8 or int32 (elem_bytes 1 or 4)");
  if (K < 1 || K > 64) return eae_set_error(EAE_ERR_ARG, "scene_confusion: the number of classes must be in 1..64");
  if (cell < 1) return eae_set_error(EAE_ERR_ARG, "scene_confusion: the cell size must be positive");
  if (oy < 0 || ox < 0) return eae_set_error(EAE_ERR_ARG, "scene_confusion: the origin must not be negative");
  if (H < 1 || W < 1 || cH < 1 || cW < 1) return eae_set_error(EAE_ERR_ARG, "scene_confusion: empty raster or map");
  if (accumulate != 0 && accumulate != 1) return eae_set_error(EAE_ERR_ARG, "scene_confusion: accumulate must be 0 or 1");
  EAE_NO_GROUP("scene_confusion_kernel");
  const hipStream_t st = (hipStream_t)stream;
  const int nbin = (K + 1) * (K + 1);
  if (!accumulate && hipMemsetAsync(counts, 0, (size_t)nbin * sizeof(long long), st) != hipSuccess)
    return eae_set_error(-3, "scene_confusion: clearing counts failed");
  // bounded grid (8 workgroups on each of 256 CUs), raised only where a workgroup's share of tiles would reach 2^31 pixels
  const unsigned G = (unsigned)(((long long)W + 2 * CONF_RUN - 2) / CONF_RUN);          // ceil((W + 15) / 16) run slots per row
  const long long ntiles = ((long long)H * G + CONF_NT - 1) / CONF_NT;
  const long long max_share = (0x7fffffffLL / (CONF_NT * CONF_RUN)) - 1;          // tiles per workgroup
  long long grid = ntiles < 2048 ? ntiles : 2048;
  if ((ntiles + grid - 1) / grid > max_share) grid = (ntiles + max_share - 1) / max_share;
  if (grid > 0x7fffffffLL) return eae_set_error(EAE_ERR_ARG, "scene_confusion: raster too large");
  const size_t lds = (size_t)nbin * sizeof(int);
  if (elem_bytes == 1)
    hipLaunchKernelGGL(scene_confusion_kernel<uint8_t>, dim3((unsigned)grid), dim3(CONF_NT), lds, st, (const uint8_t*)truth, H, W, pred, cH,
                       cW, (unsigned)cell, (unsigned)oy, (unsigned)ox, mask, K, G, ntiles, (unsigned long long*)counts);
  else
    hipLaunchKernelGGL(scene_confusion_kernel<int32_t>, dim3((unsigned)grid), dim3(CONF_NT), lds, st, (const int32_t*)truth, H, W, pred, cH,
                       cW, (unsigned)cell, (unsigned)oy, (unsigned)ox, mask, K, G, ntiles, (unsigned long long*)counts);
  EAE_LAUNCH_CHECK();
  return 0;
}

// ---- scene calls: one checked window set and one batch driver under the seven entry points
namespace {
// The window set of a scene call.  windows == NULL: the range first .. first + count - 1 of the grid; otherwise the ids windows[0 .. count)
// (first must be 0).  The ids stay on the device (no host synchronisation): the kernels read an id outside the grid as an all-zero window
// and the epilogues write nothing for it.  Returns the grid (nH, nW).
int scene_set_checks(eae_ctx* c, const eae_scene* s, long long first, const long long* windows, long long count, long long* nH,
                     long long* nW) {
  if (windows && count <= 0) return eae_set_error(EAE_ERR_ARG, "scene: the window list is empty");
  if (!c) return eae_set_error(EAE_ERR_ARG, "scene: NULL context");
  if (!c->P || !c->bnrun) return eae_set_error(EAE_ERR_STATE, "eae_bind has not been called");
  if (c->fp8) return eae_set_error(EAE_ERR_ARG, "scene: quant=1 (fp8) contexts are not supported");
  RC(eae_scene_check(s, nH, nW));
  if (s->C != c->Cin) return eae_set_error(EAE_ERR_ARG, "scene: band count does not match the encoder's in_channels");
  if (c->H != c->W || s->patch != c->H) return eae_set_error(EAE_ERR_ARG, "scene: the patch must be the (square) image size of the model");
  if (windows ? first != 0 : count <= 0 || first < 0 || first + count > *nH * *nW)
    return eae_set_error(EAE_ERR_ARG, "scene: windows outside the grid");
  return 0;
}
int scene_list_check(const long long* windows) { return windows ? 0 : eae_set_error(EAE_ERR_ARG, "scene: NULL window list"); }

// The batch driver: the checked window set in batches of max_batch, each encoded into c->z (rows of Lp floats) by conv1 reading the scene,
// then handed to body(b0, nb, src): b0 = the batch's offset in the set, nb its size, src the scene source the encoder read.
template <typename Body>
int scene_run(eae_ctx* c, hipStream_t st, const eae_scene* s, long long nH, long long nW, long long first, const long long* windows,
              long long count, Body body) {
  invalidate_forward(c);
  c->fwd_gen += 1;          // scene activations are never differentiated: a backward of an earlier forward is refused
  RC(ensure_packed(c, st));
  RC(prep_accumulators(c, st, false));
  for (long long b0 = 0; b0 < count; b0 += c->Bm) {
    const int nb = (int)(count - b0 < c->Bm ? count - b0 : c->Bm);
    SceneSrc src;
    eae_scene_fill_src(s, nW, first + b0, &src);
    src.index = windows; src.nwin = nH * nW;
    RC(run_encoder(c, st, nullptr, nb, false, s, &src));
    RC(body(b0, nb, src));
  }
  return 0;
}

int scene_encode(eae_ctx* c, void* stream, const eae_scene* s, long long first, const long long* windows, long long count, float* z) {
  long long nH = 0, nW = 0;
  RC(scene_set_checks(c, s, first, windows, count, &nH, &nW));
  if (!z) return eae_set_error(EAE_ERR_ARG, "scene_encode: NULL z");
  hipStream_t st = (hipStream_t)stream;
  return scene_run(c, st, s, nH, nW, first, windows, count,
                   [&](long long b0, int nb, const SceneSrc&) { return copy_latent_out(c, st, z + (size_t)b0 * c->L, c->z, nb); });
}

int scene_classify(eae_ctx* c, eae_mlp* m, void* stream, const eae_scene* s, long long first, const long long* windows, long long count,
                   float* probs, long long* labels) {
  long long nH = 0, nW = 0;
  RC(scene_set_checks(c, s, first, windows, count, &nH, &nW));
  if (!m || !probs || !labels) return eae_set_error(EAE_ERR_ARG, "scene_classify: NULL mlp, probs or labels");
  int in_dim = 0, classes = 0, mb = 0;
  RC(eae_mlp_dims(m, &in_dim, &classes, &mb));
  if (in_dim != c->L) return eae_set_error(EAE_ERR_ARG, "scene_classify: the MLP's input_dim is not the encoder's latent_dim");
  hipStream_t st = (hipStream_t)stream;
  return scene_run(c, st, s, nH, nW, first, windows, count, [&](long long b0, int nb, const SceneSrc&) {
    return eae_mlp_predict(m, st, c->z, c->Lp, nb, first + b0, nH * nW, probs, labels, windows);
  });
}

// scene reconstruction: encoder -> decoder over the window set, deconv4's MSE target read from the scene itself.  Per batch the decoder up to
// deconv4, the scene-target deconv4 and the per-window finalize.  err may be NULL (reconstruct), recon may be NULL (error maps).
int scene_recon(eae_ctx* c, void* stream, const eae_scene* s, long long first, const long long* windows, long long count, float* err,
                float* band_err, float* recon, float* residual) {
  long long nH = 0, nW = 0;
  RC(scene_set_checks(c, s, first, windows, count, &nH, &nW));
  if (!c->has_enc || !c->has_dec)
    return eae_set_error(EAE_ERR_STATE, "scene reconstruction needs both halves bound (the engine of a stand-alone Encoder has no decoder)");
  if (!err && !recon) return eae_set_error(EAE_ERR_ARG, "scene reconstruction: NULL output");
  if (recon && (s->patch - s->stride) % 2)
    return eae_set_error(EAE_ERR_ARG, "scene_reconstruct: patch - stride must be even (the owned spans are centred)");
  Deconv4SceneArgs r;
  r.part = c->msepart;         // [tiles][edge_lp_stride(C)] floats were carved: edge_bp_stride(C) <= edge_lp_stride(C)
  r.recon = recon; r.residual = residual;
  r.Wg = (int)eae_scene_extent(nW, s->patch, s->stride);
  r.gplane = eae_scene_extent(nH, s->patch, s->stride) * r.Wg;
  if (s->border) { r.Wg = s->W; r.gplane = (long long)s->H * s->W; }      // the stitched raster of a bordered scene is the real scene
  r.nH = (int)nH; r.m = (s->patch - s->stride) / 2;
  hipStream_t st = (hipStream_t)stream;
  return scene_run(c, st, s, nH, nW, first, windows, count, [&](long long b0, int nb, const SceneSrc& src) {
    Deconv4Args d;
    RC(run_decoder_trunk(c, st, c->z, nb, false, d));
    RC(eae_launch_deconv4_scene(st, eae_scene_src3_kind(s), d, src, r));
    if (err) RC(eae_launch_scene_err_finalize(st, c->msepart, nb, s->patch, s->C, first + b0, windows, nH * nW, err, band_err));
    return 0;
  });
}
}  // namespace

extern "C" int eae_scene_encode(eae_ctx* c, void* stream, const eae_scene* s, long long first, int B, float* z) {
  return scene_encode(c, stream, s, first, nullptr, B, z);
}
extern "C" int eae_scene_encode_windows(eae_ctx* c, void* stream, const eae_scene* s, const long long* windows, long long count,
                                        float* z) {
  RC(scene_list_check(windows));
  return scene_encode(c, stream, s, 0, windows, count, z);
}

extern "C" int eae_scene_classify(eae_ctx* c, eae_mlp* m, void* stream, const eae_scene* s, long long first, long long count, float* probs,
                                  long long* labels) {
  return scene_classify(c, m, stream, s, first, nullptr, count, probs, labels);
}
extern "C" int eae_scene_classify_windows(eae_ctx* c, eae_mlp* m, void* stream, const eae_scene* s, const long long* windows,
                                          long long count, float* probs, long long* labels) {
  RC(scene_list_check(windows));
  return scene_classify(c, m, stream, s, 0, windows, count, probs, labels);
}

extern "C" int eae_scene_recon_error(eae_ctx* c, void* stream, const eae_scene* s, long long first, long long count, float* err,
                                     float* band_err) {
  return scene_recon(c, stream, s, first, nullptr, count, err, band_err, nullptr, nullptr);
}
extern "C" int eae_scene_recon_error_windows(eae_ctx* c, void* stream, const eae_scene* s, const long long* windows, long long count,
                                             float* err, float* band_err) {
  RC(scene_list_check(windows));
  return scene_recon(c, stream, s, 0, windows, count, err, band_err, nullptr, nullptr);
}
extern "C" int eae_scene_reconstruct(eae_ctx* c, void* stream, const eae_scene* s, const long long* windows, long long count, float* recon,
                                     float* residual) {
  return scene_recon(c, stream, s, 0, windows, count, nullptr, nullptr, recon, residual);
}
