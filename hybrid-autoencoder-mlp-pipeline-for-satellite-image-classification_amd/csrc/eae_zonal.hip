// Zonal statistics (include/eae.h, "zonal statistics"): what a class map says inside every zone of a zone raster,
// and a per-zone value painted back at pixel resolution.
//   accumulate: the raster is streamed in RUNS of 16 consecutive pixels of one row that start at a 16-element boundary of its memory
//               (scene_confusion_kernel's unit: whole runs are 16-byte loads, the clipped first and last runs of a row load element by
//               element).  A thread keeps one OPEN KEY (zone, cell) with a pixel count and flushes it only when the key changes: `run`
//               to the zone's vote and `run * q` to its K probability sums.  A workgroup owns a vertical strip of tiles (same columns,
//               consecutive rows) and the key stays open from row to row, so the interior of a parcel is flushed once per cell, not
//               once per row.  A flush goes to a table in LDS, one row of K + 1 (+ K) 64-bit counters per zone the workgroup has
//               met, found by a bounded hash probe; a zone that finds no row adds to global memory directly.  The table goes to
//               global memory with 64-bit integer atomics when the strip ends, or at the next barrier after a zone found no row
//               (which empties it for the zones that follow).
//   paint:      four ids per thread from a 16-byte boundary, two 16-byte stores through a buffer window of the workgroup's own span.
// Integers only: 64-bit integer adds in LDS and in global memory, no float atomics.  Integer addition is associative, so the tables do
// not depend on which adds were merged, on the table's occupancy, on the launch geometry or on the order of arrival.
#include "eae_internal.h"
#include "eae_common.hip.h"

namespace {

constexpr int ZN_NT = 256, ZN_RUN = 16;
constexpr int ZN_PROBES = 4;                 // rows tried for a zone before it goes to global memory directly
constexpr int ZN_LDS_BYTES = 48 * 1024;      // the counters of the LDS table (the keys come on top); 24 KiB measured slower
constexpr int ZN_MAX_ROWS = 512;
constexpr int ZN_GRID = 1024;                // workgroups at most (4 on each of 256 CUs): longer strips, fewer end-of-strip flushes
constexpr int ZN_SYNC = 4;                   // tiles between two barriers (the vote on emptying the table)
constexpr int ZN_QB = 4;                     // probabilities loaded together ahead of their adds

typedef unsigned long long u64;
// the table's pointers carry the LDS address space: its adds are then LDS instructions whatever the compiler does with the branches
// around them (a pointer that may be LDS or global makes every add a flat one)
typedef __attribute__((address_space(3))) u64 lds_u64;
typedef __attribute__((address_space(3))) int lds_int;
__device__ __forceinline__ void lds_add(lds_u64* p, u64 v) { __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
// the workgroup barrier, from builtins for the same reason as glb_add below
__device__ __forceinline__ void wg_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}
// (the builtin, not atomicAdd(): the library function lacks the kernel's EAE_NO_PK target attribute and would stay a call, section 18)
__device__ __forceinline__ void glb_add(u64* p, u64 v) { __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// q(p) = rint(2^32 * min(max(p, 0), 1)) in double, round-half-even; NaN -> 0 (the first comparison is false).  A float times 2^32 is
// exact in double, so this is the NumPy expression of the header bit for bit.
__device__ __forceinline__ u64 zonal_q(float p) {
  const float c = p > 0.f ? (p < 1.f ? p : 1.f) : 0.f;
  return (u64)__builtin_rint((double)c * 4294967296.0);
}

// the table column of cell x of a map row: its label in [0, K), else K (rowin: the row lies inside the map; lrow is read only then)
__device__ __forceinline__ int zonal_cell_class(const long long* __restrict__ lrow, bool rowin, unsigned cW, unsigned x, int K) {
  if (!rowin || x >= cW) return K;
  const long long v = lrow[x];
  return v >= 0 && v < K ? (int)v : K;
}

struct ZonalTab {
  lds_int* keys;      // [rows]: the zone of a row, -1 = free; keys[rows], keys[rows + 1]: the spill flags of the votes on emptying the table
  lds_u64* cnt;       // [rows][RW]: votes [K + 1], then probability sums [K] (with probs)
  int rows, shift, RW, K;
  u64 *votes, *psums;
  const long long* labels;
  const float* probs;
  unsigned cH, cW;
};

// One flush: `run` pixels of zone z in cell (cy, cx).  Returns true when the zone found no row of the table (the adds then went to
// global memory).
__device__ __forceinline__ bool zonal_flush(const ZonalTab& t, int z, unsigned cy, unsigned cx, unsigned run) {
  const long long cellidx = (long long)cy * t.cW + cx;      // read only for a cell inside the map
  const int c = zonal_cell_class(t.labels + (long long)cy * t.cW, cy < t.cH, t.cW, cx, t.K);
  const long long plane = (long long)t.cH * t.cW;
  unsigned h = ((unsigned)z * 0x9E3779B1u) >> t.shift;
  int row = -1;
#pragma unroll
  for (int p = 0; p < ZN_PROBES; ++p) {
    int k = __hip_atomic_load(t.keys + h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (k == -1) {
      int expected = -1;      // claim the free row; a lost race leaves the winner's zone in `expected`
      k = __hip_atomic_compare_exchange_strong(t.keys + h, &expected, z, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)
              ? z : expected;
    }
    if (k == z) { row = (int)h; break; }
    h = (h + 1) & (unsigned)(t.rows - 1);
  }
  if (row >= 0) lds_add(t.cnt + row * t.RW + c, (u64)run);
  else glb_add(t.votes + (size_t)z * (t.K + 1) + c, (u64)run);
  if (t.probs && c < t.K) {
    const float* pp = t.probs + cellidx;
    for (int j0 = 0; j0 < t.K; j0 += ZN_QB) {               // the loads of a batch are issued together, ahead of its adds
      float pv[ZN_QB];
#pragma unroll
      for (int i = 0; i < ZN_QB; ++i) pv[i] = j0 + i < t.K ? pp[(j0 + i) * plane] : 0.f;
#pragma unroll
      for (int i = 0; i < ZN_QB; ++i)
        if (j0 + i < t.K) {
          if (row >= 0) lds_add(t.cnt + row * t.RW + t.K + 1 + j0 + i, run * zonal_q(pv[i]));
          else glb_add(t.psums + (size_t)z * t.K + j0 + i, run * zonal_q(pv[i]));
        }
    }
  }
  return row < 0;
}

// The table to global memory: consecutive threads take consecutive counters of a row (contiguous segments of a table row), zeros are
// skipped.  Every thread of the workgroup calls it, between barriers; it leaves the table empty.
__device__ __forceinline__ void zonal_drain(const ZonalTab& t, int tid) {
  const int n = t.rows * t.RW, K1 = t.K + 1;
  for (int i = tid; i < n; i += ZN_NT) {
    const u64 v = t.cnt[i];
    if (!v) continue;
    const int row = i / t.RW, e = i - row * t.RW, z = t.keys[row];
    t.cnt[i] = 0;
    if (e < K1) glb_add(t.votes + (size_t)z * K1 + e, v);
    else glb_add(t.psums + (size_t)z * t.K + (e - K1), v);
  }
  wg_barrier();
  for (int i = tid; i < t.rows; i += ZN_NT) t.keys[i] = -1;
  if (tid == 0) { t.keys[t.rows] = 0; t.keys[t.rows + 1] = 0; }
  wg_barrier();
}

// 16 ids of a run as ints: the id when it is in [0, Z) (Z < 2^31), else -1
template <typename T> __device__ __forceinline__ int zonal_id(T v, long long Z) { return v >= 0 && (long long)v < Z ? (int)v : -1; }

// Tile (ty, tx) = TH rows x TW run slots (TW * TH = ZN_NT, TW = 1 << tw_log2: narrow rasters fill a workgroup with several rows);
// tiles are numbered tx * tilesY + ty and a workgroup takes `chunk` consecutive ones: a vertical strip.
template <typename T>
__global__ EAE_NO_PK __launch_bounds__(ZN_NT) void zonal_accumulate_kernel(const T* __restrict__ zones, int H, int W,
                                                                        const long long* __restrict__ labels,
                                                                        const float* __restrict__ probs, int cH, int cW, unsigned cell,
                                                                        unsigned oy, unsigned ox, const unsigned char* __restrict__ mask,
                                                                        int K, long long Z, unsigned G, int tw_log2, long long tilesY,
                                                                        long long ntiles, long long chunk, int rows, u64* votes,
                                                                        u64* psums) {
  extern __shared__ u64 zonal_lds[];                       // cnt [rows][RW], then keys [rows + 2]
  constexpr int V = ZN_RUN;
  const int tid = threadIdx.x;
  ZonalTab t;
  t.rows = rows;
  t.shift = 32 - (31 - __builtin_clz((unsigned)rows));     // rows is a power of two >= 2
  t.K = K;
  t.RW = K + 1 + (probs ? K : 0);
  t.cnt = (lds_u64*)zonal_lds;
  t.keys = (lds_int*)(zonal_lds + (size_t)rows * t.RW);
  t.votes = votes;
  t.psums = psums;
  t.labels = labels;
  t.probs = probs;
  t.cH = (unsigned)cH;
  t.cW = (unsigned)cW;
  for (int i = tid; i < rows * t.RW; i += ZN_NT) t.cnt[i] = 0;
  for (int i = tid; i < rows; i += ZN_NT) t.keys[i] = -1;
  if (tid == 0) { t.keys[rows] = 0; t.keys[rows + 1] = 0; }
  wg_barrier();
  const u64 base_el = reinterpret_cast<uintptr_t>(zones) / sizeof(T);        // element address of pixel (0, 0)
  const int TW = 1 << tw_log2, TH = ZN_NT >> tw_log2;
  const unsigned dy = (unsigned)tid >> tw_log2, dg = (unsigned)tid & (unsigned)(TW - 1);
  const long long t0 = blockIdx.x * chunk, t1 = t0 + chunk < ntiles ? t0 + chunk : ntiles;
  // the open key of this thread: `run` pixels of zone curz in cell (cury, curx) that have gone nowhere yet; curz = -1: none.  It
  // stays open from one tile to the next: in a strip of one-row tiles the thread meets the same columns row after row, so the
  // interior of a parcel is flushed once per cell, not once per row.
  int curz = -1;
  unsigned curx = 0, cury = 0, run = 0;
  bool spilled = false;
  for (long long ti = t0; ti < t1; ++ti) {                 // workgroup-uniform trip count: every thread reaches the barriers
    const long long tx = ti / tilesY, ty = ti - tx * tilesY;
    const long long y = ty * TH + dy;
    const unsigned long long g = (unsigned long long)tx * TW + dg;
    if (y < H && g < G) {
      const long long row = y * W;
      const int m = (int)((base_el + (u64)row) & (V - 1));
      const long long gx = (long long)g * V - m;            // first column of the run; < 0 for a clipped first run
      const int lo = gx > 0 ? (int)gx : 0, hi = gx + V < W ? (int)(gx + V) : W;
      if (lo < hi) {                                        // (not the empty last slot of a row)
        const bool full = hi - lo == V;
        const T* p = zones + row + gx;                      // dereferenced at [lo - gx, hi - gx) only
        int zv[V], mk[V];                                   // ids and mask bytes of the run (statically indexed: registers)
        if (full) {                                         // 16 elements from a 16-element boundary
          const uint4* p4 = reinterpret_cast<const uint4*>(p);
          if constexpr (sizeof(T) == 4) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const uint4 w = p4[i];
              zv[4 * i] = zonal_id((int)w.x, Z); zv[4 * i + 1] = zonal_id((int)w.y, Z);
              zv[4 * i + 2] = zonal_id((int)w.z, Z); zv[4 * i + 3] = zonal_id((int)w.w, Z);
            }
          } else {
#pragma unroll
            for (int i = 0; i < 8; ++i) {
              const uint4 w = p4[i];
              zv[2 * i] = zonal_id((long long)(((u64)w.y << 32) | w.x), Z);
              zv[2 * i + 1] = zonal_id((long long)(((u64)w.w << 32) | w.z), Z);
            }
          }
        } else {
#pragma unroll
          for (int v = 0; v < V; ++v) zv[v] = (gx + v >= lo && gx + v < hi) ? zonal_id(p[v], Z) : -1;
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
        // the cell of pixel (y, lo), stepped along the row
        const unsigned cy = ((unsigned)y + oy) / cell;
        unsigned cx = ((unsigned)lo + ox) / cell, rem = ((unsigned)lo + ox) - cx * cell;
        // (a one-step path for whole runs of one id was measured and is not here: the lanes of a wave rarely all qualify, so a wave
        // ran both paths, 273 against 240 us on the parcel case of tools/zonal_bench.py)
#pragma unroll
        for (int v = 0; v < V; ++v) {
          const bool in = gx + v >= lo && gx + v < hi;
          if (in) {
            const int z = mk[v] == 0 ? zv[v] : -1;
            if (z != curz || (z >= 0 && (cx != curx || cy != cury))) {
              if (curz >= 0) spilled |= zonal_flush(t, curz, cury, curx, run);
              curz = z;
              curx = cx;
              cury = cy;
              run = 0;
            }
            ++run;
            if (++rem == cell) { rem = 0; ++cx; }
          }
        }
      }
    }
    if (ti + 1 == t1 && curz >= 0) spilled |= zonal_flush(t, curz, cury, curx, run);      // the strip ends: close the open key
    // tiles in which a zone found no row: empty the table for the zones that follow
    if (((ti - t0) % ZN_SYNC) == ZN_SYNC - 1 || ti + 1 == t1) {
      // The votes alternate between two flags.  A wave that is late to read this vote's flag cannot find the next vote's write in
      // it: that goes to the other flag, and the write after that lies behind the next vote's barrier, which waits for the late
      // wave.  So every wave reads the same value and all of them drain or none does.  The drain clears both flags between its
      // barriers, when no vote is open.
      const int flag = t.rows + (int)(((ti - t0) / ZN_SYNC) & 1);
      if (spilled) t.keys[flag] = 1;
      wg_barrier();
      if (t.keys[flag]) zonal_drain(t, tid);
      spilled = false;
    }
  }
  zonal_drain(t, tid);
}

// out = values[zones] where the id is in [0, Z), else fill.  Unit u of the flattened raster = the 4 ids [4 u - m, 4 u - m + 4), m = the
// element misalignment of pixel 0 from a 4-element boundary: a whole unit is one 16-byte load of int32 ids (two of int64) and two
// 16-byte stores; the clipped first and last units go element by element.  The stores take the workgroup's own span as their buffer
// window (OutRsrc: a store outside it is dropped by the hardware), an element outside the raster stores at OOB_OFF.
constexpr int ZP_UNIT = 4;
template <typename T>
__global__ __launch_bounds__(ZN_NT) void zonal_paint_kernel(const T* __restrict__ zones, long long n, const long long* __restrict__ values,
                                                            long long Z, long long fill, long long* __restrict__ out) {
  const int m = (int)((reinterpret_cast<uintptr_t>(zones) / sizeof(T)) & (ZP_UNIT - 1));
  const long long wb = (long long)blockIdx.x * (ZN_NT * ZP_UNIT) - m;          // the workgroup's first element (< 0: clipped)
  const long long w0 = wb > 0 ? wb : 0, w1 = wb + ZN_NT * ZP_UNIT < n ? wb + ZN_NT * ZP_UNIT : n;
  OutRsrc o;
  o.init(out + w0, (long)(w1 - w0) * 8);
  const long long e0 = wb + (long long)threadIdx.x * ZP_UNIT;                  // the unit's first element
  if (e0 >= n) return;
  long long v[ZP_UNIT];
  const bool full = e0 >= 0 && e0 + ZP_UNIT <= n;
  const T* p = zones + e0;                                                     // dereferenced inside [0, n) only
  if (full) {
    const uint4* p4 = reinterpret_cast<const uint4*>(p);
    if constexpr (sizeof(T) == 4) {
      const uint4 w = p4[0];
      v[0] = (int)w.x; v[1] = (int)w.y; v[2] = (int)w.z; v[3] = (int)w.w;
    } else {
      const uint4 a = p4[0], b = p4[1];
      v[0] = (long long)(((u64)a.y << 32) | a.x); v[1] = (long long)(((u64)a.w << 32) | a.z);
      v[2] = (long long)(((u64)b.y << 32) | b.x); v[3] = (long long)(((u64)b.w << 32) | b.z);
    }
  } else {
#pragma unroll
    for (int i = 0; i < ZP_UNIT; ++i) v[i] = (e0 + i >= 0 && e0 + i < n) ? (long long)p[i] : -1;
  }
#pragma unroll
  for (int i = 0; i < ZP_UNIT; ++i) v[i] = v[i] >= 0 && v[i] < Z ? values[v[i]] : fill;
  const uint32_t off = (uint32_t)(e0 - w0) * 8u;            // full: e0 >= w0
  if (full) {
    o.st16<EAE_WT_ZONAL>(off, make_uint4((unsigned)v[0], (unsigned)((u64)v[0] >> 32), (unsigned)v[1], (unsigned)((u64)v[1] >> 32)));
    o.st16<EAE_WT_ZONAL>(off + 16u, make_uint4((unsigned)v[2], (unsigned)((u64)v[2] >> 32), (unsigned)v[3], (unsigned)((u64)v[3] >> 32)));
  } else {
#pragma unroll
    for (int i = 0; i < ZP_UNIT; ++i) {
      const bool in = e0 + i >= 0 && e0 + i < n;
      o.st8<EAE_WT_ZONAL>(in ? (uint32_t)(e0 + i - w0) * 8u : OOB_OFF, (u32x2){(unsigned)v[i], (unsigned)((u64)v[i] >> 32)});
    }
  }
}

int zonal_raster_check(const char* who, const void* zones, int elem_bytes, int H, int W) {
  static thread_local char msg[160];
  const char* what = nullptr;
  if (!zones) what = "NULL zones";
  else if (elem_bytes != 4 && elem_bytes != 8) what = "zones must be int32 or int64 (zone_elem_bytes 4 or 8)";
  else if (reinterpret_cast<uintptr_t>(zones) % (unsigned)elem_bytes) what = "the zones pointer is not aligned to its element size";
  else if (H < 1 || W < 1) what = "empty raster";
  else if ((long long)H * W >= (1LL << 31)) what = "H * W must be below 2^31";
  if (!what) return 0;
  snprintf(msg, sizeof msg, "%s: %s", who, what);
  return eae_set_error(EAE_ERR_ARG, msg);
}

}  // namespace

extern "C" int eae_zonal_accumulate(void* stream, const void* zones, int zone_elem_bytes, int H, int W, const long long* labels,
                                    const float* probs, int cH, int cW, int cell, int oy, int ox, const unsigned char* mask, int K,
                                    long long Z, int accumulate, long long* votes, long long* prob_sums) {
  if (int rc = zonal_raster_check("zonal_accumulate", zones, zone_elem_bytes, H, W)) return rc;
  if (!labels || !votes) return eae_set_error(EAE_ERR_ARG, "zonal_accumulate: NULL labels or votes");
  if ((probs != nullptr) != (prob_sums != nullptr))
    return eae_set_error(EAE_ERR_ARG, "zonal_accumulate: probs and prob_sums must be given together or not at all");
  if (K < 1 || K > 64) return eae_set_error(EAE_ERR_ARG, "zonal_accumulate: the number of classes must be in 1..64");
  if (Z < 1 || Z > 0x7fffffffLL / (K + 1)) return eae_set_error(EAE_ERR_ARG, "zonal_accumulate: Z must be >= 1 and Z * (K + 1) <= 2^31 - 1");
  if (cell < 1) return eae_set_error(EAE_ERR_ARG, "zonal_accumulate: the cell size must be positive");
  if (oy < 0 || ox < 0) return eae_set_error(EAE_ERR_ARG, "zonal_accumulate: the origin must not be negative");
  if (cH < 1 || cW < 1) return eae_set_error(EAE_ERR_ARG, "zonal_accumulate: empty map");
  if (accumulate != 0 && accumulate != 1) return eae_set_error(EAE_ERR_ARG, "zonal_accumulate: accumulate must be 0 or 1");
  EAE_NO_GROUP("zonal_accumulate_kernel");
  const hipStream_t st = (hipStream_t)stream;
  if (!accumulate && (hipMemsetAsync(votes, 0, (size_t)Z * (K + 1) * sizeof(long long), st) != hipSuccess ||
                      (prob_sums && hipMemsetAsync(prob_sums, 0, (size_t)Z * K * sizeof(long long), st) != hipSuccess)))
    return eae_set_error(EAE_ERR_HIP, "zonal_accumulate: clearing the tables failed");
  // the tile: the smallest power of two of run slots that holds a row, at most a workgroup's 256; the rest of the workgroup takes rows
  const unsigned G = (unsigned)(((long long)W + 2 * ZN_RUN - 2) / ZN_RUN);             // ceil((W + 15) / 16) run slots per row
  int tw_log2 = 0;
  while ((1u << tw_log2) < G && (1 << tw_log2) < ZN_NT) ++tw_log2;
  const int TW = 1 << tw_log2, TH = ZN_NT / TW;
  const long long tilesX = ((long long)G + TW - 1) / TW, tilesY = ((long long)H + TH - 1) / TH, ntiles = tilesX * tilesY;
  // bounded grid, every workgroup a strip of `chunk` consecutive tiles
  const long long chunk = (ntiles + ZN_GRID - 1) / ZN_GRID, grid = (ntiles + chunk - 1) / chunk;
  // the LDS table: the largest power of two of rows whose counters fit ZN_LDS_BYTES (K = 64 with probs: 32 rows; K = 10: 256)
  const int RW = K + 1 + (probs ? K : 0);
  int rows = 2;
  while (rows * 2 <= ZN_MAX_ROWS && (size_t)rows * 2 * RW * sizeof(u64) <= (size_t)ZN_LDS_BYTES) rows *= 2;
  const size_t lds = (size_t)rows * RW * sizeof(u64) + (size_t)(rows + 2) * sizeof(int);
  if (zone_elem_bytes == 4)
    hipLaunchKernelGGL(zonal_accumulate_kernel<int32_t>, dim3((unsigned)grid), dim3(ZN_NT), lds, st, (const int32_t*)zones, H, W, labels,
                       probs, cH, cW, (unsigned)cell, (unsigned)oy, (unsigned)ox, mask, K, Z, G, tw_log2, tilesY, ntiles, chunk, rows,
                       (u64*)votes, (u64*)prob_sums);
  else
    hipLaunchKernelGGL(zonal_accumulate_kernel<long long>, dim3((unsigned)grid), dim3(ZN_NT), lds, st, (const long long*)zones, H, W,
                       labels, probs, cH, cW, (unsigned)cell, (unsigned)oy, (unsigned)ox, mask, K, Z, G, tw_log2, tilesY, ntiles, chunk,
                       rows, (u64*)votes, (u64*)prob_sums);
  EAE_LAUNCH_CHECK();
  return 0;
}

extern "C" int eae_zonal_paint(void* stream, const void* zones, int zone_elem_bytes, int H, int W, const long long* values, long long Z,
                               long long fill, long long* out) {
  if (int rc = zonal_raster_check("zonal_paint", zones, zone_elem_bytes, H, W)) return rc;
  if (!values || !out) return eae_set_error(EAE_ERR_ARG, "zonal_paint: NULL values or out");
  if (Z < 1) return eae_set_error(EAE_ERR_ARG, "zonal_paint: Z must be >= 1");
  EAE_NO_GROUP("zonal_paint_kernel");
  const long long n = (long long)H * W;
  // units start m elements ahead of pixel 0 (the kernel's m): ceil((n + m) / 1024) workgroups, none of them empty
  const long long m = (long long)((reinterpret_cast<uintptr_t>(zones) / (unsigned)zone_elem_bytes) & (ZP_UNIT - 1));
  const long long blocks = (n + m + ZN_NT * ZP_UNIT - 1) / (ZN_NT * ZP_UNIT);
  if (zone_elem_bytes == 4)
    hipLaunchKernelGGL(zonal_paint_kernel<int32_t>, dim3((unsigned)blocks), dim3(ZN_NT), 0, (hipStream_t)stream, (const int32_t*)zones, n,
                       values, Z, fill, out);
  else
    hipLaunchKernelGGL(zonal_paint_kernel<long long>, dim3((unsigned)blocks), dim3(ZN_NT), 0, (hipStream_t)stream, (const long long*)zones,
                       n, values, Z, fill, out);
  EAE_LAUNCH_CHECK();
  return 0;
}
