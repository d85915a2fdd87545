// Map post-processing (include/eae.h, "map post-processing"): what cleans a class map on the device.
//   majority:     mode filter over a clipped (2r+1)^2 window, an int8 tile with its halo in LDS; the classes present in a window are
//                 gathered into a 64-bit mask and only those are counted, the count in a scalar register per pass.
//   regions:      (eae_map_regions for classes in [0, K), eae_map_regions_wide for arbitrary int64 labels: one set of kernels, templated
//                 on how a cell's label is read and kept)
//                 connected-component labelling by union-find with union-by-minimum in three launches: every 32 x 32 tile is labelled
//                 in LDS and its parents written as global linear indices; the tile borders are merged with device-scope atomics on the
//                 parent array; every cell is flattened to its root.  A root is the smallest linear index of its set, so the result is
//                 unique: no dependence on the grid, on dispatch order or on the order in which the atomics arrive.
//   region_stats: area and bounding box per root with integer atomics, one set per horizontal run of a wave's 64 cells.
//   sieve_pass:   small regions take the class of their largest edge neighbour that is not small: a 64-bit atomicMax of
//                 (area << 32) | (0xFFFFFFFF - id) per small root, then one pass that rewrites the cells.
// Integers only: vector stores and integer atomics, no floating point anywhere.  No workgroup waits for another one.
#include "eae_internal.h"

namespace {

constexpr int RG_NT = 256;            // threads per workgroup: 4 waves
constexpr int RG_T = 32;              // tile edge of the labelling kernel (1024 cells, 4 per thread)
constexpr int RG_CELLS = RG_T * RG_T;
constexpr int MJ_RMAX = 7;
constexpr int MJ_SIDE = RG_T + 2 * MJ_RMAX;   // 46: tile + halo at the largest radius
constexpr int MJ_LD = 48;             // LDS row stride in bytes

__device__ __forceinline__ int cls_of(long long v, int K) { return v >= 0 && v < (long long)K ? (int)v : -1; }

// How the region kernels read a cell's label and keep it in LDS.  `read` maps the stored value to what two cells are compared by, a
// negative result being "unclassified".  ClassCell: a class in [0, K), K <= 64, kept as int8 (eae_map_regions).  WideCell: any value
// >= 0 is a label, kept and compared on all 64 bits (eae_map_regions_wide).
struct ClassCell {
  typedef signed char kept_t;
  int K;
  __device__ __forceinline__ kept_t read(long long v) const { return (kept_t)cls_of(v, K); }
};
struct WideCell {
  typedef long long kept_t;
  __device__ __forceinline__ kept_t read(long long v) const { return v >= 0 ? v : -1; }
};

// ---------------------------------------------------------------------------------------------------------------
// Union-find with union-by-minimum.  Invariant: p[i] <= i, and a stored value only ever decreases (atomic min).  The root of a set is
// therefore its smallest member.
// ---------------------------------------------------------------------------------------------------------------
template <int SCOPE>
__device__ __forceinline__ int uf_find(int* p, int x) {
  // terminates: p[x] < x unless x is a root, so x strictly decreases and is bounded by 0
  for (;;) {
    const int q = __hip_atomic_load(p + x, __ATOMIC_RELAXED, SCOPE);
    if (q == x) return x;
    x = q;
  }
}

template <int SCOPE>
__device__ __forceinline__ void uf_union(int* p, int a, int b) {
  // terminates: a pass that does not return replaces a by the value p[a] held, which is < a (a was no root any more), and find only
  // lowers a and b: a + b strictly decreases, bounded by 0.  The link a -> old that the min may have overwritten is not lost: the
  // loop goes on to unite old with b.
  for (;;) {
    a = uf_find<SCOPE>(p, a);
    b = uf_find<SCOPE>(p, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = __hip_atomic_fetch_min(p + a, b, __ATOMIC_RELAXED, SCOPE);
    if (old == a) return;
    a = old;
  }
}

// regions, first kernel: one 32 x 32 tile per workgroup.  Thread (lx, lyb) owns the cells (lx, lyb + 8 i), i < 4.  Cells outside
// the map and unclassified cells carry class -1 and are never united.  parent[cell] = the global linear index of the cell's root in
// the tile (the tile's smallest member of the set: row-major order is the same in the tile and in the map), -1 for an unclassified cell.
template <typename Cell>
__global__ __launch_bounds__(RG_NT) void regions_tile_kernel(const long long* __restrict__ labels, int H, int W, Cell cell, int conn8,
                                                              int tilesX, int* __restrict__ parent) {
  typedef typename Cell::kept_t kept_t;
  __shared__ int lp[RG_CELLS];
  __shared__ kept_t cl[RG_CELLS];
  const int tile = blockIdx.x, ty0 = (tile / tilesX) * RG_T, tx0 = (tile % tilesX) * RG_T;
  const int tid = threadIdx.x, lx = tid & (RG_T - 1), lyb = tid >> 5;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int ly = lyb + 8 * i, li = ly * RG_T + lx, y = ty0 + ly, x = tx0 + lx;
    kept_t c = -1;
    if (y < H && x < W) c = cell.read(labels[(size_t)y * W + x]);
    cl[li] = c;
    lp[li] = li;
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int ly = lyb + 8 * i, li = ly * RG_T + lx;
    const kept_t c = cl[li];
    if (c < 0) continue;
    if (lx > 0 && cl[li - 1] == c) uf_union<__HIP_MEMORY_SCOPE_WORKGROUP>(lp, li, li - 1);
    if (ly > 0) {
      if (cl[li - RG_T] == c) uf_union<__HIP_MEMORY_SCOPE_WORKGROUP>(lp, li, li - RG_T);
      if (conn8) {
        if (lx > 0 && cl[li - RG_T - 1] == c) uf_union<__HIP_MEMORY_SCOPE_WORKGROUP>(lp, li, li - RG_T - 1);
        if (lx < RG_T - 1 && cl[li - RG_T + 1] == c) uf_union<__HIP_MEMORY_SCOPE_WORKGROUP>(lp, li, li - RG_T + 1);
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int ly = lyb + 8 * i, li = ly * RG_T + lx, y = ty0 + ly, x = tx0 + lx;
    if (y >= H || x >= W) continue;
    int r = -1;
    if (cl[li] >= 0) {
      const int root = uf_find<__HIP_MEMORY_SCOPE_WORKGROUP>(lp, li);
      r = (int)((long long)(ty0 + (root >> 5)) * W + tx0 + (root & (RG_T - 1)));
    }
    parent[(size_t)y * W + x] = r;
  }
}

// regions, second kernel: one thread per cell of a tile border.  Jobs [0, nh): the cells of the rows y = 32, 64, ... (the first row
// of a tile), united with their neighbours in the row above; jobs [nh, nh + nv): the cells of the columns x = 32, 64, ..., united with
// their neighbours in the column to the left.  With 8-connectivity the two diagonal neighbours on the far side are taken as well; a
// pair reached from both kinds of job is united twice, which changes nothing.  Every access to `parent` is a device-scope atomic:
// workgroups on different XCDs work on the same chains, and a plain load may be served by another XCD's stale L2.
template <typename Cell>
__global__ __launch_bounds__(RG_NT) void regions_merge_kernel(const long long* __restrict__ labels, int H, int W, Cell cell, int conn8,
                                                               long long nh, long long nv, int* parent) {
  long long j = (long long)blockIdx.x * RG_NT + threadIdx.x;
  long long me, o0, o1 = -1, o2 = -1;                          // the cell and its neighbours across the border; -1: none
  if (j < nh) {
    const int y = (int)(j / W + 1) * RG_T, x = (int)(j % W);
    me = (long long)y * W + x;
    o0 = me - W;
    if (conn8 && x > 0) o1 = me - W - 1;
    if (conn8 && x < W - 1) o2 = me - W + 1;
  } else if (j < nh + nv) {
    j -= nh;
    const int x = (int)(j / H + 1) * RG_T, y = (int)(j % H);
    me = (long long)y * W + x;
    o0 = me - 1;
    if (conn8 && y > 0) o1 = me - W - 1;
    if (conn8 && y < H - 1) o2 = me + W - 1;
  } else {
    return;
  }
  const typename Cell::kept_t c = cell.read(labels[me]);
  if (c < 0) return;
  if (cell.read(labels[o0]) == c) uf_union<__HIP_MEMORY_SCOPE_AGENT>(parent, (int)me, (int)o0);
  if (o1 >= 0 && cell.read(labels[o1]) == c) uf_union<__HIP_MEMORY_SCOPE_AGENT>(parent, (int)me, (int)o1);
  if (o2 >= 0 && cell.read(labels[o2]) == c) uf_union<__HIP_MEMORY_SCOPE_AGENT>(parent, (int)me, (int)o2);
}

// regions, third kernel: every cell walks to its root.  `parent` is read only here, behind a kernel boundary: plain loads.
__global__ __launch_bounds__(RG_NT) void regions_flatten_kernel(const int* __restrict__ parent, long long n,
                                                                 long long* __restrict__ regions) {
  const long long i = (long long)blockIdx.x * RG_NT + threadIdx.x;
  if (i >= n) return;
  int x = (int)i, p = parent[i];
  if (p >= 0) {
    // terminates: parent[x] < x unless x is a root, so x strictly decreases
    while (p != x) { x = p; p = parent[x]; }
  }
  regions[i] = p < 0 ? -1 : (long long)x;
}

// region_stats: a wave takes 64 consecutive cells of one row at a time.  A lane is the head of a run when its region differs from the
// lane's to its left; the head adds the run's length to area[root] and the run's extent to bbox[root], so a region that fills the
// segment costs one set of atomics instead of 64.  bbox holds (y0, x0) as unsigned minima (cleared to 0xFFFFFFFF) and (y1, x1) as
// signed maxima (cleared to -1).  A value outside [0, n) is no region.
__global__ __launch_bounds__(RG_NT) void region_stats_kernel(const long long* __restrict__ regions, int H, int W, int segs,
                                                              long long nseg, long long n, int* area, int* bbox) {
  const int lane = threadIdx.x & 63;
  const long long wave = ((long long)blockIdx.x * RG_NT + threadIdx.x) >> 6, nwaves = (long long)gridDim.x * (RG_NT / 64);
  for (long long s = wave; s < nseg; s += nwaves) {            // wave-uniform trip count: every lane reaches the ballot
    const int y = (int)(s / segs), x = (int)(s % segs) * 64 + lane;
    long long r = -2;                                          // beyond the row's end: ends the last run
    if (x < W) r = regions[(size_t)y * W + x];
    const long long left = __shfl_up(r, 1, 64);
    const bool head = lane == 0 || r != left;
    const unsigned long long heads = __ballot(head);
    if (head && r >= 0 && r < n) {
      const unsigned long long rest = lane == 63 ? 0ull : heads >> (lane + 1);
      const int len = rest ? __ffsll((long long)rest) : 64 - lane;
      atomicAdd(area + r, len);
      if (bbox) {
        int* b = bbox + 4 * (size_t)r;
        atomicMin(reinterpret_cast<unsigned*>(b), (unsigned)y);
        atomicMin(reinterpret_cast<unsigned*>(b) + 1, (unsigned)x);
        atomicMax(b + 2, y);
        atomicMax(b + 3, x + len - 1);
      }
    }
  }
}

// sieve, first kernel: every cell of a small region offers its region the edge neighbours that belong to another region that is not
// small.  The slot of a small root keeps the greatest key (area << 32) | (0xFFFFFFFF - id): the largest area, then the lowest id,
// whatever the order of arrival.  The relaxed load only spares atomics: a stale value is a lower one.
__global__ __launch_bounds__(RG_NT) void sieve_vote_kernel(const long long* __restrict__ regions, const int* __restrict__ area, int H,
                                                            int W, long long n, long long min_size, unsigned long long* slot) {
  const long long i = (long long)blockIdx.x * RG_NT + threadIdx.x;
  if (i >= n) return;
  const long long r = regions[i];
  if (r < 0 || r >= n || area[r] >= min_size) return;
  const int y = (int)(i / W), x = (int)(i % W);
  const long long nb[4] = {y > 0 ? i - W : -1, x > 0 ? i - 1 : -1, x < W - 1 ? i + 1 : -1, y < H - 1 ? i + W : -1};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (nb[k] < 0) continue;
    const long long q = regions[nb[k]];
    if (q < 0 || q >= n || q == r) continue;
    const int aq = area[q];
    if (aq < min_size) continue;
    const unsigned long long key = ((unsigned long long)(unsigned)aq << 32) | (0xFFFFFFFFu - (unsigned)q);
    if (__hip_atomic_load(slot + r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < key) atomicMax(slot + r, key);
  }
}

// sieve, second kernel: a cell of a small region whose slot was set takes the class stored at the winner's id (a cell of the winner);
// every other cell is copied as stored.
__global__ __launch_bounds__(RG_NT) void sieve_apply_kernel(const long long* __restrict__ labels, const long long* __restrict__ regions,
                                                             const int* __restrict__ area, long long n, long long min_size,
                                                             const unsigned long long* __restrict__ slot, long long* __restrict__ out,
                                                             unsigned long long* changed) {
  const long long i = (long long)blockIdx.x * RG_NT + threadIdx.x;
  bool diff = false;
  if (i < n) {
    const long long v = labels[i], r = regions[i];
    long long o = v;
    if (r >= 0 && r < n && area[r] < min_size) {
      const unsigned long long key = slot[r];
      if (key) o = labels[0xFFFFFFFFu - (unsigned)key];
    }
    out[i] = o;
    diff = o != v;
  }
  if (changed) {
    const unsigned long long m = __ballot(diff);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(changed, (unsigned long long)__popcll(m));
  }
}

// majority: one 32 x 32 tile of outputs per workgroup, the tile and its halo of r cells as int8 classes in LDS (-1: unclassified or
// outside the map, which is what clips the window).  Per output cell: the classes present in the window as a 64-bit mask, then one
// counting pass per present class in ascending order (strict > keeps the lowest id), the centre's own count kept on the way.
__global__ __launch_bounds__(RG_NT) void map_majority_kernel(const long long* __restrict__ in, int H, int W, int K, int r, int fill,
                                                              int tilesX, long long* __restrict__ out) {
  __shared__ signed char t[MJ_SIDE * MJ_LD];
  const int tile = blockIdx.x, ty0 = (tile / tilesX) * RG_T, tx0 = (tile % tilesX) * RG_T;
  const int tid = threadIdx.x, lx = tid & (RG_T - 1), lyb = tid >> 5;
  const int side = RG_T + 2 * r, d = 2 * r + 1;
  for (int idx = tid; idx < side * side; idx += RG_NT) {
    const int ly = idx / side, lxx = idx - ly * side, y = ty0 - r + ly, x = tx0 - r + lxx;
    int c = -1;
    if (y >= 0 && y < H && x >= 0 && x < W) c = cls_of(in[(size_t)y * W + x], K);
    t[ly * MJ_LD + lxx] = (signed char)c;
  }
  __syncthreads();
  for (int i = 0; i < 4; ++i) {
    const int ly = lyb + 8 * i, y = ty0 + ly, x = tx0 + lx;
    if (y >= H || x >= W) continue;
    const signed char* w0 = t + ly * MJ_LD + lx;               // the window's first cell: rows ly .. ly + 2r of the staged tile
    const int centre = w0[r * MJ_LD + r];
    unsigned long long present = 0;
    for (int dy = 0; dy < d; ++dy)
      for (int dx = 0; dx < d; ++dx) {
        const int c = w0[dy * MJ_LD + dx];
        if (c >= 0) present |= 1ull << c;
      }
    long long o;
    if (!present || (centre < 0 && !fill)) {
      o = in[(size_t)y * W + x];                               // as stored, whatever value that is
    } else {
      int best = -1, bestn = 0, cn = 0;
      // terminates: every pass clears the lowest set bit of m
      for (unsigned long long m = present; m; m &= m - 1) {
        const int k = __ffsll((long long)m) - 1;
        int cnt = 0;
        for (int dy = 0; dy < d; ++dy)
          for (int dx = 0; dx < d; ++dx) cnt += w0[dy * MJ_LD + dx] == k;
        if (cnt > bestn) { bestn = cnt; best = k; }
        if (k == centre) cn = cnt;
      }
      if (centre >= 0 && cn == bestn) best = centre;
      o = best;
    }
    out[(size_t)y * W + x] = o;
  }
}

const char* map_dims_msg = "map: H and W must be >= 1 and H * W < 2^31";
int map_dims_ok(int H, int W) { return H >= 1 && W >= 1 && (long long)H * W < (1LL << 31); }
unsigned cell_blocks(long long n) { return (unsigned)((n + RG_NT - 1) / RG_NT); }

}  // namespace

extern "C" long long eae_map_workspace_bytes(int H, int W) {
  if (!map_dims_ok(H, W)) return eae_set_error(EAE_ERR_ARG, map_dims_msg);
  return (long long)H * W * 8;              // int32 parents (regions) or 64-bit slots (sieve_pass): the larger of the two
}

extern "C" int eae_map_majority(void* stream, const long long* in, int H, int W, int K, int radius, int fill, long long* out) {
  if (!map_dims_ok(H, W)) return eae_set_error(EAE_ERR_ARG, map_dims_msg);
  if (!in || !out || in == out) return eae_set_error(EAE_ERR_ARG, "map_majority: NULL in or out, or in == out");
  if (K < 1 || K > 64) return eae_set_error(EAE_ERR_ARG, "map_majority: the number of classes must be in 1..64");
  if (radius < 1 || radius > MJ_RMAX) return eae_set_error(EAE_ERR_ARG, "map_majority: the radius must be in 1..7");
  EAE_NO_GROUP("map_majority_kernel");
  const int tilesX = (W + RG_T - 1) / RG_T, tilesY = (H + RG_T - 1) / RG_T;
  hipLaunchKernelGGL(map_majority_kernel, dim3((unsigned)((long long)tilesX * tilesY)), dim3(RG_NT), 0, (hipStream_t)stream, in, H, W, K,
                     radius, fill != 0, tilesX, out);
  EAE_LAUNCH_CHECK();
  return 0;
}

namespace {

// the three launches of a region labelling, for either kind of cell; `who` names the call in the messages
template <typename Cell>
int map_regions_run(const char* who, void* stream, const long long* labels, int H, int W, Cell cell, int connectivity, long long* regions,
                    void* workspace, long long workspace_bytes) {
  static thread_local char msg[160];
  const char* what = nullptr;
  if (!labels || !regions) what = "NULL labels or regions";
  else if (connectivity != 4 && connectivity != 8) what = "the connectivity must be 4 or 8";
  else if (!workspace || workspace_bytes < (long long)H * W * 8) what = "the workspace is NULL or smaller than eae_map_workspace_bytes";
  if (what) {
    snprintf(msg, sizeof msg, "%s: %s", who, what);
    return eae_set_error(EAE_ERR_ARG, msg);
  }
  const long long n = (long long)H * W;
  EAE_NO_GROUP("regions_tile_kernel");
  const hipStream_t st = (hipStream_t)stream;
  int* parent = (int*)workspace;
  const int conn8 = connectivity == 8;
  const int tilesX = (W + RG_T - 1) / RG_T, tilesY = (H + RG_T - 1) / RG_T;
  hipLaunchKernelGGL(regions_tile_kernel<Cell>, dim3((unsigned)((long long)tilesX * tilesY)), dim3(RG_NT), 0, st, labels, H, W, cell, conn8,
                     tilesX, parent);
  EAE_LAUNCH_CHECK();
  const long long nh = (long long)(tilesY - 1) * W, nv = (long long)(tilesX - 1) * H;
  if (nh + nv > 0) {
    hipLaunchKernelGGL(regions_merge_kernel<Cell>, dim3(cell_blocks(nh + nv)), dim3(RG_NT), 0, st, labels, H, W, cell, conn8, nh, nv,
                       parent);
    EAE_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(regions_flatten_kernel, dim3(cell_blocks(n)), dim3(RG_NT), 0, st, (const int*)parent, n, regions);
  EAE_LAUNCH_CHECK();
  return 0;
}

}  // namespace

extern "C" int eae_map_regions(void* stream, const long long* labels, int H, int W, int K, int connectivity, long long* regions,
                               void* workspace, long long workspace_bytes) {
  if (!map_dims_ok(H, W)) return eae_set_error(EAE_ERR_ARG, map_dims_msg);
  if (K < 1 || K > 64) return eae_set_error(EAE_ERR_ARG, "map_regions: the number of classes must be in 1..64");
  return map_regions_run("map_regions", stream, labels, H, W, ClassCell{K}, connectivity, regions, workspace, workspace_bytes);
}

extern "C" int eae_map_regions_wide(void* stream, const long long* labels, int H, int W, int connectivity, long long* regions,
                                    void* workspace, long long workspace_bytes) {
  if (!map_dims_ok(H, W)) return eae_set_error(EAE_ERR_ARG, map_dims_msg);
  return map_regions_run("map_regions_wide", stream, labels, H, W, WideCell{}, connectivity, regions, workspace, workspace_bytes);
}

extern "C" int eae_map_region_stats(void* stream, const long long* regions, int H, int W, int* area, int* bbox) {
  if (!map_dims_ok(H, W)) return eae_set_error(EAE_ERR_ARG, map_dims_msg);
  if (!regions || !area) return eae_set_error(EAE_ERR_ARG, "map_region_stats: NULL regions or area");
  EAE_NO_GROUP("region_stats_kernel");
  const hipStream_t st = (hipStream_t)stream;
  const long long n = (long long)H * W;
  if (hipMemsetAsync(area, 0, (size_t)n * sizeof(int), st) != hipSuccess ||
      (bbox && hipMemsetAsync(bbox, 0xFF, (size_t)n * 4 * sizeof(int), st) != hipSuccess))
    return eae_set_error(EAE_ERR_HIP, "map_region_stats: clearing area or bbox failed");
  const int segs = (W + 63) / 64;
  const long long nseg = (long long)H * segs, blocks = (nseg + RG_NT / 64 - 1) / (RG_NT / 64);
  // bounded grid (16 workgroups on each of 256 CUs), the waves striding over the segments
  hipLaunchKernelGGL(region_stats_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(RG_NT), 0, st, regions, H, W, segs, nseg,
                     n, area, bbox);
  EAE_LAUNCH_CHECK();
  return 0;
}

extern "C" int eae_map_sieve_pass(void* stream, const long long* labels, const long long* regions, const int* area, int H, int W,
                                  long long min_size, long long* out, long long* changed, void* workspace, long long workspace_bytes) {
  if (!map_dims_ok(H, W)) return eae_set_error(EAE_ERR_ARG, map_dims_msg);
  if (!labels || !regions || !area || !out || out == labels)
    return eae_set_error(EAE_ERR_ARG, "map_sieve_pass: NULL labels, regions, area or out, or out == labels");
  if (min_size < 1) return eae_set_error(EAE_ERR_ARG, "map_sieve_pass: min_size must be >= 1");
  const long long n = (long long)H * W;
  if (!workspace || workspace_bytes < n * 8)
    return eae_set_error(EAE_ERR_ARG, "map_sieve_pass: the workspace is NULL or smaller than eae_map_workspace_bytes");
  EAE_NO_GROUP("sieve_vote_kernel");
  const hipStream_t st = (hipStream_t)stream;
  unsigned long long* slot = (unsigned long long*)workspace;
  if (hipMemsetAsync(slot, 0, (size_t)n * 8, st) != hipSuccess || (changed && hipMemsetAsync(changed, 0, sizeof(long long), st) != hipSuccess))
    return eae_set_error(EAE_ERR_HIP, "map_sieve_pass: clearing the slots or the changed counter failed");
  hipLaunchKernelGGL(sieve_vote_kernel, dim3(cell_blocks(n)), dim3(RG_NT), 0, st, regions, area, H, W, n, min_size, slot);
  EAE_LAUNCH_CHECK();
  hipLaunchKernelGGL(sieve_apply_kernel, dim3(cell_blocks(n)), dim3(RG_NT), 0, st, labels, regions, area, n, min_size,
                     (const unsigned long long*)slot, out, (unsigned long long*)changed);
  EAE_LAUNCH_CHECK();
  return 0;
}
