// ccl.hip -- row f1 of SURVEY.md section 8: 26-connected multi-label connected components on the GPU.
//
// Replaces cc3d.connected_components as called at kimimaro/utility.py:74-77 (third-party, source absent)
// together with fastremap.renumber/refit (utility.py:71,79): two voxels are in the same component iff they
// are joined by a 26-connected chain of voxels with the same non-zero label.  Components are numbered
// 1..N in order of first appearance in the Fortran-order raster (= increasing minimum linear index), the
// numbering the host helper kh_host_ccl26 produces.
//
// Lock-free union-find (every parent pointer points to a SMALLER index, so the root of a set is its
// minimum element, stale reads are harmless and no cycle can form):
//   init     parent[i] = first voxel of i's x run inside its 64-lane chunk (foreground) / NONE (background)
//   link     the unions with the 13 already-rastered same-label neighbours that the labels do not show to be redundant
//            (atomicCAS on roots)
//   flatten  parent[i] = root(i)
//   number   roots are counted per 1024-voxel chunk, the chunk counts are scanned, every root gets
//            id = 1 + (number of roots before it), every voxel copies its root's id.
// HBM-bound sweeps (lanes along x); the link pass is the only irregular one.
#include "common.h"

namespace kh {

static constexpr uint32_t CCL_NONE = 0xFFFFFFFFu;

// init: lanes along x.  A voxel starts as a child of the first voxel of its x run INSIDE its 64-lane chunk (one ballot per chunk:
// no atomics, and the "link with the left neighbour" union of rounds 1-4 disappears for 63 voxels in 64); a run that continues
// over a chunk boundary is joined there by one union in the link pass.  Pointers still point to smaller (or equal) indices.
template <typename LT>
__global__ __launch_bounds__(256) void ccl_init_kernel(const LT* __restrict__ lab, uint32_t* __restrict__ parent, int sx, int64_t nrows) {
  const int xt = (sx + 255) >> 8;
  const int64_t ntiles = (int64_t)xt * nrows;
  const int lane = threadIdx.x & 63;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int x = (int)(t % xt) * 256 + threadIdx.x;
    const int64_t i = x + (int64_t)sx * (t / xt);
    const LT L = x < sx ? lab[i] : (LT)0;
    LT Lm = (LT)__shfl_up((unsigned long long)L, 1);
    const bool start = L != 0 && (lane == 0 || Lm != L);
    const unsigned long long m = __builtin_amdgcn_ballot_w64(start) & ((lane == 63) ? ~0ull : ((2ull << lane) - 1ull));
    if (x < sx) parent[i] = L != 0 ? (uint32_t)(i - (lane - (63 - __clzll((long long)m)))) : CCL_NONE;
  }
}

__device__ __forceinline__ uint32_t ccl_ld(uint32_t* parent, uint32_t i) {
  return __hip_atomic_load(&parent[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint32_t ccl_find(uint32_t* parent, uint32_t i) {
  uint32_t p = ccl_ld(parent, i);
  while (p != i) {
    const uint32_t gp = ccl_ld(parent, p);
    if (gp != p) __hip_atomic_store(&parent[i], gp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // path halving
    i = p;
    p = gp;
  }
  return i;
}
__device__ __forceinline__ void ccl_union(uint32_t* parent, uint32_t a, uint32_t b) {
  for (;;) {
    a = ccl_find(parent, a);
    b = ccl_find(parent, b);
    if (a == b) return;
    if (a < b) { const uint32_t t = a; a = b; b = t; }  // a > b: the larger root hangs under the smaller
    const uint32_t old = atomicCAS(&parent[a], a, b);
    if (old == a) return;
    a = old;
  }
}

// link: the 13 neighbours that precede a voxel in the raster lie in its own row (x - 1) and in four earlier rows
// (dy, dz) = (-1, 0), (-1, -1), (0, -1), (+1, -1) at x - 1, x, x + 1.  Most of those unions would find the two voxels in one set
// already -- two root searches and, in rounds 1-4, a compare-and-swap each (34.7 GB of traffic for 3.7 GB of labels).  They
// are skipped by looking at the labels first (a look before the atomic):
//   * its own row: the x runs are pre-linked by ccl_init_kernel inside every 64-lane chunk; only a run that crosses a chunk
//     boundary needs a union, at the chunk's first voxel;
//   * an earlier row r', for the FIRST voxel of a run: the voxel above it (x, r') if it has the label -- (x - 1, r') and
//     (x + 1, r') are then in the same run of r' --, else (x - 1, r') and (x + 1, r');
//   * an earlier row r', for any other voxel of a run: only (x + 1, r'), and only when (x, r') does NOT have the label -- else
//     (x + 1, r') belongs to a run of r' that an earlier voxel of this run has linked already.
// Every pair of adjacent runs still gets a link: take the leftmost voxel of this run that touches the run of r'; it is either
// the first voxel of this run (first rule) or sits one to the left of that run's start (second rule).
template <typename LT>
__global__ __launch_bounds__(256) void ccl_link_kernel(const LT* __restrict__ lab, uint32_t* parent, int sx, int sy, int sz) {
  const int xt = (sx + 255) >> 8;
  const int64_t ntiles = (int64_t)xt * sy * sz;
  const int64_t sxy = (int64_t)sx * sy;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int x = (int)(t % xt) * 256 + threadIdx.x;
    const int64_t r = t / xt;
    const int y = (int)(r % sy), z = (int)(r / sy);
    if (x >= sx) continue;
    const int64_t i = x + (int64_t)sx * y + sxy * z;
    const LT L = lab[i];
    if (L == 0) continue;
    const bool left = x > 0 && lab[i - 1] == L;
    if (left && (x & 63) == 0) ccl_union(parent, (uint32_t)i, (uint32_t)(i - 1));
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const int dy = k == 2 ? 0 : (k == 3 ? 1 : -1);
      const int dz = k == 0 ? 0 : -1;
      const int ny = y + dy, nz = z + dz;
      if (ny < 0 || ny >= sy || nz < 0) continue;
      const int64_t j = i + (int64_t)sx * dy + sxy * dz;
      const bool b = lab[j] == L;
      const bool c = x + 1 < sx && lab[j + 1] == L;
      if (left) {
        if (c && !b) ccl_union(parent, (uint32_t)i, (uint32_t)(j + 1));
      } else if (b) {
        ccl_union(parent, (uint32_t)i, (uint32_t)j);
      } else {
        if (x > 0 && lab[j - 1] == L) ccl_union(parent, (uint32_t)i, (uint32_t)(j - 1));
        if (c) ccl_union(parent, (uint32_t)i, (uint32_t)(j + 1));
      }
    }
  }
}

__global__ __launch_bounds__(256) void ccl_flatten_count_kernel(uint32_t* parent, int64_t n, uint32_t* chunk_counts) {
  // one chunk = 1024 voxels = 4 per thread; also counts the roots of the chunk
  __shared__ uint32_t cnt;
  const int64_t nchunks = (n + 1023) / 1024;
  for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
    if (threadIdx.x == 0) cnt = 0;
    __syncthreads();
    uint32_t mine = 0;
    for (int k = 0; k < 4; k++) {
      const int64_t i = c * 1024 + k * 256 + threadIdx.x;
      if (i < n) {
        const uint32_t p = parent[i];
        if (p != CCL_NONE) {
          const uint32_t r = ccl_find(parent, (uint32_t)i);
          parent[i] = r;
          mine += (r == (uint32_t)i);
        }
      }
    }
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(&cnt, mine);
    __syncthreads();
    if (threadIdx.x == 0) chunk_counts[c] = cnt;
    __syncthreads();
  }
}

// exclusive scan of chunk_counts (in place) by ONE workgroup; total -> *total
__global__ __launch_bounds__(1024) void ccl_scan_kernel(uint32_t* counts, int64_t nchunks, uint32_t* total) {
  __shared__ uint32_t wsum[16];
  __shared__ uint32_t carry;
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t b = 0; b < nchunks; b += 1024) {
    const int64_t i = b + threadIdx.x;
    const uint32_t v = i < nchunks ? counts[i] : 0u;
    uint32_t s = v;  // inclusive scan inside the wave
    for (int o = 1; o < 64; o <<= 1) { const uint32_t t = __shfl_up(s, o); if (lane >= o) s += t; }
    if (lane == 63) wsum[wave] = s;
    __syncthreads();
    uint32_t base = carry;
    for (int w = 0; w < wave; w++) base += wsum[w];
    if (i < nchunks) counts[i] = base + s - v;
    __syncthreads();
    if (threadIdx.x == 1023) carry = base + s;
    __syncthreads();
  }
  if (threadIdx.x == 0) *total = carry;
}

__global__ __launch_bounds__(256) void ccl_number_roots_kernel(const uint32_t* __restrict__ parent, int64_t n,
                                                               const uint32_t* __restrict__ chunk_base,
                                                               uint32_t* __restrict__ out, uint32_t* __restrict__ rep) {
  // ids of the roots of a chunk, in index order: chunk_base + rank inside the chunk + 1
  __shared__ uint32_t wbase[4];
  const int64_t nchunks = (n + 1023) / 1024;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
    uint32_t running = chunk_base[c];
    for (int k = 0; k < 4; k++) {  // index order: k-th quarter, then thread
      const int64_t i = c * 1024 + k * 256 + threadIdx.x;
      const bool root = i < n && parent[i] == (uint32_t)i;
      const unsigned long long m = __ballot(root);
      if (lane == 0) wbase[wave] = (uint32_t)__popcll(m);
      __syncthreads();
      uint32_t before = running;
      for (int w = 0; w < wave; w++) before += wbase[w];
      const uint32_t tot = wbase[0] + wbase[1] + wbase[2] + wbase[3];
      if (root) {
        const uint32_t id = before + (uint32_t)__popcll(m & ((1ull << lane) - 1ull)) + 1u;
        out[i] = id;
        rep[id] = (uint32_t)i;
      }
      running += tot;
      __syncthreads();
    }
  }
}

__global__ __launch_bounds__(256) void ccl_relabel_kernel(uint32_t* parent, int64_t n, uint32_t* out, uint16_t* out16,
                                                          const uint32_t* __restrict__ total) {
  // out16: the ids once more as u16 when there are fewer than 65536 components (fastremap.refit, kimimaro/utility.py:79):
  // every later sweep over the component volume then reads 2 instead of 4 bytes per voxel
  const bool narrow = out16 != nullptr && *total < 65536u;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const uint32_t p = ccl_ld(parent, (uint32_t)i);
    if (p == CCL_NONE) { out[i] = 0; if (narrow) out16[i] = 0; continue; }
    if (p == (uint32_t)i) { if (narrow) out16[i] = (uint16_t)out[i]; continue; }   // roots were numbered by ccl_number_roots_kernel
    // parent[i] is an ancestor but not necessarily the root: a path-halving store of another thread's find may have
    // landed after the flatten pass wrote the root (seen on a 10^6-voxel component: a few voxels kept label 0)
    const uint32_t id = out[ccl_find(parent, (uint32_t)i)];
    out[i] = id;
    if (narrow) out16[i] = (uint16_t)id;
  }
}

static inline unsigned ccl_grid(int64_t n, int per_block, int64_t cap = 16384) {
  int64_t g = (n + per_block - 1) / per_block;
  if (g > cap) g = cap;
  if (g < 1) g = 1;
  return (unsigned)g;
}

template <typename LT>
static int ccl_impl(const LT* lab, int64_t sx, int64_t sy, int64_t sz, uint32_t* parent, uint32_t* chunk_counts, uint32_t* out,
                    uint32_t* rep, uint32_t* total, uint16_t* out16, hipStream_t st) {
  const int64_t n = sx * sy * sz;
  const int64_t nchunks = (n + 1023) / 1024;
  const int64_t ntiles = ((sx + 255) / 256) * sy * sz;
  hipLaunchKernelGGL((ccl_init_kernel<LT>), dim3(ccl_grid(ntiles, 1, 1 << 20)), dim3(256), 0, st, lab, parent, (int)sx, sy * sz);
  hipLaunchKernelGGL((ccl_link_kernel<LT>), dim3(ccl_grid(ntiles, 1, 1 << 20)), dim3(256), 0, st, lab, parent, (int)sx, (int)sy, (int)sz);
  hipLaunchKernelGGL(ccl_flatten_count_kernel, dim3(ccl_grid(nchunks, 1)), dim3(256), 0, st, parent, n, chunk_counts);
  hipLaunchKernelGGL(ccl_scan_kernel, dim3(1), dim3(1024), 0, st, chunk_counts, nchunks, total);
  hipLaunchKernelGGL(ccl_number_roots_kernel, dim3(ccl_grid(nchunks, 1)), dim3(256), 0, st, parent, n, chunk_counts, out, rep);
  hipLaunchKernelGGL(ccl_relabel_kernel, dim3(ccl_grid(n, 256)), dim3(256), 0, st, parent, n, out, out16, total);
  KH_LAUNCH_CHECK();
  return KH_OK;
}

// ------------------------------------------------------------------------------------------------
// Components of a voxel connectivity graph (cc3d.color_connectivity_graph(voxel_graph, connectivity=26) followed by
// `cc_labels *= all_labels > 0`, kimimaro/utility.py:73-75; cc3d's source is absent: PARITY UNPINNED).  Two foreground voxels are
// joined iff they are 26-neighbours and the graph word of the LATER one in the raster allows the step back to the earlier one
// (cc3d reads the graph while it rasters; its own graphs are symmetric, so either reading gives the same sets).  Same union-find,
// numbering and outputs as kh_ccl26.
// Also unpinned: two foreground voxels are never linked THROUGH background voxels here, while color_connectivity_graph(graph)
// works on the graph alone and `* (labels > 0)` only masks its result afterwards -- two foreground islands that the graph joins by
// way of background voxels would share an id there and get two here.
// A component of the graph may hold several labels; the host names it by the label at its last run start in the raster
// (skeletontricks.get_mapping, kimimaro/utility.py:82), not by the representative voxel `rep` reports.
template <typename LT>
__global__ __launch_bounds__(256) void cclg_init_kernel(const LT* __restrict__ lab, uint32_t* __restrict__ parent, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    parent[i] = lab[i] != 0 ? (uint32_t)i : CCL_NONE;
}
template <typename LT>
__global__ __launch_bounds__(256) void cclg_link_kernel(const LT* __restrict__ lab, const uint32_t* __restrict__ graph, uint32_t* parent,
                                                        int sx, int sy, int sz) {
  const int xt = (sx + 255) >> 8;
  const int64_t ntiles = (int64_t)xt * sy * sz;
  const int64_t sxy = (int64_t)sx * sy;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int x = (int)(t % xt) * 256 + threadIdx.x;
    const int64_t r = t / xt;
    const int y = (int)(r % sy), z = (int)(r / sy);
    if (x >= sx) continue;
    const int64_t i = x + (int64_t)sx * y + sxy * z;
    if (lab[i] == 0) continue;
    const uint32_t dirs = graph_to_directions(graph[i]);
#pragma unroll
    for (int k = 0; k < 26; k++) {
      int dx = 0, dy = 0, dz = 0;
      dir_delta(k, dx, dy, dz);
      if (!(dz < 0 || (dz == 0 && (dy < 0 || (dy == 0 && dx < 0))))) continue;     // the 13 neighbours earlier in the raster
      if (!((dirs >> k) & 1u)) continue;
      const int nx = x + dx, ny = y + dy, nz = z + dz;
      if (nx < 0 || nx >= sx || ny < 0 || ny >= sy || nz < 0) continue;
      const int64_t j = i + dx + (int64_t)sx * dy + sxy * dz;
      if (lab[j] != 0) ccl_union(parent, (uint32_t)i, (uint32_t)j);
    }
  }
}
template <typename LT>
static int cclg_impl(const LT* lab, const uint32_t* graph, int64_t sx, int64_t sy, int64_t sz, uint32_t* parent, uint32_t* chunk_counts,
                     uint32_t* out, uint32_t* rep, uint32_t* total, uint16_t* out16, hipStream_t st) {
  const int64_t n = sx * sy * sz;
  const int64_t nchunks = (n + 1023) / 1024;
  const int64_t ntiles = ((sx + 255) / 256) * sy * sz;
  hipLaunchKernelGGL((cclg_init_kernel<LT>), dim3(ccl_grid(n, 256)), dim3(256), 0, st, lab, parent, n);
  hipLaunchKernelGGL((cclg_link_kernel<LT>), dim3(ccl_grid(ntiles, 1, 1 << 20)), dim3(256), 0, st, lab, graph, parent, (int)sx, (int)sy, (int)sz);
  hipLaunchKernelGGL(ccl_flatten_count_kernel, dim3(ccl_grid(nchunks, 1)), dim3(256), 0, st, parent, n, chunk_counts);
  hipLaunchKernelGGL(ccl_scan_kernel, dim3(1), dim3(1024), 0, st, chunk_counts, nchunks, total);
  hipLaunchKernelGGL(ccl_number_roots_kernel, dim3(ccl_grid(nchunks, 1)), dim3(256), 0, st, parent, n, chunk_counts, out, rep);
  hipLaunchKernelGGL(ccl_relabel_kernel, dim3(ccl_grid(n, 256)), dim3(256), 0, st, parent, n, out, out16, total);
  KH_LAUNCH_CHECK();
  return KH_OK;
}

// edt.edt(labels, voxel_graph=) (kimimaro/intake.py:174-183; the `edt` package is absent: PARITY UNPINNED).  The package's
// published method: the image is doubled along every axis, a voxel (x, y, z) sits at cell (2x, 2y, 2z), the cell between it and
// its +x / +y / +z neighbour is foreground iff the voxel is and its graph word allows that step (bits 0 / 2 / 4 of cc3d's
// layout), the other cells of its 2 x 2 x 2 block follow the voxel itself; a binary transform of the cells with HALF the voxel
// pitch is sampled at the voxel cells.  A wall between two voxels thus lies half a pitch from either.  Without a black border
// the cells behind the last voxel of an axis follow the voxel (no wall at the array's end, like at its start).
template <typename LT>
__global__ __launch_bounds__(256) void edt_graph_cells_kernel(const LT* __restrict__ lab, const uint32_t* __restrict__ graph, int sx, int sy,
                                                              int sz, int black_border, uint8_t* __restrict__ cells) {
  const int64_t n = (int64_t)sx * sy * sz;
  const int64_t sx2 = 2 * (int64_t)sx, sxy2 = sx2 * 2 * sy;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int x = (int)(i % sx), y = (int)((i / sx) % sy), z = (int)(i / ((int64_t)sx * sy));
    const uint8_t fg = lab[i] != 0 ? 1 : 0;
    const uint32_t gw = graph[i];
    const bool ex = !black_border && x == sx - 1, ey = !black_border && y == sy - 1, ez = !black_border && z == sz - 1;
    const uint8_t px = (uint8_t)(fg & (ex ? 1u : (gw & 1u)));
    const uint8_t py = (uint8_t)(fg & (ey ? 1u : ((gw >> 2) & 1u)));
    const uint8_t pz = (uint8_t)(fg & (ez ? 1u : ((gw >> 4) & 1u)));
    uint8_t* c = cells + 2 * x + sx2 * (2 * (int64_t)y) + sxy2 * (2 * (int64_t)z);
    *reinterpret_cast<uint16_t*>(c) = (uint16_t)(fg | (px << 8));
    *reinterpret_cast<uint16_t*>(c + sx2) = (uint16_t)(py | (fg << 8));
    *reinterpret_cast<uint16_t*>(c + sxy2) = (uint16_t)(pz | (fg << 8));
    *reinterpret_cast<uint16_t*>(c + sxy2 + sx2) = (uint16_t)(fg | (fg << 8));
  }
}
__global__ __launch_bounds__(256) void edt_graph_sample_kernel(const float* __restrict__ fine, int sx, int sy, int sz, float* __restrict__ out) {
  const int64_t n = (int64_t)sx * sy * sz;
  const int64_t sx2 = 2 * (int64_t)sx, sxy2 = sx2 * 2 * sy;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int x = (int)(i % sx), y = (int)((i / sx) % sy), z = (int)(i / ((int64_t)sx * sy));
    out[i] = fine[2 * x + sx2 * (2 * (int64_t)y) + sxy2 * (2 * (int64_t)z)];
  }
}

// ------------------------------------------------------------------------------------------------
// Row f3: binary hole filling (fill_voids.fill as called at kimimaro/trace.py:109 -- third-party, source absent;
// restated as "every background voxel that has no 6-connected background path to the border of the array
// becomes foreground", the definition scipy.ndimage.binary_fill_holes shares).  Same union-find as above on
// the background voxels with the 3 already-rastered face neighbours, then every set that owns a voxel on a
// face of the array is marked open, and the closed ones are filled.
__global__ __launch_bounds__(256) void fill_init_kernel(const uint8_t* __restrict__ mask, uint32_t* __restrict__ parent,
                                                        uint8_t* __restrict__ open, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    parent[i] = mask[i] == 0 ? (uint32_t)i : CCL_NONE;
    open[i] = 0;
  }
}

__global__ __launch_bounds__(256) void fill_link_kernel(const uint8_t* __restrict__ mask, uint32_t* parent, int sx, int sy, int sz) {
  const int xt = (sx + 255) >> 8;
  const int64_t ntiles = (int64_t)xt * sy * sz;
  const int64_t sxy = (int64_t)sx * sy;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int x = (int)(t % xt) * 256 + threadIdx.x;
    const int64_t r = t / xt;
    const int y = (int)(r % sy), z = (int)(r / sy);
    if (x >= sx) continue;
    const int64_t i = x + (int64_t)sx * y + sxy * z;
    if (mask[i] != 0) continue;
    if (x > 0 && mask[i - 1] == 0) ccl_union(parent, (uint32_t)i, (uint32_t)(i - 1));
    if (y > 0 && mask[i - sx] == 0) ccl_union(parent, (uint32_t)i, (uint32_t)(i - sx));
    if (z > 0 && mask[i - sxy] == 0) ccl_union(parent, (uint32_t)i, (uint32_t)(i - sxy));
  }
}

// ndim: dimensionality of the caller's array -- an axis beyond it (extent 1) is not an axis and has no faces: a 2-D image's border
// is its outline (fill_voids.fill on the six faces of a crop, kimimaro/intake.py:655-666)
__global__ __launch_bounds__(256) void fill_mark_open_kernel(uint32_t* parent, uint8_t* open, int sx, int sy, int sz, int ndim) {
  const int64_t sxy = (int64_t)sx * sy, n = sxy * sz;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int64_t z = i / sxy, r = i - z * sxy, y = r / sx, x = r - y * sx;
    const bool face = x == 0 || x == sx - 1 || (ndim >= 2 && (y == 0 || y == sy - 1)) || (ndim >= 3 && (z == 0 || z == sz - 1));
    if (face && parent[i] != CCL_NONE) open[ccl_find(parent, (uint32_t)i)] = 1;
  }
}

__global__ __launch_bounds__(256) void fill_apply_kernel(const uint8_t* __restrict__ mask, uint32_t* parent,
                                                         const uint8_t* __restrict__ open, uint8_t* __restrict__ out, int64_t n,
                                                         unsigned long long* filled) {
  unsigned long long mine = 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    uint8_t v = mask[i] != 0;
    if (!v && !open[ccl_find(parent, (uint32_t)i)]) { v = 1; mine++; }
    out[i] = v;
  }
  for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o);
  if ((threadIdx.x & 63) == 0 && mine) atomicAdd(filled, mine);
}

}  // namespace kh

extern "C" int kh_ccl26(const void* labels, int label_bytes, int64_t sx, int64_t sy, int64_t sz, uint32_t* parent,
                        uint32_t* chunk_counts, uint32_t* out, uint32_t* representative, uint32_t* ncomponents, uint16_t* out16,
                        void* stream) {
  if (int rc = kh::require_device()) return rc;
  if (!labels || !parent || !chunk_counts || !out || !representative || !ncomponents || sx <= 0 || sy <= 0 || sz <= 0 ||
      sx * sy * sz >= (1ll << 32) - 1) {
    kh::set_error("kh_ccl26: bad arguments (null pointer, empty volume or >= 2^32-1 voxels)");
    return KH_EINVAL;
  }
  hipStream_t st = (hipStream_t)stream;
  switch (label_bytes) {
    case 1: return kh::ccl_impl((const uint8_t*)labels, sx, sy, sz, parent, chunk_counts, out, representative, ncomponents, out16, st);
    case 2: return kh::ccl_impl((const uint16_t*)labels, sx, sy, sz, parent, chunk_counts, out, representative, ncomponents, out16, st);
    case 4: return kh::ccl_impl((const uint32_t*)labels, sx, sy, sz, parent, chunk_counts, out, representative, ncomponents, out16, st);
    case 8: return kh::ccl_impl((const uint64_t*)labels, sx, sy, sz, parent, chunk_counts, out, representative, ncomponents, out16, st);
    default: kh::set_error("kh_ccl26: label_bytes must be 1, 2, 4 or 8"); return KH_EINVAL;
  }
}

extern "C" int kh_fill_voids(const uint8_t* mask, int64_t sx, int64_t sy, int64_t sz, uint32_t* parent, uint8_t* open,
                             uint8_t* out, int64_t* filled, void* stream) {
  return kh_fill_voids_nd(mask, 3, sx, sy, sz, parent, open, out, filled, stream);
}

extern "C" int kh_fill_voids_nd(const uint8_t* mask, int ndim, int64_t sx, int64_t sy, int64_t sz, uint32_t* parent, uint8_t* open,
                                uint8_t* out, int64_t* filled, void* stream) {
  if (int rc = kh::require_device()) return rc;
  if (!mask || !parent || !open || !out || !filled || sx <= 0 || sy <= 0 || sz <= 0 || sx * sy * sz >= (1ll << 32) - 1 ||
      ndim < 1 || ndim > 3 || (ndim < 3 && sz != 1) || (ndim < 2 && sy != 1)) {
    kh::set_error("kh_fill_voids: bad arguments (null pointer, empty volume, >= 2^32-1 voxels, or an axis beyond ndim with extent > 1)");
    return KH_EINVAL;
  }
  hipStream_t st = (hipStream_t)stream;
  const int64_t n = sx * sy * sz;
  KH_HIP_CHECK(hipMemsetAsync(filled, 0, sizeof(int64_t), st));
  hipLaunchKernelGGL(kh::fill_init_kernel, dim3(kh::ccl_grid(n, 256)), dim3(256), 0, st, mask, parent, open, n);
  const int64_t ntiles = ((sx + 255) / 256) * sy * sz;
  hipLaunchKernelGGL(kh::fill_link_kernel, dim3(kh::ccl_grid(ntiles, 1, 1 << 20)), dim3(256), 0, st, mask, parent, (int)sx,
                     (int)sy, (int)sz);
  hipLaunchKernelGGL(kh::fill_mark_open_kernel, dim3(kh::ccl_grid(n, 256)), dim3(256), 0, st, parent, open, (int)sx, (int)sy,
                     (int)sz, ndim);
  hipLaunchKernelGGL(kh::fill_apply_kernel, dim3(kh::ccl_grid(n, 256)), dim3(256), 0, st, mask, parent, open, out, n,
                     (unsigned long long*)filled);
  KH_LAUNCH_CHECK();
  return KH_OK;
}

extern "C" int kh_ccl26_graph(const void* labels, int label_bytes, const uint32_t* graph, int64_t sx, int64_t sy, int64_t sz,
                              uint32_t* parent, uint32_t* chunk_counts, uint32_t* out, uint32_t* representative, uint32_t* ncomponents,
                              uint16_t* out16, void* stream) {
  if (int rc = kh::require_device()) return rc;
  if (!labels || !graph || !parent || !chunk_counts || !out || !representative || !ncomponents || sx <= 0 || sy <= 0 || sz <= 0 ||
      sx * sy * sz >= (1ll << 32) - 1) {
    kh::set_error("kh_ccl26_graph: bad arguments (null pointer, empty volume or >= 2^32-1 voxels)");
    return KH_EINVAL;
  }
  hipStream_t st = (hipStream_t)stream;
  switch (label_bytes) {
    case 1: return kh::cclg_impl((const uint8_t*)labels, graph, sx, sy, sz, parent, chunk_counts, out, representative, ncomponents, out16, st);
    case 2: return kh::cclg_impl((const uint16_t*)labels, graph, sx, sy, sz, parent, chunk_counts, out, representative, ncomponents, out16, st);
    case 4: return kh::cclg_impl((const uint32_t*)labels, graph, sx, sy, sz, parent, chunk_counts, out, representative, ncomponents, out16, st);
    case 8: return kh::cclg_impl((const uint64_t*)labels, graph, sx, sy, sz, parent, chunk_counts, out, representative, ncomponents, out16, st);
    default: kh::set_error("kh_ccl26_graph: label_bytes must be 1, 2, 4 or 8"); return KH_EINVAL;
  }
}

extern "C" int kh_edt_graph_cells(const void* labels, int label_bytes, const uint32_t* graph, int64_t sx, int64_t sy, int64_t sz,
                                  int black_border, uint8_t* cells, void* stream) {
  if (int rc = kh::require_device()) return rc;
  if (!labels || !graph || !cells || sx <= 0 || sy <= 0 || sz <= 0 || 8 * sx * sy * sz >= (1ll << 32)) {
    kh::set_error("kh_edt_graph_cells: bad arguments (null pointer, empty volume or >= 2^32 cells)");
    return KH_EINVAL;
  }
  hipStream_t st = (hipStream_t)stream;
  const int64_t n = sx * sy * sz;
  const dim3 grid(kh::ccl_grid(n, 256));
  switch (label_bytes) {
    case 1: hipLaunchKernelGGL((kh::edt_graph_cells_kernel<uint8_t>), grid, dim3(256), 0, st, (const uint8_t*)labels, graph, (int)sx, (int)sy, (int)sz, black_border, cells); break;
    case 2: hipLaunchKernelGGL((kh::edt_graph_cells_kernel<uint16_t>), grid, dim3(256), 0, st, (const uint16_t*)labels, graph, (int)sx, (int)sy, (int)sz, black_border, cells); break;
    case 4: hipLaunchKernelGGL((kh::edt_graph_cells_kernel<uint32_t>), grid, dim3(256), 0, st, (const uint32_t*)labels, graph, (int)sx, (int)sy, (int)sz, black_border, cells); break;
    default: kh::set_error("kh_edt_graph_cells: label_bytes must be 1, 2 or 4"); return KH_EINVAL;
  }
  KH_LAUNCH_CHECK();
  return KH_OK;
}

extern "C" int kh_edt_graph_sample(const float* fine, int64_t sx, int64_t sy, int64_t sz, float* out, void* stream) {
  if (int rc = kh::require_device()) return rc;
  if (!fine || !out || sx <= 0 || sy <= 0 || sz <= 0) { kh::set_error("kh_edt_graph_sample: bad arguments"); return KH_EINVAL; }
  hipLaunchKernelGGL(kh::edt_graph_sample_kernel, dim3(kh::ccl_grid(sx * sy * sz, 256)), dim3(256), 0, (hipStream_t)stream, fine, (int)sx,
                     (int)sy, (int)sz, out);
  KH_LAUNCH_CHECK();
  return KH_OK;
}

// ------------------------------------------------------------------------------------------------
// Holes of every label in one pass (kimimaro.intake.fill_all_holes, kimimaro/intake.py:747-795).
// A REGION is a 6-connected component of equal value, value 0 included.  hole(L) -- what the reference's per-crop fill_voids.fill
// paints with L -- is a union of regions, so the voxel work is one union-find over the volume (the one above, on the 3 already-
// rastered face neighbours of equal value), a table per region, and the set of region pairs that share a voxel face; which region
// goes to whom is decided on that small graph by the host (kh_host_resolve_holes, common.hip).
namespace kh {

// init: as ccl_init_kernel, but every voxel takes part (0 is a value like any other)
template <typename LT>
__global__ __launch_bounds__(256) void reg_init_kernel(const LT* __restrict__ lab, uint32_t* __restrict__ parent, int sx, int64_t nrows) {
  const int xt = (sx + 255) >> 8;
  const int64_t ntiles = (int64_t)xt * nrows;
  const int lane = threadIdx.x & 63;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int x = (int)(t % xt) * 256 + threadIdx.x;
    const int64_t i = x + (int64_t)sx * (t / xt);
    const LT L = x < sx ? lab[i] : (LT)0;
    LT Lm = (LT)__shfl_up((unsigned long long)L, 1);
    const bool start = lane == 0 || Lm != L;      // (the lanes behind the row's end come after its voxels: they start no run of theirs)
    const unsigned long long m = __builtin_amdgcn_ballot_w64(start) & ((lane == 63) ? ~0ull : ((2ull << lane) - 1ull));
    if (x < sx) parent[i] = (uint32_t)(i - (lane - (63 - __clzll((long long)m))));
  }
}

// link: the x runs are pre-linked inside every 64-lane chunk (one union where a run crosses a chunk boundary).  The voxel above /
// in front is linked unless the voxel to the left has the value and so has ITS neighbour in that row: the two rows' runs then
// overlap further left, and the leftmost voxel of the overlap has made the link.
template <typename LT>
__global__ __launch_bounds__(256) void reg_link_kernel(const LT* __restrict__ lab, uint32_t* parent, int sx, int sy, int sz) {
  const int xt = (sx + 255) >> 8;
  const int64_t ntiles = (int64_t)xt * sy * sz;
  const int64_t sxy = (int64_t)sx * sy;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int x = (int)(t % xt) * 256 + threadIdx.x;
    const int64_t r = t / xt;
    const int y = (int)(r % sy), z = (int)(r / sy);
    if (x >= sx) continue;
    const int64_t i = x + (int64_t)sx * y + sxy * z;
    const LT L = lab[i];
    const bool left = x > 0 && lab[i - 1] == L;
    if (left && (x & 63) == 0) ccl_union(parent, (uint32_t)i, (uint32_t)(i - 1));
    if (y > 0 && lab[i - sx] == L && !(left && lab[i - sx - 1] == L)) ccl_union(parent, (uint32_t)i, (uint32_t)(i - sx));
    if (z > 0 && lab[i - sxy] == L && !(left && lab[i - sxy - 1] == L)) ccl_union(parent, (uint32_t)i, (uint32_t)(i - sxy));
  }
}

template <typename LT>
static int regions_impl(const LT* lab, int64_t sx, int64_t sy, int64_t sz, uint32_t* parent, uint32_t* chunk_counts, uint32_t* out,
                        uint32_t* rep, uint32_t* total, hipStream_t st) {
  const int64_t n = sx * sy * sz;
  const int64_t nchunks = (n + 1023) / 1024;
  const int64_t ntiles = ((sx + 255) / 256) * sy * sz;
  hipLaunchKernelGGL((reg_init_kernel<LT>), dim3(ccl_grid(ntiles, 1, 1 << 20)), dim3(256), 0, st, lab, parent, (int)sx, sy * sz);
  hipLaunchKernelGGL((reg_link_kernel<LT>), dim3(ccl_grid(ntiles, 1, 1 << 20)), dim3(256), 0, st, lab, parent, (int)sx, (int)sy, (int)sz);
  hipLaunchKernelGGL(ccl_flatten_count_kernel, dim3(ccl_grid(nchunks, 1)), dim3(256), 0, st, parent, n, chunk_counts);
  hipLaunchKernelGGL(ccl_scan_kernel, dim3(1), dim3(1024), 0, st, chunk_counts, nchunks, total);
  hipLaunchKernelGGL(ccl_number_roots_kernel, dim3(ccl_grid(nchunks, 1)), dim3(256), 0, st, parent, n, chunk_counts, out, rep);
  hipLaunchKernelGGL(ccl_relabel_kernel, dim3(ccl_grid(n, 256)), dim3(256), 0, st, parent, n, out, (uint16_t*)nullptr, total);
  KH_LAUNCH_CHECK();
  return KH_OK;
}

// table, per region: the value (read at its representative voxel), the voxel count, whether it owns a voxel on a face of the array.
template <typename LT>
__global__ __launch_bounds__(256) void reg_value_kernel(const LT* __restrict__ lab, const uint32_t* __restrict__ rep, int64_t nregions,
                                                        unsigned long long* __restrict__ value) {
  for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r <= nregions; r += (int64_t)gridDim.x * 256)
    value[r] = r == 0 ? 0ull : (unsigned long long)lab[rep[r]];
}

// lanes along x: the first lane of a run of equal region ids inside its 64-lane chunk adds the run's length and sets the face flag
// for the whole run (one atomic per run, not per voxel; the flag is looked at before it is written).  faces: which faces of the array
// count (bit 0 x == 0, bit 1 x == sx-1, bits 2, 3 the y faces, 4, 5 the z faces); kh_region_table passes all six, kh_region_table_box
// those of a box that are faces of its dataset (XsBox::dataset_faces of section.hip)
__global__ __launch_bounds__(256) void reg_table_kernel(const uint32_t* __restrict__ region, int sx, int sy, int sz, int ndim,
                                                        uint32_t faces, uint32_t* __restrict__ count, uint8_t* face) {
  const int xt = (sx + 255) >> 8;
  const int64_t ntiles = (int64_t)xt * sy * sz;
  const int lane = threadIdx.x & 63;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int x = (int)(t % xt) * 256 + threadIdx.x;
    const int64_t row = t / xt;
    const int y = (int)(row % sy), z = (int)(row / sy);
    const bool valid = x < sx;
    const uint32_t r = valid ? region[x + (int64_t)sx * row] : 0u;      // (0 is no region id)
    const uint32_t rm = __shfl_up(r, 1);
    const bool start = valid && (lane == 0 || rm != r);
    const unsigned long long starts = __builtin_amdgcn_ballot_w64(start);
    const int nvalid = __popcll(__builtin_amdgcn_ballot_w64(valid));   // the valid lanes of a chunk are its first ones
    if (start) {
      const unsigned long long later = lane == 63 ? 0ull : (starts & ~((2ull << lane) - 1ull));
      const int end = later ? __builtin_ctzll(later) : nvalid;
      const int len = end - lane;
      atomicAdd(&count[r], (uint32_t)len);
      const uint32_t on = (x == 0 ? 1u : 0u) | (x + len == sx ? 2u : 0u) |
                          (ndim >= 2 ? (y == 0 ? 4u : 0u) | (y == sy - 1 ? 8u : 0u) : 0u) |
                          (ndim >= 3 ? (z == 0 ? 16u : 0u) | (z == sz - 1 ? 32u : 0u) : 0u);
      const bool f = (on & faces) != 0u;
      if (f && face[r] == 0) face[r] = 1;
    }
  }
}

// pairs: the set of unordered pairs of regions that share a voxel face, as keys (smaller id << 32 | larger id) in an open-addressing
// hash set in HBM (0 = empty slot; linear probing).  A key equal to the previous lane's key of the same direction is dropped first
// (a run of one region lying on a run of another gives one key per 64 lanes); the slot is read with a plain load before any
// compare-and-swap, so a pair that is in the set already costs no atomic.  A probe sequence longer than REG_MAX_PROBES sets
// state[1]: the caller retries with a larger table.  state[0] counts the keys inserted.
static constexpr int REG_MAX_PROBES = 512;
__device__ __forceinline__ void reg_pair_insert(unsigned long long* table, unsigned long long mask, unsigned long long key, uint32_t* state) {
  unsigned long long h = key * 0x9E3779B97F4A7C15ull;
  h ^= h >> 29;
  h *= 0xBF58476D1CE4E5B9ull;
  h ^= h >> 32;
  unsigned long long slot = h & mask;
  for (int probe = 0; probe < REG_MAX_PROBES; probe++, slot = (slot + 1) & mask) {
    const unsigned long long cur = __hip_atomic_load(&table[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == key) return;
    if (cur != 0ull) continue;
    const unsigned long long old = atomicCAS(&table[slot], 0ull, key);
    if (old == 0ull) { atomicAdd(&state[0], 1u); return; }
    if (old == key) return;
  }
  __hip_atomic_store(&state[1], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(256) void reg_pairs_kernel(const uint32_t* __restrict__ region, int sx, int sy, int sz,
                                                        unsigned long long* table, unsigned long long mask, uint32_t* state) {
  const int xt = (sx + 255) >> 8;
  const int64_t ntiles = (int64_t)xt * sy * sz;
  const int64_t sxy = (int64_t)sx * sy;
  const int lane = threadIdx.x & 63;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    // a table that has overflowed is abandoned (the whole wave leaves: the shuffles below need all of its lanes)
    if (__shfl(__hip_atomic_load(&state[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), 0) != 0u) return;
    const int x = (int)(t % xt) * 256 + threadIdx.x;
    const int64_t row = t / xt;
    const int y = (int)(row % sy), z = (int)(row / sy);
    const bool valid = x < sx;
    const int64_t i = x + (int64_t)sx * row;
    const uint32_t r = valid ? region[i] : 0u;
#pragma unroll
    for (int d = 0; d < 3; d++) {
      const bool there = valid && (d == 0 ? x > 0 : (d == 1 ? y > 0 : z > 0));
      const uint32_t q = there ? region[i - (d == 0 ? 1 : (d == 1 ? (int64_t)sx : sxy))] : r;
      unsigned long long key = q == r ? 0ull : (((unsigned long long)(q < r ? q : r) << 32) | (unsigned long long)(q < r ? r : q));
      const unsigned long long before = __shfl_up(key, 1);
      if (lane > 0 && before == key) key = 0ull;
      if (key != 0ull) reg_pair_insert(table, mask, key, state);
    }
  }
}

// seam pairs: two facing planes of region ids on either side of a cut through a dataset, low[p] facing high[p]; the
// keys low[p] << 32 | high[p] go into the set above by the same insert.  The caller numbers the regions so that the low side has the
// smaller ids; the kernel reads no labels and does not ask whether the two regions carry one value.
__global__ __launch_bounds__(256) void reg_seam_pairs_kernel(const uint32_t* __restrict__ low, const uint32_t* __restrict__ high, int64_t m,
                                                             unsigned long long* table, unsigned long long mask, uint32_t* state) {
  const int lane = threadIdx.x & 63;
  const int64_t ntiles = (m + 255) >> 8;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    if (__shfl(__hip_atomic_load(&state[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), 0) != 0u) return;
    const int64_t p = t * 256 + threadIdx.x;
    unsigned long long key = p < m ? (((unsigned long long)low[p] << 32) | (unsigned long long)high[p]) : 0ull;
    const unsigned long long before = __shfl_up(key, 1);
    if (lane > 0 && before == key) key = 0ull;
    if (key != 0ull) reg_pair_insert(table, mask, key, state);
  }
}

// apply: a voxel of a region with an owner takes the owner's value
template <typename LT>
__global__ __launch_bounds__(256) void reg_apply_kernel(const uint32_t* __restrict__ region, const unsigned long long* __restrict__ owner,
                                                        LT* __restrict__ lab, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const unsigned long long o = owner[region[i]];
    if (o != 0ull) lab[i] = (LT)o;
  }
}

// apply for a core of a dataset: the ids are the dataset's provisional ids, the table holds the core's own range
// base + 1 .. base + nregions.  An id outside that range reads no table entry: the voxel is left alone and counted in state[1] (the
// ids may come from a caller's file).  One block-uniform trip count, so every ballot sees its whole wave; a wave sums its two
// counts over its trips and adds each with one atomic at the end.
template <typename LT>
__global__ __launch_bounds__(256) void reg_apply_box_kernel(const uint32_t* __restrict__ region, uint32_t base, uint32_t nregions,
                                                            const unsigned long long* __restrict__ owner, LT* __restrict__ lab, int64_t n,
                                                            unsigned long long* state) {
  unsigned long long painted = 0ull, outside = 0ull;
  for (int64_t t = (int64_t)blockIdx.x * 256; t < n; t += (int64_t)gridDim.x * 256) {
    const int64_t i = t + threadIdx.x;
    const bool valid = i < n;
    const uint32_t r = valid ? region[i] - base : 1u;                     // u32 arithmetic: an id below base wraps above nregions
    const bool known = r - 1u < nregions;
    const unsigned long long o = (valid && known) ? owner[r] : 0ull;
    if (o != 0ull) lab[i] = (LT)o;
    painted += (unsigned long long)__popcll(__builtin_amdgcn_ballot_w64(o != 0ull));
    outside += (unsigned long long)__popcll(__builtin_amdgcn_ballot_w64(valid && !known));
  }
  if ((threadIdx.x & 63) == 0) {
    if (painted) atomicAdd(&state[0], painted);
    if (outside) atomicAdd(&state[1], outside);
  }
}

}  // namespace kh

#define KH_REG_DISPATCH(bytes, name, CALL)                   \
  switch (bytes) {                                           \
    case 1: { typedef uint8_t LT; CALL; } break;             \
    case 2: { typedef uint16_t LT; CALL; } break;            \
    case 4: { typedef uint32_t LT; CALL; } break;            \
    case 8: { typedef uint64_t LT; CALL; } break;            \
    default: kh::set_error(name ": label_bytes must be 1, 2, 4 or 8"); return KH_EINVAL; \
  }

extern "C" int kh_regions6(const void* labels, int label_bytes, int64_t sx, int64_t sy, int64_t sz, uint32_t* parent,
                           uint32_t* chunk_counts, uint32_t* region, uint32_t* representative, uint32_t* nregions, void* stream) {
  if (int rc = kh::require_device()) return rc;
  if (!labels || !parent || !chunk_counts || !region || !representative || !nregions || sx <= 0 || sy <= 0 || sz <= 0 ||
      sx >= (1ll << 31) || sy >= (1ll << 31) || sz >= (1ll << 31) || sx * sy * sz >= (1ll << 32) - 1) {
    kh::set_error("kh_regions6: bad arguments (null pointer, empty volume or >= 2^32-1 voxels)");
    return KH_EINVAL;
  }
  hipStream_t st = (hipStream_t)stream;
  KH_REG_DISPATCH(label_bytes, "kh_regions6",
                  return kh::regions_impl((const LT*)labels, sx, sy, sz, parent, chunk_counts, region, representative, nregions, st));
  return KH_OK;
}

static int region_table_impl(const char* name, const void* labels, int label_bytes, const uint32_t* region,
                             const uint32_t* representative, int64_t nregions, int ndim, int64_t sx, int64_t sy, int64_t sz,
                             uint32_t faces, uint64_t* value, uint32_t* count, uint8_t* face, void* stream) {
  if (int rc = kh::require_device()) return rc;
  if (!labels || !region || !representative || !value || !count || !face || sx <= 0 || sy <= 0 || sz <= 0 || sx >= (1ll << 31) ||
      sy >= (1ll << 31) || sz >= (1ll << 31) || sx * sy * sz >= (1ll << 32) - 1 || nregions < 1 || nregions > sx * sy * sz ||
      ndim < 1 || ndim > 3 || (ndim < 3 && sz != 1) || (ndim < 2 && sy != 1)) {
    kh::set_error("%s: bad arguments (null pointer, empty volume, >= 2^32-1 voxels, nregions outside [1, nvox], or an "
                  "axis beyond ndim with extent > 1)", name);
    return KH_EINVAL;
  }
  if (faces > 63u) {
    kh::set_error("%s: dataset_faces has six bits", name);
    return KH_EINVAL;
  }
  hipStream_t st = (hipStream_t)stream;
  KH_HIP_CHECK(hipMemsetAsync(count, 0, sizeof(uint32_t) * (size_t)(nregions + 1), st));
  KH_HIP_CHECK(hipMemsetAsync(face, 0, (size_t)(nregions + 1), st));
  KH_REG_DISPATCH(label_bytes, "kh_region_table",      // (the message serves both entries: the argument is the same)
                  hipLaunchKernelGGL((kh::reg_value_kernel<LT>), dim3(kh::ccl_grid(nregions + 1, 256)), dim3(256), 0, st,
                                     (const LT*)labels, representative, nregions, (unsigned long long*)value));
  const int64_t ntiles = ((sx + 255) / 256) * sy * sz;
  hipLaunchKernelGGL(kh::reg_table_kernel, dim3(kh::ccl_grid(ntiles, 1, 1 << 20)), dim3(256), 0, st, region, (int)sx, (int)sy, (int)sz,
                     ndim, faces, count, face);
  KH_LAUNCH_CHECK();
  return KH_OK;
}

extern "C" int kh_region_table(const void* labels, int label_bytes, const uint32_t* region, const uint32_t* representative,
                               int64_t nregions, int ndim, int64_t sx, int64_t sy, int64_t sz, uint64_t* value, uint32_t* count,
                               uint8_t* face, void* stream) {
  return region_table_impl("kh_region_table", labels, label_bytes, region, representative, nregions, ndim, sx, sy, sz, 63u, value, count,
                           face, stream);
}

extern "C" int kh_region_table_box(const void* labels, int label_bytes, const uint32_t* region, const uint32_t* representative,
                                   int64_t nregions, int ndim, int64_t sx, int64_t sy, int64_t sz, uint32_t dataset_faces,
                                   uint64_t* value, uint32_t* count, uint8_t* face, void* stream) {
  return region_table_impl("kh_region_table_box", labels, label_bytes, region, representative, nregions, ndim, sx, sy, sz, dataset_faces,
                           value, count, face, stream);
}

extern "C" int kh_region_pairs(const uint32_t* region, int64_t sx, int64_t sy, int64_t sz, uint64_t* table, int64_t capacity,
                               uint32_t* state, void* stream) {
  if (int rc = kh::require_device()) return rc;
  if (!region || !table || !state || sx <= 0 || sy <= 0 || sz <= 0 || sx >= (1ll << 31) || sy >= (1ll << 31) || sz >= (1ll << 31) ||
      sx * sy * sz >= (1ll << 32) - 1 || capacity < 64 || (capacity & (capacity - 1)) != 0) {
    kh::set_error("kh_region_pairs: bad arguments (null pointer, empty volume, >= 2^32-1 voxels, or a capacity that is no power of "
                  "two >= 64)");
    return KH_EINVAL;
  }
  hipStream_t st = (hipStream_t)stream;
  KH_HIP_CHECK(hipMemsetAsync(table, 0, sizeof(uint64_t) * (size_t)capacity, st));
  KH_HIP_CHECK(hipMemsetAsync(state, 0, 2 * sizeof(uint32_t), st));
  const int64_t ntiles = ((sx + 255) / 256) * sy * sz;
  hipLaunchKernelGGL(kh::reg_pairs_kernel, dim3(kh::ccl_grid(ntiles, 1, 1 << 20)), dim3(256), 0, st, region, (int)sx, (int)sy, (int)sz,
                     (unsigned long long*)table, (unsigned long long)(capacity - 1), state);
  KH_LAUNCH_CHECK();
  return KH_OK;
}

extern "C" int kh_region_seam_pairs(const uint32_t* low, const uint32_t* high, int64_t m, uint64_t* table, int64_t capacity,
                                    uint32_t* state, void* stream) {
  if (int rc = kh::require_device()) return rc;
  if (!low || !high || !table || !state || m <= 0 || m >= (1ll << 32) || capacity < 64 || (capacity & (capacity - 1)) != 0) {
    kh::set_error("kh_region_seam_pairs: bad arguments (null pointer, m outside [1, 2^32), or a capacity that is no power of two >= 64)");
    return KH_EINVAL;
  }
  hipStream_t st = (hipStream_t)stream;
  KH_HIP_CHECK(hipMemsetAsync(table, 0, sizeof(uint64_t) * (size_t)capacity, st));
  KH_HIP_CHECK(hipMemsetAsync(state, 0, 2 * sizeof(uint32_t), st));
  hipLaunchKernelGGL(kh::reg_seam_pairs_kernel, dim3(kh::ccl_grid((m + 255) / 256, 1, 1 << 20)), dim3(256), 0, st, low, high, m,
                     (unsigned long long*)table, (unsigned long long)(capacity - 1), state);
  KH_LAUNCH_CHECK();
  return KH_OK;
}

extern "C" int kh_region_apply(const uint32_t* region, const uint64_t* owner, void* labels, int label_bytes, int64_t nvox,
                               void* stream) {
  if (int rc = kh::require_device()) return rc;
  if (!region || !owner || !labels || nvox <= 0 || nvox >= (1ll << 32) - 1) {
    kh::set_error("kh_region_apply: bad arguments (null pointer, empty volume or >= 2^32-1 voxels)");
    return KH_EINVAL;
  }
  hipStream_t st = (hipStream_t)stream;
  KH_REG_DISPATCH(label_bytes, "kh_region_apply",
                  hipLaunchKernelGGL((kh::reg_apply_kernel<LT>), dim3(kh::ccl_grid(nvox, 256)), dim3(256), 0, st, region,
                                     (const unsigned long long*)owner, (LT*)labels, nvox));
  KH_LAUNCH_CHECK();
  return KH_OK;
}

extern "C" int kh_region_apply_box(const uint32_t* region, uint32_t base, int64_t nregions, const uint64_t* owner, void* labels,
                                   int label_bytes, int64_t nvox, uint64_t* state, void* stream) {
  if (int rc = kh::require_device()) return rc;
  if (!region || !owner || !labels || !state || nvox <= 0 || nvox >= (1ll << 32) - 1 || nregions < 1 ||
      (int64_t)base + nregions > (1ll << 32) - 1 || (label_bytes != 1 && label_bytes != 2 && label_bytes != 4 && label_bytes != 8)) {
    kh::set_error("kh_region_apply_box: bad arguments (null pointer, empty volume or >= 2^32-1 voxels, nregions < 1, "
                  "base + nregions above 2^32-1, or label_bytes not 1, 2, 4 or 8)");      // (before anything is written)
    return KH_EINVAL;
  }
  hipStream_t st = (hipStream_t)stream;
  KH_HIP_CHECK(hipMemsetAsync(state, 0, 2 * sizeof(uint64_t), st));
  // a streaming pass: blocks that stride over the volume, a few per CU, rather than one short-lived block per 256 voxels
  KH_REG_DISPATCH(label_bytes, "kh_region_apply_box",
                  hipLaunchKernelGGL((kh::reg_apply_box_kernel<LT>), dim3(kh::ccl_grid(nvox, 256, 2048)), dim3(256), 0, st, region, base,
                                     (uint32_t)nregions, (const unsigned long long*)owner, (LT*)labels, nvox,
                                     (unsigned long long*)state));
  KH_LAUNCH_CHECK();
  return KH_OK;
}
