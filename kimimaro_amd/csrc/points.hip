// points.hip -- the two point queries of the public interface that are whole-volume passes (gfx950).
//
//   kh_nearest_label_voxels   kimimaro.synapses_to_targets (kimimaro/intake.py:706-745): for every (label, centroid) query the voxel
//                             of that label nearest to the centroid -- scipy's cdist + np.argmin(axis=0) over
//                             np.vstack((labels == label).nonzero()).T, for ALL labels and centroids in two passes over the volume
//                             instead of one pass and one dense distance matrix per label.
//   kh_nearest_label_voxels_box   the same sweep (nearest_sweep, one body for both) on ONE BOX of a dataset that is never resident as
//                             a whole, on running per-query results that stay on the device from box to box
//                             (synapses_to_targets_chunked), with the carry rule between its passes.
//   kh_binary_edge_count /    skeletontricks.extract_edges_from_binary_image (skeletontricks.pyx:1047-1086, skeletontricks.hpp:399-495)
//   kh_binary_edge_emit       on the words of kh_neighbor_mask: count, (the caller's scan), emit -- in a canonical order instead of
//                             the iteration order of an unordered_set.
//
// Both are HBM-bound sweeps with lanes along x.  Every global atomic on gfx950 is a fabric round trip: the nearest
// voxel passes reduce inside the wave and ask the memory only when a lane beats what is already there; the edge count adds once
// per wave.
#include "common.h"

namespace kh {

static inline unsigned points_grid(int64_t n, int64_t cap) {
  if (n > cap) n = cap;
  if (n < 1) n = 1;
  return (unsigned)n;
}

__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const unsigned long long o = __shfl_xor(v, d);
    v = o < v ? o : v;
  }
  return v;
}

__global__ void fill_u64_kernel(unsigned long long* p, int64_t n, unsigned long long v) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) p[i] = v;
}

// a voxel coordinate of nearest_sweep: in a dataset 64 bits, in a resident volume the int it is
template <bool BOX>
using coord_t = typename std::conditional<BOX, int64_t, int>::type;

// ONE body for both nearest-voxel kernels: the sweep of a volume of extent (ex, ey, ez).
// PASS 1: best_d[g] = min over the label's voxels of the bits of d (non-negative doubles order like u64).
// PASS 2: best_c[g] = min C-order index X*dsy*dsz + Y*dsz + Z over the label's voxels whose d has exactly those bits.
// A block walks a CONTIGUOUS range of x tiles (256 voxels of one row): a thread's next voxel is the one 256 further along the row or
// the same x of the next row, which mostly carries the label it has just looked up -- the search of the table is then skipped.
// With BOX the volume is one box, low corner (lox, loy, loz), of a dataset with y and z extents dsy, dsz.  Three
// things differ:
//   the coordinate   distances and the index come from X = lox + x in the DATASET, 64 bits; without BOX lo is 0 and X stays the int x,
//                    so that its conversion to double remains the 32-bit one
//   the row          query q owns row g = qidx[q] of the running best_d / best_c; without BOX row q, and qidx is not read
//   the extents      dsy, dsz of the index are the dataset's; without BOX the volume's own sy, sz
template <typename LT, int PASS, bool BOX>
__device__ __forceinline__ void nearest_sweep(const LT* __restrict__ lab, int ex, int ey, int ez, coord_t<BOX> lox, coord_t<BOX> loy,
                                              coord_t<BOX> loz, coord_t<BOX> dsy, coord_t<BOX> dsz, int64_t tiles_per_block,
                                              const unsigned long long* __restrict__ table, const uint32_t* __restrict__ qstart, int nlab,
                                              const double* __restrict__ cen, const uint32_t* __restrict__ qidx, unsigned long long* best_d,
                                              unsigned long long* best_c) {
  const int xt = (ex + 255) >> 8;
  const int64_t ntiles = (int64_t)xt * ey * ez;
  const int64_t t0 = (int64_t)blockIdx.x * tiles_per_block;
  const int64_t t1 = (t0 + tiles_per_block < ntiles) ? t0 + tiles_per_block : ntiles;
  unsigned long long lastL = 0;
  int lastSlot = -2;                      // -2: nothing looked up yet; -1: lastL is not in the table
  for (int64_t t = t0; t < t1; t++) {
    const int x = (int)(t % xt) * 256 + (int)threadIdx.x;
    const int64_t r = t / xt;
    const int y = (int)(r % ey), z = (int)(r / ey);
    int slot = -1;
    if (x < ex) {
      const unsigned long long L = (unsigned long long)lab[x + (int64_t)ex * (y + (int64_t)ey * z)];
      if (lastSlot == -2 || L != lastL) {
        int lo = 0, hi = nlab;            // first entry >= L
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (table[mid] < L) lo = mid + 1; else hi = mid;
        }
        lastL = L;
        lastSlot = (lo < nlab && table[lo] == L) ? lo : -1;
      }
      slot = lastSlot;
    }
    const coord_t<BOX> X = lox + x, Y = loy + y, Z = loz + z;       // the voxel in the dataset
    // the distinct labels of the wave, one after the other; the lanes of one label combine before anything goes to memory
    unsigned long long todo = __ballot(slot >= 0);
    while (todo) {
      const int s = __shfl(slot, __ffsll((long long)todo) - 1);
      const bool mine = slot == s;
      todo &= ~__ballot(mine);
      const uint32_t q0 = qstart[s], q1 = qstart[s + 1];
      for (uint32_t q = q0; q < q1; q++) {
        const uint32_t g = BOX ? qidx[q] : q;
        // scipy's euclidean kernel: s = 0; s += d*d per axis; sqrt(s) -- every operation rounded (no contraction in this library)
        const double dx = (double)X - cen[3 * (size_t)q + 0];
        const double dy = (double)Y - cen[3 * (size_t)q + 1];
        const double dz = (double)Z - cen[3 * (size_t)q + 2];
        const double d = __dsqrt_rn((dx * dx + dy * dy) + dz * dz);
        const unsigned long long key = (unsigned long long)__double_as_longlong(d);
        const unsigned long long cur = best_d[g];     // PASS 1: may be stale, i.e. too large -- costs an atomic, never a result
        if (PASS == 1) {
          if (!__any(mine && key < cur)) continue;
          const unsigned long long m = wave_min_u64(mine ? key : ~0ull);
          const unsigned long long holders = __ballot(mine && key == m);
          if ((int)(threadIdx.x & 63) == __ffsll((long long)holders) - 1) atomicMin(&best_d[g], m);
        } else {
          const bool hit = mine && key == cur;
          if (!__any(hit)) continue;
          const unsigned long long c = ((unsigned long long)X * (unsigned long long)dsy + (unsigned long long)Y) * (unsigned long long)dsz + (unsigned long long)Z;
          const unsigned long long m = wave_min_u64(hit ? c : ~0ull);
          if (hit && c == m && m < best_c[g]) atomicMin(&best_c[g], m);
        }
      }
    }
  }
}

template <typename LT, int PASS>
__global__ __launch_bounds__(256) void nearest_kernel(const LT* __restrict__ lab, int sx, int sy, int sz, int64_t tiles_per_block,
                                                      const unsigned long long* __restrict__ table, const uint32_t* __restrict__ qstart,
                                                      int nlab, const double* __restrict__ cen, unsigned long long* best_d,
                                                      unsigned long long* best_c) {
  nearest_sweep<LT, PASS, false>(lab, sx, sy, sz, 0, 0, 0, sy, sz, tiles_per_block, table, qstart, nlab, cen, nullptr, best_d, best_c);
}

// The running results of a dataset in boxes: best_d / best_c come in holding the best of the boxes visited so far and are never
// filled here.
//   carry_save   scratch[q] = best_d[qidx[q]]                        the distances that came in
//   PASS 1       best_d[g] = min(itself, the box's distances)        nearest_sweep<.., 1, true>
//   carry_reset  best_c[g] = ~0 where best_d[g] != scratch[q]         a lowered distance makes the index of earlier boxes stale
//   PASS 2       best_c[g] = min(itself, the box's indices at best_d[g])   an index that was kept competes with this box's
__global__ void carry_save_kernel(const uint32_t* __restrict__ qidx, int64_t nq, const unsigned long long* __restrict__ best_d,
                                  unsigned long long* __restrict__ scratch) {
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < nq; q += (int64_t)gridDim.x * blockDim.x) scratch[q] = best_d[qidx[q]];
}

__global__ void carry_reset_kernel(const uint32_t* __restrict__ qidx, int64_t nq, const unsigned long long* __restrict__ best_d,
                                   const unsigned long long* __restrict__ scratch, unsigned long long* __restrict__ best_c) {
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < nq; q += (int64_t)gridDim.x * blockDim.x) {
    const uint32_t g = qidx[q];
    if (best_d[g] != scratch[q]) best_c[g] = ~0ull;
  }
}

template <typename LT, int PASS>
__global__ __launch_bounds__(256) void nearest_box_kernel(const LT* __restrict__ lab, int ex, int ey, int ez, int64_t lox, int64_t loy,
                                                          int64_t loz, int64_t dsy, int64_t dsz, int64_t tiles_per_block,
                                                          const unsigned long long* __restrict__ table,
                                                          const uint32_t* __restrict__ qstart, int nlab, const double* __restrict__ cen,
                                                          const uint32_t* __restrict__ qidx, unsigned long long* best_d,
                                                          unsigned long long* best_c) {
  nearest_sweep<LT, PASS, true>(lab, ex, ey, ez, lox, loy, loz, dsy, dsz, tiles_per_block, table, qstart, nlab, cen, qidx, best_d, best_c);
}

// the 13 directions of dir_delta whose neighbour comes LATER in the Fortran raster, as a mask
__host__ __device__ constexpr uint32_t later_dirs() {
  uint32_t m = 0;
  for (int k = 0; k < 26; k++) {
    int dx = 0, dy = 0, dz = 0;
    dir_delta(k, dx, dy, dz);
    if (dz > 0 || (dz == 0 && (dy > 0 || (dy == 0 && dx > 0)))) m |= 1u << k;
  }
  return m;
}

// per voxel: does it lie on an edge (a neighbour in one of the `dirs` directions), and how many edges does it own -- those to its
// later neighbours.  totals[0] += vertices, totals[1] += edges: one atomic each per wave.
__global__ __launch_bounds__(256) void binary_edge_count_kernel(const uint32_t* __restrict__ nbr, int64_t nvox, uint32_t dirs,
                                                                uint8_t* __restrict__ is_vertex, uint8_t* __restrict__ n_owned,
                                                                unsigned long long* totals) {
  constexpr uint32_t LATER = later_dirs();
  unsigned long long nv = 0, ne = 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvox; i += (int64_t)gridDim.x * blockDim.x) {
    const uint32_t m = nbr[i] & dirs;
    const uint32_t own = (uint32_t)__popc(m & LATER);
    is_vertex[i] = m != 0;
    n_owned[i] = (uint8_t)own;
    nv += m != 0;
    ne += own;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    nv += __shfl_xor(nv, d);
    ne += __shfl_xor(ne, d);
  }
  if ((threadIdx.x & 63) == 0) {
    if (nv) atomicAdd(&totals[0], nv);
    if (ne) atomicAdd(&totals[1], ne);
  }
}

// vscan / escan: INCLUSIVE scans of is_vertex / n_owned over the raster.  The lower-indexed voxel of a pair owns the edge and emits
// its later neighbours in ascending index: rows (a, b), a < b, sorted by a, then b.
__global__ __launch_bounds__(256) void binary_edge_emit_kernel(const uint32_t* __restrict__ nbr, int sx, int sy, int sz, uint32_t dirs,
                                                               const int64_t* __restrict__ vscan, const int64_t* __restrict__ escan,
                                                               uint32_t* __restrict__ vertices, uint32_t* __restrict__ edges) {
  constexpr uint32_t LATER = later_dirs();
  // the 13 later directions in ascending (dz, dy, dx), i.e. ascending linear index of the neighbour
  constexpr int ORDER[13] = {1, 7, 3, 9, 21, 11, 23, 15, 5, 17, 24, 13, 25};
  const int xt = (sx + 255) >> 8;
  const int64_t ntiles = (int64_t)xt * sy * sz;
  const int64_t sxy = (int64_t)sx * sy;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int x = (int)(t % xt) * 256 + (int)threadIdx.x;
    const int64_t r = t / xt;
    const int y = (int)(r % sy), z = (int)(r / sy);
    if (x >= sx) continue;
    const int64_t i = x + (int64_t)sx * y + sxy * z;
    const uint32_t m = nbr[i] & dirs;
    if (m == 0) continue;
    const int64_t rank = vscan[i] - 1;
    vertices[3 * rank + 0] = (uint32_t)x;
    vertices[3 * rank + 1] = (uint32_t)y;
    vertices[3 * rank + 2] = (uint32_t)z;
    const uint32_t own = m & LATER;
    int64_t e = escan[i] - __popc(own);
#pragma unroll
    for (int j = 0; j < 13; j++) {
      const int k = ORDER[j];
      if (!((own >> k) & 1u)) continue;
      int dx = 0, dy = 0, dz = 0;
      dir_delta(k, dx, dy, dz);
      // (a set bit says the neighbour is inside the volume and foreground: its mask has the opposite bit, so it is a vertex)
      edges[2 * e + 0] = (uint32_t)rank;
      edges[2 * e + 1] = (uint32_t)(vscan[i + dx + (int64_t)sx * dy + sxy * dz] - 1);
      e++;
    }
  }
}

}  // namespace kh

using namespace kh;

#define KH_POINTS_DISPATCH(bytes, CALL)                      \
  switch (bytes) {                                           \
    case 1: { typedef uint8_t LT; CALL; } break;             \
    case 2: { typedef uint16_t LT; CALL; } break;            \
    case 4: { typedef uint32_t LT; CALL; } break;            \
    case 8: { typedef uint64_t LT; CALL; } break;            \
    default: set_error("label_bytes must be 1, 2, 4 or 8"); return KH_EINVAL; \
  }

extern "C" int kh_nearest_label_voxels(const void* labels, int label_bytes, int64_t sx, int64_t sy, int64_t sz,
                                       const uint64_t* table, const uint32_t* query_start, int64_t nlabels, const double* centroids,
                                       int64_t nqueries, uint64_t* best_distance, uint64_t* best_voxel, void* stream) {
  if (int rc = require_device()) return rc;
  if (sx <= 0 || sy <= 0 || sz <= 0 || sx >= (1ll << 31) || sy >= (1ll << 31) || sz >= (1ll << 31) || nlabels <= 0 ||
      nlabels >= (1ll << 31) || nqueries <= 0 || nqueries >= (1ll << 32)) {
    set_error("kh_nearest_label_voxels: extents in [1, 2^31), 1 <= nlabels < 2^31, 1 <= nqueries < 2^32");
    return KH_EINVAL;
  }
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(fill_u64_kernel, dim3(points_grid((nqueries + 255) / 256, 1024)), dim3(256), 0, st,
                     (unsigned long long*)best_distance, nqueries, ~0ull);
  hipLaunchKernelGGL(fill_u64_kernel, dim3(points_grid((nqueries + 255) / 256, 1024)), dim3(256), 0, st,
                     (unsigned long long*)best_voxel, nqueries, ~0ull);
  const int64_t ntiles = ((sx + 255) / 256) * sy * sz;
  const unsigned grid = points_grid(ntiles, 4096);
  const int64_t per_block = (ntiles + grid - 1) / grid;
  KH_POINTS_DISPATCH(label_bytes, hipLaunchKernelGGL((nearest_kernel<LT, 1>), dim3(grid), dim3(256), 0, st, (const LT*)labels, (int)sx,
                                                     (int)sy, (int)sz, per_block, (const unsigned long long*)table, query_start,
                                                     (int)nlabels, centroids, (unsigned long long*)best_distance,
                                                     (unsigned long long*)best_voxel));
  KH_POINTS_DISPATCH(label_bytes, hipLaunchKernelGGL((nearest_kernel<LT, 2>), dim3(grid), dim3(256), 0, st, (const LT*)labels, (int)sx,
                                                     (int)sy, (int)sz, per_block, (const unsigned long long*)table, query_start,
                                                     (int)nlabels, centroids, (unsigned long long*)best_distance,
                                                     (unsigned long long*)best_voxel));
  KH_LAUNCH_CHECK();
  return KH_OK;
}

extern "C" int kh_nearest_label_voxels_box(const void* labels, int label_bytes, int64_t ex, int64_t ey, int64_t ez, int64_t lox,
                                           int64_t loy, int64_t loz, int64_t dsy, int64_t dsz, const uint64_t* table,
                                           const uint32_t* query_start, int64_t nlabels, const double* centroids,
                                           const uint32_t* query_index, int64_t nqueries, uint64_t* best_distance,
                                           uint64_t* best_voxel, uint64_t* scratch, void* stream) {
  if (int rc = require_device()) return rc;
  if (ex <= 0 || ey <= 0 || ez <= 0 || ex >= (1ll << 31) || ey >= (1ll << 31) || ez >= (1ll << 31) || lox < 0 || loy < 0 || loz < 0 ||
      dsy <= 0 || dsz <= 0 || nlabels <= 0 || nlabels >= (1ll << 31) || nqueries <= 0 || nqueries >= (1ll << 32)) {
    set_error("kh_nearest_label_voxels_box: extents in [1, 2^31), lo >= 0, dataset extents >= 1, 1 <= nlabels < 2^31, "
              "1 <= nqueries < 2^32");
    return KH_EINVAL;
  }
  if (label_bytes != 1 && label_bytes != 2 && label_bytes != 4 && label_bytes != 8) {
    set_error("label_bytes must be 1, 2, 4 or 8");
    return KH_EINVAL;
  }
  hipStream_t st = (hipStream_t)stream;
  unsigned long long* bd = (unsigned long long*)best_distance;
  unsigned long long* bc = (unsigned long long*)best_voxel;
  const unsigned qgrid = points_grid((nqueries + 255) / 256, 1024);
  const int64_t ntiles = ((ex + 255) / 256) * ey * ez;
  const unsigned blocks = points_grid(ntiles, 4096);     // the sibling's launch shape, on the box
  const int64_t per_block = (ntiles + blocks - 1) / blocks;
  hipLaunchKernelGGL(carry_save_kernel, dim3(qgrid), dim3(256), 0, st, query_index, nqueries, bd, (unsigned long long*)scratch);
  KH_POINTS_DISPATCH(label_bytes, hipLaunchKernelGGL((nearest_box_kernel<LT, 1>), dim3(blocks), dim3(256), 0, st, (const LT*)labels,
                                                     (int)ex, (int)ey, (int)ez, lox, loy, loz, dsy, dsz, per_block,
                                                     (const unsigned long long*)table, query_start, (int)nlabels, centroids,
                                                     query_index, bd, bc));
  hipLaunchKernelGGL(carry_reset_kernel, dim3(qgrid), dim3(256), 0, st, query_index, nqueries, bd, (unsigned long long*)scratch, bc);
  KH_POINTS_DISPATCH(label_bytes, hipLaunchKernelGGL((nearest_box_kernel<LT, 2>), dim3(blocks), dim3(256), 0, st, (const LT*)labels,
                                                     (int)ex, (int)ey, (int)ez, lox, loy, loz, dsy, dsz, per_block,
                                                     (const unsigned long long*)table, query_start, (int)nlabels, centroids,
                                                     query_index, bd, bc));
  KH_LAUNCH_CHECK();
  return KH_OK;
}

extern "C" int kh_binary_edge_count(const uint32_t* nbrmask, int64_t nvox, uint32_t directions, uint8_t* is_vertex, uint8_t* n_owned,
                                    uint64_t* totals, void* stream) {
  if (int rc = require_device()) return rc;
  if (nvox <= 0) {
    set_error("kh_binary_edge_count: nvox must be positive");
    return KH_EINVAL;
  }
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(fill_u64_kernel, dim3(1), dim3(64), 0, st, (unsigned long long*)totals, (int64_t)2, 0ull);
  hipLaunchKernelGGL(binary_edge_count_kernel, dim3(points_grid((nvox + 255) / 256, 4096)), dim3(256), 0, st, nbrmask, nvox,
                     directions, is_vertex, n_owned, (unsigned long long*)totals);
  KH_LAUNCH_CHECK();
  return KH_OK;
}

extern "C" int kh_binary_edge_emit(const uint32_t* nbrmask, int64_t sx, int64_t sy, int64_t sz, uint32_t directions,
                                   const int64_t* vertex_scan, const int64_t* edge_scan, uint32_t* vertices, uint32_t* edges,
                                   void* stream) {
  if (int rc = require_device()) return rc;
  if (sx <= 0 || sy <= 0 || sz <= 0 || sx >= (1ll << 31) || sy >= (1ll << 31) || sz >= (1ll << 31)) {
    set_error("kh_binary_edge_emit: extents in [1, 2^31)");
    return KH_EINVAL;
  }
  hipStream_t st = (hipStream_t)stream;
  const int64_t ntiles = ((sx + 255) / 256) * sy * sz;
  hipLaunchKernelGGL(binary_edge_emit_kernel, dim3(points_grid(ntiles, 1 << 20)), dim3(256), 0, st, nbrmask, (int)sx, (int)sy, (int)sz,
                     directions, vertex_scan, edge_scan, vertices, edges);
  KH_LAUNCH_CHECK();
  return KH_OK;
}
