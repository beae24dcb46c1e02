// graph.hip -- kh_voxel_graph: the voxel connectivity graph of a label volume (gfx950).
//
//   cc3d.voxel_connectivity_graph(labels, connectivity) is what the reference's docstring sends its users to for the voxel_graph=
//   of kimimaro.skeletonize (kimimaro/intake.py:66,113-117).  PARITY UNPINNED: cc3d's source is absent from the reference tree; the
//   word is DEFINED in include/kimi_hip.h and DESIGN.md 3.21, in the bit layout the reference reads (dijkstra_invalidation.hpp:
//   152-190, graph_to_directions in common.h).  `pairs` extends "same label" by a list of label pairs that belong together (the
//   supervoxels of an agglomerated segmentation); the list is NOT closed transitively.
//
// HBM-bound: label_bytes read and 4 bytes written per voxel.  A workgroup of four waves takes a tile of 64 x 8 x 4 voxels; the tile
// and its one-voxel apron are read once, coalesced, into LDS (cells outside the array hold 0 and are masked by position, never by
// value: every label value is legal).  A wave owns one z plane of the tile, a lane one x, and walks the 8 rows in y with the 3 x 3 x 3
// values around its voxel in registers: 9 LDS reads per voxel, the other 18 carried over from the rows before.  Every voxel writes
// its own word once: no atomics.  With `pairs` only the steps whose two values differ and are both non-zero are searched, once per
// DISTINCT other value of a voxel (the 26 neighbours see very few) and not at all when it is the pair looked up last, which stays in
// registers with its verdict; the table is staged in LDS up to KH_GRAPH_LDS_PAIRS rows, beyond it is searched in global memory,
// where the L2 holds it.
#include "common.h"

namespace kh {

constexpr int VG_TX = 64, VG_TY = 8, VG_TZ = 4;                          // voxels of a tile
constexpr int VG_AX = VG_TX + 2, VG_AY = VG_TY + 2, VG_AZ = VG_TZ + 2;   // with the apron
constexpr int VG_CELLS = VG_AX * VG_AY * VG_AZ;                          // 3 960 cells: 31 680 B of 8-byte labels
constexpr int VG_LDS_PAIRS = KH_GRAPH_LDS_PAIRS;                         // 2 048 rows: 32 768 B; with the tile below the 64 KiB of static LDS
static_assert(VG_CELLS * 8 + VG_LDS_PAIRS * 16 <= 65536, "tile and staged pairs exceed the static LDS of a workgroup");

// the bits of a graph word whose step has component `sign` (-1 / +1) along `axis`
constexpr uint32_t vg_side_mask(int axis, int sign) {
  uint32_t m = 0;
  for (int b = 0; b < 26; b++) {
    int d[3] = {0, 0, 0};
    dir_delta(graph_bit_direction(b), d[0], d[1], d[2]);
    if (d[axis] == sign) m |= 1u << b;
  }
  return m;
}
// graph_bit_direction is the inverse of graph_to_directions' table: bit b of the word <-> bit graph_bit_direction(b) of the direction word
constexpr bool vg_tables_agree() {
  constexpr int BIT[26] = {1, 0, 3, 2, 5, 4, 9, 7, 8, 6, 17, 13, 16, 12, 15, 11, 14, 10, 25, 24, 23, 21, 22, 20, 19, 18};
  for (int i = 0; i < 26; i++)
    if (graph_bit_direction(BIT[i]) != i) return false;
  return true;
}
static_assert(vg_tables_agree(), "graph_bit_direction does not invert graph_to_directions");
static_assert(vg_side_mask(0, 1) == 0x1544541u && vg_side_mask(2, -1) == 0x3C3C020u, "cc3d's layout: +x bits, -z bits");

// the tile cell of the neighbour that bit b names, relative to the voxel's own cell, for a b known at run time only: the 26 steps
// packed two bits per component (0 -> -1, 1 -> 0, 2 -> +1)
constexpr uint64_t vg_packed_steps(int axis) {
  uint64_t p = 0;
  for (int b = 0; b < 26; b++) {
    int d[3] = {0, 0, 0};
    dir_delta(graph_bit_direction(b), d[0], d[1], d[2]);
    p |= (uint64_t)(d[axis] + 1) << (2 * b);
  }
  return p;
}
__device__ __forceinline__ int vg_cell_offset(int b) {
  constexpr uint64_t PX = vg_packed_steps(0), PY = vg_packed_steps(1), PZ = vg_packed_steps(2);
  const int dx = (int)((PX >> (2 * b)) & 3) - 1, dy = (int)((PY >> (2 * b)) & 3) - 1, dz = (int)((PZ >> (2 * b)) & 3) - 1;
  return dx + VG_AX * dy + VG_AX * VG_AY * dz;
}

// is the row (lo, hi) in the table of `n` rows, sorted lexicographically, unique
template <typename P>
__device__ __forceinline__ bool vg_pair_listed(P pairs, int64_t n, uint64_t lo, uint64_t hi) {
  int64_t a = 0, b = n;                            // the first row that is not below (lo, hi)
  while (a < b) {
    const int64_t m = (a + b) >> 1;
    const uint64_t pl = pairs[2 * m], ph = pairs[2 * m + 1];
    if (pl < lo || (pl == lo && ph < hi)) a = m + 1; else b = m;
  }
  return a < n && pairs[2 * a] == lo && pairs[2 * a + 1] == hi;
}

// MODE 0: no pairs; 1: the table staged in LDS (npairs <= VG_LDS_PAIRS); 2: the table in global memory
template <typename LT, int MODE>
__global__ __launch_bounds__(256) void voxel_graph_kernel(const LT* __restrict__ lab, int sx, int sy, int sz, uint32_t allowed,
                                                          const uint64_t* __restrict__ pairs, int64_t npairs,
                                                          uint32_t* __restrict__ out) {
  __shared__ LT tile[VG_CELLS];
  __shared__ uint64_t spairs[MODE == 1 ? 2 * VG_LDS_PAIRS : 2];
  const int tid = threadIdx.x;
  if (MODE == 1)
    for (int i = tid; i < 2 * (int)npairs; i += 256) spairs[i] = pairs[i];
  const int ntx = (sx + VG_TX - 1) / VG_TX, nty = (sy + VG_TY - 1) / VG_TY, ntz = (sz + VG_TZ - 1) / VG_TZ;
  const int64_t ntiles = (int64_t)ntx * nty * ntz;
  const int64_t sxy = (int64_t)sx * sy;
  const int lx = tid & 63, lz = tid >> 6;          // a lane's x and its wave's z plane in the tile
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int x0 = (int)(t % ntx) * VG_TX;
    const int64_t r = t / ntx;
    const int y0 = (int)(r % nty) * VG_TY, z0 = (int)(r / nty) * VG_TZ;
    __syncthreads();                               // the tile's readers of the turn before are through (first turn: spairs is written)
    // (cell by cell over the whole workgroup: filling row by row, a wave per row of 66 with a two-lane tail, measured 23 % slower)
    for (int c = tid; c < VG_CELLS; c += 256) {
      const int cx = c % VG_AX, cy = (c / VG_AX) % VG_AY, cz = c / (VG_AX * VG_AY);
      const int gx = x0 - 1 + cx, gy = y0 - 1 + cy, gz = z0 - 1 + cz;
      LT v = 0;
      if (gx >= 0 && gy >= 0 && gz >= 0 && gx < sx && gy < sy && gz < sz) v = lab[gx + (int64_t)sx * gy + sxy * gz];
      tile[c] = v;
    }
    __syncthreads();
    const int x = x0 + lx, z = z0 + lz;
    if (x >= sx || z >= sz) continue;              // (no barrier below this line inside the turn)
    uint32_t inside = allowed;
    if (x == 0) inside &= ~vg_side_mask(0, -1);
    if (x == sx - 1) inside &= ~vg_side_mask(0, 1);
    if (z == 0) inside &= ~vg_side_mask(2, -1);
    if (z == sz - 1) inside &= ~vg_side_mask(2, 1);
    // w[j][k][i]: the value at (x - 1 + i, y - 1 + j, z - 1 + k)
    LT w[3][3][3];
    const LT* base = tile + lx + VG_AX * VG_AY * lz;   // the cell of (x - 1, y0 - 1, z - 1)
#pragma unroll
    for (int j = 1; j < 3; j++)
#pragma unroll
      for (int k = 0; k < 3; k++)
#pragma unroll
        for (int i = 0; i < 3; i++) w[j][k][i] = base[i + VG_AX * (j - 1) + VG_AX * VG_AY * k];
    uint64_t seen_lo = 0, seen_hi = 0;             // the pair looked up last (0, 0: none -- a pair never names 0) and its verdict
    bool seen = false;
#pragma unroll
    for (int ly = 0; ly < VG_TY; ly++) {
      const int y = y0 + ly;
      if (y >= sy) break;
#pragma unroll
      for (int k = 0; k < 3; k++)
#pragma unroll
        for (int i = 0; i < 3; i++) {
          w[0][k][i] = w[1][k][i];
          w[1][k][i] = w[2][k][i];
          w[2][k][i] = base[i + VG_AX * (ly + 2) + VG_AX * VG_AY * k];
        }
      uint32_t mask = inside;
      if (y == 0) mask &= ~vg_side_mask(1, -1);
      if (y == sy - 1) mask &= ~vg_side_mask(1, 1);
      const LT L = w[1][1][1];
      uint32_t g = 0;
#pragma unroll
      for (int b = 0; b < 26; b++) {
        int dx = 0, dy = 0, dz = 0;
        dir_delta(graph_bit_direction(b), dx, dy, dz);
        g |= (uint32_t)(w[1 + dy][1 + dz][1 + dx] == L) << b;
      }
      g &= mask;
      if (MODE != 0 && L != 0) {
        uint32_t filled = 0;
#pragma unroll
        for (int b = 0; b < 26; b++) {
          int dx = 0, dy = 0, dz = 0;
          dir_delta(graph_bit_direction(b), dx, dy, dz);
          filled |= (uint32_t)(w[1 + dy][1 + dz][1 + dx] != 0) << b;
        }
        // the steps inside the array whose two values differ and are both non-zero; one turn per DISTINCT other value -- the wave
        // runs as many searches as its neediest lane sees values, not one per step.  The value of a step chosen at run time comes
        // from the tile (it is still there: the next barrier is the next turn's), the comparisons from the registers.
        uint32_t open = mask & ~g & filled;
        const LT* centre = base + 1 + VG_AX * (ly + 1) + VG_AX * VG_AY;
        while (open) {
          const int first = __ffs((int)open) - 1;
          const LT N = centre[vg_cell_offset(first)];
          uint32_t same = 1u << first;
#pragma unroll
          for (int b = 0; b < 26; b++) {
            int dx = 0, dy = 0, dz = 0;
            dir_delta(graph_bit_direction(b), dx, dy, dz);
            same |= (uint32_t)(w[1 + dy][1 + dz][1 + dx] == N) << b;
          }
          same &= open | (1u << first);
          const uint64_t lo = L < N ? (uint64_t)L : (uint64_t)N, hi = L < N ? (uint64_t)N : (uint64_t)L;
          if (lo != seen_lo || hi != seen_hi) {
            seen = MODE == 1 ? vg_pair_listed(spairs, npairs, lo, hi) : vg_pair_listed(pairs, npairs, lo, hi);
            seen_lo = lo;
            seen_hi = hi;
          }
          if (seen) g |= same;
          open &= ~same;                           // (at least the bit `first`: the loop ends after 26 turns at the most)
        }
      }
      out[x + (int64_t)sx * y + sxy * z] = g;
    }
  }
}

template <typename LT>
static int voxel_graph_launch(const void* labels, int sx, int sy, int sz, uint32_t allowed, const uint64_t* pairs, int64_t npairs,
                              uint32_t* graph, hipStream_t st) {
  const int64_t ntiles = (int64_t)((sx + VG_TX - 1) / VG_TX) * ((sy + VG_TY - 1) / VG_TY) * ((sz + VG_TZ - 1) / VG_TZ);
  const dim3 grid((unsigned)(ntiles < (1 << 20) ? ntiles : (1 << 20))), block(256);
  if (npairs == 0)
    hipLaunchKernelGGL((voxel_graph_kernel<LT, 0>), grid, block, 0, st, (const LT*)labels, sx, sy, sz, allowed, pairs, npairs, graph);
  else if (npairs <= VG_LDS_PAIRS)
    hipLaunchKernelGGL((voxel_graph_kernel<LT, 1>), grid, block, 0, st, (const LT*)labels, sx, sy, sz, allowed, pairs, npairs, graph);
  else
    hipLaunchKernelGGL((voxel_graph_kernel<LT, 2>), grid, block, 0, st, (const LT*)labels, sx, sy, sz, allowed, pairs, npairs, graph);
  KH_LAUNCH_CHECK();
  return KH_OK;
}

}  // namespace kh

using namespace kh;

extern "C" int kh_voxel_graph(const void* labels, int label_bytes, int64_t sx, int64_t sy, int64_t sz, int connectivity,
                              const uint64_t* pairs, int64_t npairs, uint32_t* graph, void* stream) {
  if (int rc = require_device()) return rc;
  if (!labels || !graph || sx <= 0 || sy <= 0 || sz <= 0 || npairs < 0 || (npairs > 0 && !pairs)) {
    set_error("kh_voxel_graph: bad arguments");
    return KH_EINVAL;
  }
  if (sx >= (1ll << 32) || sy >= (1ll << 32) || sz >= (1ll << 32) || sx * sy >= (1ll << 32) || sx * sy * sz >= (1ll << 32)) {
    set_error("kh_voxel_graph: fewer than 2^32 voxels");
    return KH_EINVAL;
  }
  if (sx >= (1ll << 31) || sy >= (1ll << 31) || sz >= (1ll << 31) || npairs >= (1ll << 31)) {
    set_error("kh_voxel_graph: an extent or the pair table has 2^31 entries or more");
    return KH_EINVAL;
  }
  if (connectivity != 6 && connectivity != 18 && connectivity != 26) {
    set_error("kh_voxel_graph: connectivity must be 6, 18 or 26");
    return KH_EINVAL;
  }
  const uint32_t allowed = connectivity == 6 ? 0x3Fu : connectivity == 18 ? 0x3FFFFu : 0x3FFFFFFu;
  if (!pairs) npairs = 0;
  hipStream_t st = (hipStream_t)stream;
  switch (label_bytes) {
    case 1: return voxel_graph_launch<uint8_t>(labels, (int)sx, (int)sy, (int)sz, allowed, pairs, npairs, graph, st);
    case 2: return voxel_graph_launch<uint16_t>(labels, (int)sx, (int)sy, (int)sz, allowed, pairs, npairs, graph, st);
    case 4: return voxel_graph_launch<uint32_t>(labels, (int)sx, (int)sy, (int)sz, allowed, pairs, npairs, graph, st);
    case 8: return voxel_graph_launch<uint64_t>(labels, (int)sx, (int)sy, (int)sz, allowed, pairs, npairs, graph, st);
    default: set_error("kh_voxel_graph: label_bytes must be 1, 2, 4 or 8"); return KH_EINVAL;
  }
}
