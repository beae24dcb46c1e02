// backtrack.h -- the predecessor walk that turns a distance field into a path (pred_edge, backtrack<RAILS>).
// Needs search_state.h (NONE64, pack, ld_f32_l2) and common.h.
#pragma once
#include "search_state.h"

namespace kh {

// wave 0 only: canonical predecessor walk (oracle ko_walk).  Writes the path (start first) to out[0..];
// returns its length (0 on failure).
//   - normally pred(v) = the achieving neighbour (fl(d[u] + f[v]) == d[v]) with d[u] < d[v] minimising (d[u], index);
//   - at the rail end of a railroad (f == 0) every achieving neighbour has d[u] == d[v]: smallest index;
//   - float-absorption plateau (all achieving neighbours have d[u] == d[v]): breadth-first search over the
//     equal-distance achieving neighbours (FIFO, neighbours in direction order) to the first voxel that is
//     `target` (the search's source: zero weights around it make a plateau at distance 0 that nothing lies
//     below) or has a strictly smaller achieving predecessor; the BFS route is followed.  bq / bpar: scratch
//     lists (>= Nf entries), visited marks live in bit 4 of the label's own qstate bytes.
// With a voxel graph (kh_apply_voxel_graph) the masks are one-way: bit k of nbrmask[v] says "a step FROM v in direction k is
// allowed".  A predecessor u of v needs the step u -> v, i.e. the bit of the OPPOSITE direction in u's word; without a graph
// the masks are symmetric and v's own word serves (one load less per step).
__device__ __forceinline__ bool pred_edge(const Geometry& g, const uint32_t* __restrict__ nbrmask, uint32_t v, int lane, bool graph) {
  if (lane >= 26) return false;
  if (!graph) return ((nbrmask[v] >> lane) & 1u) != 0u;
  int dx, dy, dz;
  dir_delta(lane, dx, dy, dz);
  const uint32_t sx = (uint32_t)g.sx, sxy = (uint32_t)g.sxy;
  const uint32_t z = v / sxy, r = v - z * sxy, y = r / sx, x = r - y * sx;
  const int nx = (int)x + dx, ny = (int)y + dy, nz = (int)z + dz;
  if (nx < 0 || ny < 0 || nz < 0 || nx >= g.sx || ny >= g.sy || nz >= g.sz) return false;
  // the opposite direction: the table of common.h lists every direction next to its opposite (0/1, 2/3, ... are pairs by
  // construction for the faces; looked up by offset for the rest)
  int opp = 0;
#pragma unroll
  for (int j = 0; j < 26; j++) {
    int ex, ey, ez;
    dir_delta(j, ex, ey, ez);
    if (ex == -dx && ey == -dy && ez == -dz) opp = j;
  }
  const uint32_t u = v + (uint32_t)g.off[lane];
  return ((nbrmask[u] >> opp) & 1u) != 0u;
}

template <bool RAILS>
__device__ __attribute__((noinline)) uint32_t backtrack(const Geometry& g, const uint32_t* __restrict__ nbrmask,
                                                        const float* __restrict__ pdrf, const float* dist,
                                                        uint32_t rail_end, uint32_t target, uint32_t* out, uint32_t cap,
                                                        uint32_t* bq, uint32_t* bpar, uint32_t bcap, uint8_t* qstate,
                                                        uint32_t* status, bool graph = false) {
  const int lane = threadIdx.x & 63;
  const unsigned long long below = (1ull << lane) - 1ull;
  uint32_t v = rail_end, n = 0;
  if (lane == 0) out[0] = v;
  n = 1;
  while (v != target) {
    const float dv = ld_f32_l2(&dist[v]);
    const float fv = pdrf[v];
    const bool at_rail_end = RAILS && v == rail_end;
    unsigned long long key = NONE64;
    if (pred_edge(g, nbrmask, v, lane, graph)) {
      const uint32_t u = v + (uint32_t)g.off[lane];
      const float fu = pdrf[u];
      if (!RAILS || fu != 0.0f) {
        const float du = ld_f32_l2(&dist[u]);
        if (du != KH_INF && du + fv == dv && (at_rail_end || du < dv)) key = pack(du, u);
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const unsigned long long ok = __shfl_xor(key, o);
      if (ok < key) key = ok;
    }
    if (key != NONE64) {
      if (n >= cap) { if (lane == 0) atomicOr(status, KH_ST_PATH_OVERFLOW); return 0; }
      v = (uint32_t)key;
      if (lane == 0) out[n] = v;
      n++;
      continue;
    }
    if (at_rail_end) { if (lane == 0) atomicOr(status, KH_ST_NO_RAIL); return 0; }
    // ---- plateau search
    uint32_t head = 0, tail = 1, found = 0xFFFFFFFFu;
    if (lane == 0) { bq[0] = v; bpar[0] = 0xFFFFFFFFu; qstate[v] |= 0x10; }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    while (head < tail) {
      const uint32_t x = bq[head];
      const float dx = ld_f32_l2(&dist[x]);
      const float fx = pdrf[x];
      bool strict = false, equal = false;
      uint32_t u = 0;
      if (pred_edge(g, nbrmask, x, lane, graph)) {
        u = x + (uint32_t)g.off[lane];
        const float fu = pdrf[u];
        if (!RAILS || fu != 0.0f) {
          const float du = ld_f32_l2(&dist[u]);
          if (du != KH_INF && du + fx == dx) {
            strict = du < dx;
            equal = (du == dx) && !(qstate[u] & 0x10);
          }
        }
      }
      if (head > 0 && (x == target || __ballot(strict))) { found = head; break; }
      const unsigned long long em = __ballot(equal);
      const uint32_t cnt = (uint32_t)__popcll(em);
      if (tail + cnt > bcap) { found = 0xFFFFFFFFu; head = tail; break; }
      if (equal) {
        const uint32_t p = tail + (uint32_t)__popcll(em & below);
        bq[p] = u;
        bpar[p] = head;
        qstate[u] |= 0x10;
      }
      tail += cnt;
      head++;
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    }
    for (uint32_t i = lane; i < tail; i += 64) qstate[bq[i]] &= (uint8_t)~0x10;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    if (found == 0xFFFFFFFFu) { if (lane == 0) atomicOr(status, KH_ST_PLATEAU); return 0; }
    // route v -> ... -> bq[found] (the BFS tree, backwards), appended forwards
    uint32_t len = 0;
    for (uint32_t i = found; i != 0; i = bpar[i]) len++;
    if (n + len > cap) { if (lane == 0) atomicOr(status, KH_ST_PATH_OVERFLOW); return 0; }
    if (lane == 0) {
      uint32_t pos = n + len - 1;
      for (uint32_t i = found; i != 0; i = bpar[i]) out[pos--] = bq[i];
    }
    n += len;
    v = bq[found];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  }
  return n;
}

}  // namespace kh
