// join.hip -- the nearest vertex pairs between the parts of a skeleton group (gfx950) and the merge plan that
// reads them.
//
//   kh_part_gaps        for every ordered pair (tree part t, query part q) of a group the record R[t][q] = lexicographic minimum of
//                       (d2, kq, kt) over the vertices of both -- what kimimaro/post.py:89-218 asks of one cKDTree per part, again
//                       after every merge, computed once for all original parts of all groups.
//   kh_host_join_plan   host C, no GPU: the merge sequence of join_close_components on one group, reading only that table.
//   kh_part_clusters    the broad phase in front of both: the sets of parts of a group that are connected through pairs of boxes
//                       nearer than the bound.  No record and no merge crosses two of them, so each is a join of its own.
//
// One workgroup per unordered pair.  A lane owns a vertex of the larger part ("own" side, 256 per slab) and walks the other part in
// ascending index from LDS tiles -- every lane reads the same address, a broadcast -- keeping with a strict < its nearest other
// vertex of smallest index.  That one result serves both orientations: own side as query orders by (d2, own, other), own side as tree
// by (d2, other, own); every distance is evaluated once.  Keys are 128 bits: they are reduced in registers, across the wave with
// shuffles, across the four waves through LDS, and each record is written once by one lane -- no global atomics.
#include "common.h"
#include "unionfind.h"

#include <math.h>

#include <new>
#include <vector>

namespace kh {

static constexpr unsigned long long GAP_INF = 0x7FF0000000000000ull;    // the bits of +inf
static constexpr uint32_t GAP_NONE = 0xFFFFFFFFu;
static constexpr int64_t GAP_MAX_RECORDS = 1ll << 26;                   // 16 bytes each: 1 GiB of tables per call

struct GapKey {
  unsigned long long d2;      // bits of the non-negative f64 (they order like the values)
  unsigned long long ix;      // (first index << 32) | second index
};

__device__ __forceinline__ bool gap_less(const GapKey& a, const GapKey& b) { return a.d2 < b.d2 || (a.d2 == b.d2 && a.ix < b.ix); }

__device__ __forceinline__ GapKey gap_wave_min(GapKey k) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    GapKey o;
    o.d2 = __shfl_xor(k.d2, d);
    o.ix = __shfl_xor(k.ix, d);
    if (gap_less(o, k)) k = o;
  }
  return k;
}

// squared distance of two intervals / of a point and an interval along one axis, as the f64 difference the vertex loop would form
__device__ __forceinline__ double axis_gap(double lo_a, double hi_a, double lo_b, double hi_b) {
  const double g1 = lo_a - hi_b, g2 = lo_b - hi_a;
  const double g = g1 > g2 ? g1 : g2;
  return g > 0.0 ? g : 0.0;
}

// a lower bound of every d2 between the vertices of two parts, from their boxes (min x, y, z, max x, y, z), formed with the operations
// of the vertex loop (differences, squares and sums of f64 are monotone).  The ONE statement of it: part_gaps_kernel culls a pair on
// box_gap2 >= bound2, part_clusters_kernel calls a pair near on box_gap2 < bound2, so "near" covers "has a record" by construction.
__device__ __forceinline__ double box_gap2(const float* a, const float* b) {
  const double gx = axis_gap(a[0], a[3], b[0], b[3]), gy = axis_gap(a[1], a[4], b[1], b[4]), gz = axis_gap(a[2], a[5], b[2], b[5]);
  return (gx * gx + gy * gy) + gz * gz;
}

__device__ __forceinline__ void gap_store(unsigned long long* rec_d2, uint32_t* rec_idx, int64_t cell, unsigned long long d2, uint32_t kt,
                                          uint32_t kq, double bound2) {
  const bool some = __longlong_as_double((long long)d2) < bound2;
  rec_d2[cell] = some ? d2 : GAP_INF;
  rec_idx[2 * cell + 0] = some ? kt : GAP_NONE;
  rec_idx[2 * cell + 1] = some ? kq : GAP_NONE;
}

__global__ __launch_bounds__(256) void part_gaps_kernel(const float* __restrict__ xyz, const uint32_t* __restrict__ part_start,
                                                        const float* __restrict__ part_box, const uint32_t* __restrict__ group_start,
                                                        const double* __restrict__ bound2, const int64_t* __restrict__ rec_start,
                                                        int ngroups, unsigned long long* __restrict__ rec_d2,
                                                        uint32_t* __restrict__ rec_idx) {
  __shared__ double tx[256], ty[256], tz[256];
  __shared__ GapKey red[2][4];
  const int tid = (int)threadIdx.x;
  const int64_t cell = (int64_t)blockIdx.x;
  int lo = 0, hi = ngroups - 1;               // the group of this cell: the first g with rec_start[g + 1] > cell
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (rec_start[mid + 1] <= cell) lo = mid + 1; else hi = mid;
  }
  const int g = lo;
  const uint32_t p0 = group_start[g];
  const int64_t n = (int64_t)(group_start[g + 1] - p0);
  const int64_t base = rec_start[g];
  const int64_t local = cell - base;
  if (n <= 0 || local < 0 || local >= n * n) return;
  const int64_t t = local / n, q = local % n;
  if (t > q) return;                          // the workgroup of (q, t) writes both orientations
  const double b2 = bound2[g];
  if (t == q) {
    if (tid == 0) gap_store(rec_d2, rec_idx, cell, GAP_INF, GAP_NONE, GAP_NONE, b2);
    return;
  }
  const uint32_t st = part_start[p0 + t], sq = part_start[p0 + q];
  const uint32_t nt = part_start[p0 + t + 1] - st, nq = part_start[p0 + q + 1] - sq;
  const bool own_is_t = nt >= nq;             // lanes go to the larger part
  const int64_t X = own_is_t ? t : q, Y = own_is_t ? q : t;
  const uint32_t sX = own_is_t ? st : sq, sY = own_is_t ? sq : st;
  const uint32_t nX = own_is_t ? nt : nq, nY = own_is_t ? nq : nt;
  const int64_t cell_own_query = base + Y * n + X;     // R[Y][X]: the own side asks, the other part is the tree
  const int64_t cell_own_tree = base + X * n + Y;      // R[X][Y]
  const float* bx = part_box + 6 * (size_t)(p0 + X);
  const float* by = part_box + 6 * (size_t)(p0 + Y);
  const double ylo0 = by[0], ylo1 = by[1], ylo2 = by[2], yhi0 = by[3], yhi1 = by[4], yhi2 = by[5];
  {
    // at or above the bound the pair has no record
    if (box_gap2(bx, by) >= b2) {
      if (tid == 0) {
        gap_store(rec_d2, rec_idx, cell_own_query, GAP_INF, GAP_NONE, GAP_NONE, b2);
        gap_store(rec_d2, rec_idx, cell_own_tree, GAP_INF, GAP_NONE, GAP_NONE, b2);
      }
      return;
    }
  }
  GapKey as_query = {GAP_INF, ~0ull};         // (d2, own, other)
  GapKey as_tree = {GAP_INF, ~0ull};          // (d2, other, own)
  for (uint32_t s = 0; s < nX; s += 256) {
    const uint32_t own = s + (uint32_t)tid;
    const bool have = own < nX;
    double ox = 0.0, oy = 0.0, oz = 0.0;
    if (have) {
      const float* v = xyz + 3 * (size_t)(sX + own);
      ox = v[0];
      oy = v[1];
      oz = v[2];
    }
    // a slab none of whose vertices comes within the bound of the other part's box holds no record (>= bound: none)
    const double gx = axis_gap(ox, ox, ylo0, yhi0), gy = axis_gap(oy, oy, ylo1, yhi1), gz = axis_gap(oz, oz, ylo2, yhi2);
    const bool near = have && ((gx * gx + gy * gy) + gz * gz) < b2;
    if (!__syncthreads_or(near)) continue;
    double bd = __longlong_as_double((long long)GAP_INF);
    uint32_t bo = GAP_NONE;
    for (uint32_t y0 = 0; y0 < nY; y0 += 256) {
      __syncthreads();                        // the previous tile has been read by everyone
      if (y0 + (uint32_t)tid < nY) {
        const float* v = xyz + 3 * (size_t)(sY + y0 + (uint32_t)tid);
        tx[tid] = v[0];
        ty[tid] = v[1];
        tz[tid] = v[2];
      }
      __syncthreads();
      const int m = (int)((nY - y0) < 256u ? (nY - y0) : 256u);
#pragma unroll 4
      for (int j = 0; j < m; j++) {
        const double dx = ox - tx[j], dy = oy - ty[j], dz = oz - tz[j];
        const double d2 = (dx * dx + dy * dy) + dz * dz;
        if (d2 < bd) {                        // strict: among equally near ones the smallest index stays
          bd = d2;
          bo = y0 + (uint32_t)j;
        }
      }
    }
    if (have && bo != GAP_NONE) {
      const unsigned long long bits = (unsigned long long)__double_as_longlong(bd);
      const GapKey kq = {bits, ((unsigned long long)own << 32) | bo};
      const GapKey kt = {bits, ((unsigned long long)bo << 32) | own};
      if (gap_less(kq, as_query)) as_query = kq;
      if (gap_less(kt, as_tree)) as_tree = kt;
    }
  }
  as_query = gap_wave_min(as_query);
  as_tree = gap_wave_min(as_tree);
  __syncthreads();
  if ((tid & 63) == 0) {
    red[0][tid >> 6] = as_query;
    red[1][tid >> 6] = as_tree;
  }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < 4; w++) {
      if (gap_less(red[0][w], as_query)) as_query = red[0][w];
      if (gap_less(red[1][w], as_tree)) as_tree = red[1][w];
    }
    // (kt, kq): own side as query -> (other, own); own side as tree -> (own, other) = the low and high words of its (other, own) key
    gap_store(rec_d2, rec_idx, cell_own_query, as_query.d2, (uint32_t)as_query.ix, (uint32_t)(as_query.ix >> 32), b2);
    gap_store(rec_d2, rec_idx, cell_own_tree, as_tree.d2, (uint32_t)as_tree.ix, (uint32_t)(as_tree.ix >> 32), b2);
  }
}

// ---- the broad phase: connected sets of near parts ----------------------------------------------------------------
// The union-find of unionfind.h, whose parent array IS the output.  Its CAS words are the only global atomics of this file: 32-bit
// integers, one successful CAS per true union, and no floating-point value goes through them.
__global__ __launch_bounds__(256) void part_clusters_init_kernel(uint32_t* __restrict__ cluster, uint32_t nparts) {
  const uint32_t p = blockIdx.x * 256u + threadIdx.x;
  if (p < nparts) cluster[p] = p;
}

// One wave per position s of `order`; its part i = order[s] is tested against the parts at the later positions of its group, lanes
// strided over them.  lo along the sweep axis ascends with the position, so the first candidate j with g1 = lo_j - hi_i > 0 and
// g1 * g1 >= bound2 ends the scan: for every later one g1 is no smaller, the axis term of box_gap2 is max(g1, .) squared, and the
// sum of box_gap2 is no smaller than that term (the same f64 operations, all monotone) -- none of them is near.
__global__ __launch_bounds__(256) void part_clusters_kernel(const float* __restrict__ part_box, const uint32_t* __restrict__ group_start,
                                                            const double* __restrict__ bound2, const uint32_t* __restrict__ order,
                                                            int ngroups, uint32_t nparts, int axis, uint32_t* cluster) {
  const uint32_t s = blockIdx.x * 4u + (threadIdx.x >> 6);
  const uint32_t lane = threadIdx.x & 63u;
  if (s >= nparts) return;
  int lo = 0, hi = ngroups - 1;               // the group of this position: the first g with group_start[g + 1] > s
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (group_start[mid + 1] <= s) lo = mid + 1; else hi = mid;
  }
  const uint32_t p0 = group_start[lo];
  uint32_t p1 = group_start[lo + 1];
  if (p1 > nparts) p1 = nparts;
  if (s < p0 || s >= p1) return;
  const uint32_t i = order[s];
  if (i < p0 || i >= p1) return;              // not a part of this group: `order` is no permutation within the groups
  const double b2 = bound2[lo];
  const float* bi = part_box + 6 * (size_t)i;
  const double hi_i = bi[3 + axis];
  for (uint32_t base = s + 1; base < p1; base += 64u) {
    const uint32_t c = base + lane;
    bool stop = false;
    if (c < p1) {
      const uint32_t j = order[c];
      if (j >= p0 && j < p1 && j != i) {
        const float* bj = part_box + 6 * (size_t)j;
        const double g1 = (double)bj[axis] - hi_i;
        stop = g1 > 0.0 && g1 * g1 >= b2;
        if (!stop && box_gap2(bi, bj) < b2) uf_unite(cluster, i, j);
      }
    }
    if (__any(stop)) break;
  }
}

__global__ __launch_bounds__(256) void part_clusters_flatten_kernel(uint32_t* cluster, uint32_t nparts) {
  const uint32_t p = blockIdx.x * 256u + threadIdx.x;
  if (p >= nparts) return;
  uint32_t x = p;
  for (;;) {                                  // read only: another lane may be storing the root of x into cluster[x] right now,
    const uint32_t up = uf_load(cluster, x);  // which is an ancestor of x like the word it replaces
    if (up == x) break;
    x = up;
  }
  __hip_atomic_store(cluster + p, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace kh

using namespace kh;

extern "C" int kh_part_clusters(const float* part_box, const uint32_t* group_start, const double* bound2, const uint32_t* order,
                                int64_t ngroups, int64_t nparts, int axis, uint32_t* cluster, void* stream) {
  if (int rc = require_device()) return rc;
  if (ngroups < 0 || ngroups >= (1ll << 31) || nparts < 0 || nparts >= (1ll << 31) || axis < 0 || axis > 2) {
    set_error("kh_part_clusters: 0 <= ngroups < 2^31, 0 <= nparts < 2^31, axis 0, 1 or 2");
    return KH_EINVAL;
  }
  if (ngroups == 0 || nparts == 0) return KH_OK;
  if (!part_box || !group_start || !bound2 || !order || !cluster) {
    set_error("kh_part_clusters: null pointer");
    return KH_EINVAL;
  }
  const unsigned n = (unsigned)nparts;
  hipLaunchKernelGGL(part_clusters_init_kernel, dim3((n + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, cluster, n);
  KH_LAUNCH_CHECK();
  hipLaunchKernelGGL(part_clusters_kernel, dim3((n + 3u) / 4u), dim3(256), 0, (hipStream_t)stream, part_box, group_start, bound2, order,
                     (int)ngroups, n, axis, cluster);
  KH_LAUNCH_CHECK();
  hipLaunchKernelGGL(part_clusters_flatten_kernel, dim3((n + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, cluster, n);
  KH_LAUNCH_CHECK();
  return KH_OK;
}

extern "C" int kh_part_gaps(const float* xyz, const uint32_t* part_start, const float* part_box, const uint32_t* group_start,
                            const double* bound2, const int64_t* rec_start, int64_t ngroups, int64_t nrecords, uint64_t* rec_d2,
                            uint32_t* rec_idx, void* stream) {
  if (int rc = require_device()) return rc;
  if (ngroups < 0 || ngroups >= (1ll << 31) || nrecords < 0 || nrecords > GAP_MAX_RECORDS) {
    set_error("kh_part_gaps: 0 <= ngroups < 2^31, 0 <= nrecords <= 2^26 (1 GiB of tables)");
    return KH_EINVAL;
  }
  if (ngroups == 0 || nrecords == 0) return KH_OK;
  if (!xyz || !part_start || !part_box || !group_start || !bound2 || !rec_start || !rec_d2 || !rec_idx) {
    set_error("kh_part_gaps: null pointer");
    return KH_EINVAL;
  }
  hipLaunchKernelGGL(part_gaps_kernel, dim3((unsigned)nrecords), dim3(256), 0, (hipStream_t)stream, xyz, part_start, part_box, group_start,
                     bound2, rec_start, (int)ngroups, (unsigned long long*)rec_d2, rec_idx);
  KH_LAUNCH_CHECK();
  return KH_OK;
}

// ---- the merge plan ----------------------------------------------------------------------------------------------
namespace {

struct Member {
  uint32_t part, offset;
};

struct Gap {
  float key;            // np.float32(d), +inf for "none" and for a pair the radius-sum test rejects
  uint32_t ka, kb;      // the edge in the numbering of the concatenated parts
};

struct Plan {
  int64_t n;
  const uint32_t* size;
  const uint64_t* d2;
  const uint32_t* idx;
  const float* radii;
  bool restrict_by_radius;
  std::vector<uint32_t> first;               // first vertex of every part in the concatenated numbering
  std::vector<std::vector<Member>> cluster;  // by slot; a fused cluster takes the slot of its first half

  Gap gap(uint32_t A, uint32_t B) const {    // cluster A as tree, cluster B as query
    double best = INFINITY;
    uint64_t bq = 0, bt = 0;
    uint32_t ea = 0, eb = 0;
    bool some = false;
    for (const Member& a : cluster[A])
      for (const Member& b : cluster[B]) {
        const int64_t c = (int64_t)a.part * n + b.part;
        double d;
        memcpy(&d, &d2[c], 8);
        if (!(d < INFINITY)) continue;
        const uint64_t kq = (uint64_t)idx[2 * c + 1] + b.offset, kt = (uint64_t)idx[2 * c + 0] + a.offset;
        if (!some || d < best || (d == best && (kq < bq || (kq == bq && kt < bt)))) {
          some = true;
          best = d;
          bq = kq;
          bt = kt;
          ea = first[a.part] + idx[2 * c + 0];
          eb = first[b.part] + idx[2 * c + 1];
        }
      }
    Gap out = {INFINITY, ea, eb};
    if (!some) return out;
    const double d = sqrt(best);
    if (restrict_by_radius) {
      const float sum = radii[ea] + radii[eb];      // float32, like a.radii[ka] + b.radii[kb]
      if (d > (double)sum) return out;
    }
    out.key = (float)d;
    return out;
  }
};

}  // namespace

extern "C" int64_t kh_host_join_plan(int64_t nparts, const uint32_t* part_size, const uint64_t* rec_d2, const uint32_t* rec_idx,
                                     const float* radii, double radius, int restrict_by_radius, uint32_t* edges) {
  if (nparts < 0 || nparts > 0xFFFFFFFFll) return -1;
  if (nparts < 2) return 0;
  if (!part_size || !rec_d2 || !rec_idx || !radii || !edges) return -1;
  try {
    Plan p;
    p.n = nparts;
    p.size = part_size;
    p.d2 = rec_d2;
    p.idx = rec_idx;
    p.radii = radii;
    p.restrict_by_radius = restrict_by_radius != 0;
    p.first.resize((size_t)nparts);
    uint64_t total = 0;
    for (int64_t i = 0; i < nparts; i++) {
      p.first[(size_t)i] = (uint32_t)total;
      total += part_size[i];
    }
    if (total > 0xFFFFFFFFull) return -1;
    for (int64_t t = 0; t < nparts; t++)
      for (int64_t q = 0; q < nparts; q++) {
        if (t == q) continue;
        const int64_t c = t * nparts + q;
        double d;
        memcpy(&d, &rec_d2[c], 8);
        if (!(d < INFINITY)) continue;
        if (rec_idx[2 * c + 0] >= part_size[t] || rec_idx[2 * c + 1] >= part_size[q]) return -1;
      }
    p.cluster.resize((size_t)nparts);
    std::vector<uint32_t> order((size_t)nparts), count((size_t)nparts);
    for (int64_t i = 0; i < nparts; i++) {
      p.cluster[(size_t)i].push_back(Member{(uint32_t)i, 0u});
      order[(size_t)i] = (uint32_t)i;
      count[(size_t)i] = part_size[i];
    }
    // key[a * n + b]: the gap key of slot a as tree and slot b as query, kept for a in front of b in the current order
    std::vector<float> key((size_t)nparts * (size_t)nparts, INFINITY);
    for (int64_t i = 0; i < nparts; i++)
      for (int64_t j = i + 1; j < nparts; j++) key[(size_t)(i * nparts + j)] = p.gap((uint32_t)i, (uint32_t)j).key;
    int64_t nedges = 0;
    while (order.size() > 1) {
      const size_t m = order.size();
      float best = INFINITY;
      size_t bi = 0, bj = 0;
      for (size_t i = 0; i < m; i++)
        for (size_t j = i + 1; j < m; j++) {
          const float k = key[(size_t)order[i] * (size_t)nparts + order[j]];
          if (k < best) {             // strict: the first (i, j) among equal keys
            best = k;
            bi = i;
            bj = j;
          }
        }
      if (!(best < INFINITY) || (double)best > radius) break;
      const uint32_t A = order[bi], B = order[bj];
      const Gap g = p.gap(A, B);
      edges[2 * nedges + 0] = g.ka;
      edges[2 * nedges + 1] = g.kb;
      nedges++;
      for (const Member& b : p.cluster[B]) p.cluster[A].push_back(Member{b.part, b.offset + count[A]});
      count[A] += count[B];
      p.cluster[B].clear();
      std::vector<uint32_t> next;
      next.reserve(m - 1);
      next.push_back(A);
      for (size_t i = 0; i < m; i++)
        if (i != bi && i != bj) next.push_back(order[i]);
      order.swap(next);
      for (size_t j = 1; j < order.size(); j++) key[(size_t)A * (size_t)nparts + order[j]] = p.gap(A, order[j]).key;
    }
    return nedges;
  } catch (const std::bad_alloc&) {
    return -2;
  }
}
