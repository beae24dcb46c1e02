// forest.hip -- the skeletons of a call packed back to back ("the forest"; gfx950): what kimimaro/post.py does to one
// skeleton at a time in Python loops over its vertices, for all skeletons of a call at once.
//
//   kh_forest_components   comp[v] = the smallest vertex connected to v: the union-find of unionfind.h on the edge list.
//   kh_forest_measure      per component, at its root: vertices, edges, cable length (f64 sum of the float32 edge lengths); per vertex:
//                          its degree.  The inputs of remove_dust and of the tree test (ne == nv - 1) of remove_loops / remove_ticks.
//   kh_forest_ticks        post._remove_ticks_component (kimimaro/post.py:262-362) for every listed tree, operation by operation.
//
// Atomics (every one is a fabric round trip).  The union-find's CAS words; one 32-bit add per edge end for the
// degrees; and for the sums per component ONE add per run of equal roots in a wave -- edges arrive sorted by their smaller vertex,
// so the lanes of a wave mostly hold one component or a few -- never one per edge.  The order in which the runs of a component reach
// its f64 sum is not fixed: remove_dust_many decides on the device only outside a band that covers every order.
// (Where the sum stays below 2^30 times the power of two at or below the smallest length, every partial sum is an exact f64 and the
// order cannot show: the tests pin the cable bit for bit on such inputs.)
// kh_forest_ticks uses none: a component belongs to one wave.
#include "common.h"
#include "unionfind.h"

#include <math.h>

namespace kh {

static constexpr uint32_t FOREST_NONE = 0xFFFFFFFFu;
static constexpr uint8_t SE_LIVE = 1, SE_REMOVABLE = 2;

// the length of an edge as Skeleton.cable_length and distance_graph form it: float32 differences, ((dx*dx) + (dy*dy)) + (dz*dz), the
// correctly rounded float32 root; no FMA (-ffp-contract=off).  Symmetric in its ends: a - b = -(b - a) exactly.
__device__ __forceinline__ float edge_length(const float* __restrict__ xyz, uint32_t a, uint32_t b) {
  const float* pa = xyz + 3 * (size_t)a;
  const float* pb = xyz + 3 * (size_t)b;
  const float dx = pb[0] - pa[0], dy = pb[1] - pa[1], dz = pb[2] - pa[2];
  return sqrtf(((dx * dx) + (dy * dy)) + (dz * dz));
}

// ---- components ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void forest_identity_kernel(uint32_t* __restrict__ comp, uint32_t nverts) {
  const uint32_t v = blockIdx.x * 256u + threadIdx.x;
  if (v < nverts) comp[v] = v;
}

__global__ __launch_bounds__(256) void forest_union_kernel(const uint32_t* __restrict__ edges, uint32_t nedges, uint32_t nverts,
                                                           uint32_t* comp) {
  const uint32_t e = blockIdx.x * 256u + threadIdx.x;
  if (e >= nedges) return;
  const uint32_t a = edges[2 * (size_t)e], b = edges[2 * (size_t)e + 1];
  if (a < nverts && b < nverts && a != b) uf_unite(comp, a, b);
}

__global__ __launch_bounds__(256) void forest_flatten_kernel(uint32_t* comp, uint32_t nverts) {
  const uint32_t v = blockIdx.x * 256u + threadIdx.x;
  if (v >= nverts) return;
  uint32_t x = v;
  for (;;) {                                  // read only: another lane may be storing the root of x into comp[x] right now, which is
    const uint32_t up = uf_load(comp, x);     // an ancestor of x like the word it replaces
    if (up == x) break;
    x = up;
  }
  __hip_atomic_store(comp + v, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- measures -----------------------------------------------------------------------------------------------------------------------
// Lanes that hold equal keys next to each other form a run.  On return the LAST lane of every run (`last`) holds the run's totals of
// cnt and sum, added in lane order by a segmented scan; the other lanes hold partial ones.  Every lane of the wave must call it.
__device__ __forceinline__ void wave_run_totals(uint32_t key, uint32_t& cnt, double& sum, bool& last) {
  const int lane = (int)(threadIdx.x & 63u);
  const uint32_t before = __shfl_up(key, 1), after = __shfl_down(key, 1);
  const bool head = lane == 0 || before != key;
  const unsigned long long heads = __ballot(head);
  const unsigned long long upto = lane == 63 ? ~0ull : ((2ull << lane) - 1ull);
  const int first = 63 - __clzll((long long)(heads & upto));      // the head of this lane's run (lane 0 is always a head)
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t c = __shfl_up(cnt, d);
    const double s = __shfl_up(sum, d);
    if (lane - d >= first) {
      cnt += c;
      sum += s;
    }
  }
  last = lane == 63 || after != key;
}

__global__ __launch_bounds__(256) void forest_zero_kernel(double* __restrict__ cable, uint32_t* __restrict__ nv, uint32_t* __restrict__ ne,
                                                          uint32_t* __restrict__ degree, uint32_t nverts) {
  const uint32_t v = blockIdx.x * 256u + threadIdx.x;
  if (v >= nverts) return;
  cable[v] = 0.0;
  nv[v] = 0u;
  ne[v] = 0u;
  degree[v] = 0u;
}

__global__ __launch_bounds__(256) void forest_count_vertices_kernel(const uint32_t* __restrict__ comp, uint32_t nverts, uint32_t* nv) {
  const uint32_t v = blockIdx.x * 256u + threadIdx.x;
  const bool have = v < nverts;
  uint32_t key = have ? comp[v] : FOREST_NONE;
  if (key >= nverts) key = FOREST_NONE;
  uint32_t cnt = have ? 1u : 0u;
  double unused = 0.0;
  bool last;
  wave_run_totals(key, cnt, unused, last);
  if (last && key != FOREST_NONE) atomicAdd(nv + key, cnt);
}

__global__ __launch_bounds__(256) void forest_measure_edges_kernel(const float* __restrict__ xyz, const uint32_t* __restrict__ edges,
                                                                   const uint32_t* __restrict__ comp, uint32_t nverts, uint32_t nedges,
                                                                   double* cable, uint32_t* ne, uint32_t* degree) {
  const uint32_t e = blockIdx.x * 256u + threadIdx.x;
  uint32_t key = FOREST_NONE, cnt = 0u;
  double sum = 0.0;
  if (e < nedges) {
    const uint32_t a = edges[2 * (size_t)e], b = edges[2 * (size_t)e + 1];
    if (a < nverts && b < nverts) {
      const uint32_t root = comp[a];
      if (root < nverts) {
        key = root;
        cnt = 1u;
        sum = (double)edge_length(xyz, a, b);
        atomicAdd(degree + a, 1u);
        atomicAdd(degree + b, 1u);
      }
    }
  }
  bool last;
  wave_run_totals(key, cnt, sum, last);
  if (last && key != FOREST_NONE) {
    atomicAdd(ne + key, cnt);
    atomicAdd(cable + key, sum);
  }
}

// ---- ticks --------------------------------------------------------------------------------------------------------------------------
// Slots are the entries of the CSR adjacency (row_start, nbr); the slot s of vertex u names the edge (u, nbr[s]) as seen from u.
// A critical vertex has degree 1 (terminal) or >= 3 (branch).  Per slot of a critical vertex c (written by forest_chains_kernel):
//   far[s]     the critical vertex the chain that leaves c through s arrives at
//   twin[s]    the slot of that vertex through which it arrives
//   len32[s]   the chain's length accumulated in float32 from c outward, one edge at a time: dist = f32(dist + step)
//   rec[s]     the superedge record the slot belongs to (written by the orientation, kept up to date by every fusion)
__global__ __launch_bounds__(256) void forest_ticks_init_kernel(const uint32_t* __restrict__ row_start, uint32_t nverts, uint32_t nslots,
                                                                int32_t* __restrict__ arity, uint8_t* __restrict__ alive) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i < nslots) alive[i] = 1;
  if (i < nverts) {
    const uint32_t deg = row_start[i + 1] - row_start[i];
    arity[i] = deg >= 3u ? (int32_t)deg : 0;          // post.py: the degree for branches, 0 for terminals
  }
}

__global__ __launch_bounds__(256) void forest_chains_kernel(const float* __restrict__ xyz, const uint32_t* __restrict__ row_start,
                                                            const uint32_t* __restrict__ nbr, const uint32_t* __restrict__ crit,
                                                            uint32_t ncrit, uint32_t nverts, uint32_t nslots, uint32_t* __restrict__ far,
                                                            uint32_t* __restrict__ twin, float* __restrict__ len32) {
  const uint32_t k = blockIdx.x * 256u + threadIdx.x;
  if (k >= ncrit) return;
  const uint32_t c = crit[k];
  if (c >= nverts) return;
  const uint32_t c0 = row_start[c], c1 = row_start[c + 1];
  for (uint32_t s = c0; s < c1 && s < nslots; s++) {
    uint32_t prev = c, cur = nbr[s];
    far[s] = c;                               // (what a malformed adjacency leaves behind stays inside the arrays)
    twin[s] = s;
    len32[s] = 0.0f;
    if (cur >= nverts) continue;
    float dist = 0.0f + edge_length(xyz, prev, cur);
    uint32_t r0 = row_start[cur], r1 = row_start[cur + 1];
    for (uint32_t guard = 0; r1 - r0 == 2u && guard < nverts; guard++) {
      const uint32_t n0 = nbr[r0], n1 = nbr[r0 + 1];
      const uint32_t next = n0 == prev ? n1 : n0;
      if (next >= nverts) break;
      dist = dist + edge_length(xyz, cur, next);
      prev = cur;
      cur = next;
      r0 = row_start[cur];
      r1 = row_start[cur + 1];
    }
    if (r1 > nslots || r0 >= r1) continue;
    uint32_t t = r0;
    for (uint32_t q = r0; q < r1; q++)
      if (nbr[q] == prev) t = q;
    far[s] = cur;
    twin[s] = t;
    len32[s] = dist;
  }
}

struct TickKey {
  unsigned long long len;     // the bits of the non-negative f64 length (they order like the values)
  unsigned long long ends;    // (larger end << 32) | smaller end: the reference's key
  uint32_t rec;
};

__device__ __forceinline__ bool tick_less(const TickKey& a, const TickKey& b) {
  return a.len < b.len || (a.len == b.len && a.ends < b.ends);
}

struct TickTables {
  const uint32_t* row_start;
  const uint32_t* nbr;
  uint32_t nverts;
  uint32_t* rec;              // per slot
  int32_t* arity;             // per vertex
  uint32_t *ea, *eb, *sa, *sb;      // per record: the ends and the slot of each end through which the superedge leaves it
  double* len;
  uint8_t* flag;
  uint8_t* alive;             // per slot
  uint32_t rec_lo, rec_hi;    // the component's records: [rec_lo, rec_hi)
};

// every edge of the path from the end `from`, leaving it through `slot`, to the end `to`, in what is left of the tree: inner
// vertices of the path have exactly two edges left
__device__ void tick_delete_path(const TickTables& T, uint32_t from, uint32_t slot, uint32_t to) {
  uint32_t prev = from;
  for (uint32_t guard = 0; guard < T.nverts; guard++) {
    const uint32_t cur = T.nbr[slot];
    T.alive[slot] = 0;
    const uint32_t r0 = T.row_start[cur], r1 = T.row_start[cur + 1];
    uint32_t next = FOREST_NONE;
    for (uint32_t q = r0; q < r1; q++) {
      if (T.nbr[q] == prev) T.alive[q] = 0;
      else if (T.alive[q]) next = q;
    }
    if (cur == to || next == FOREST_NONE) return;
    prev = cur;
    slot = next;
  }
}

// x is down to two superedges: they become one, which is removable from now on whatever its ends are (post.py:324-336).  Returns
// whether it did.
__device__ bool tick_fuse(const TickTables& T, uint32_t x) {
  const uint32_t r0 = T.row_start[x], r1 = T.row_start[x + 1];
  uint32_t s1 = FOREST_NONE, s2 = FOREST_NONE;
  int left = 0;
  for (uint32_t q = r0; q < r1; q++)
    if (T.alive[q]) {
      if (left == 0) s1 = q;
      else s2 = q;
      left++;
    }
  T.arity[x] = 0;
  if (left != 2) return false;
  const uint32_t k1 = T.rec[s1], k2 = T.rec[s2];
  if (k1 == k2 || k1 < T.rec_lo || k1 >= T.rec_hi || k2 < T.rec_lo || k2 >= T.rec_hi) return false;      // (a malformed component)
  const bool x_first1 = T.ea[k1] == x, x_first2 = T.ea[k2] == x;
  const uint32_t p = x_first1 ? T.eb[k1] : T.ea[k1], sp = x_first1 ? T.sb[k1] : T.sa[k1];
  const uint32_t q = x_first2 ? T.eb[k2] : T.ea[k2], sq = x_first2 ? T.sb[k2] : T.sa[k2];
  T.ea[k1] = p;
  T.sa[k1] = sp;
  T.eb[k1] = q;
  T.sb[k1] = sq;
  T.len[k1] = (0.0 + T.len[k1]) + T.len[k2];          // f64; a sum of two terms does not depend on their order
  T.flag[k1] = SE_LIVE | SE_REMOVABLE;
  T.flag[k2] = 0;
  T.rec[sq] = k1;
  return true;
}

// One wave per listed component.  crit[cs .. ce) are its critical vertices, ascending; the records [cs + 1, ce) of the superedge
// table are its superedges: record i is the superedge through which the orientation from `start` reached queue[i].
__global__ __launch_bounds__(64) void forest_ticks_kernel(const uint32_t* __restrict__ row_start, const uint32_t* __restrict__ nbr,
                                                          const uint32_t* __restrict__ crit, const uint32_t* __restrict__ crit_start,
                                                          uint32_t nverts, double threshold, const uint32_t* far, const uint32_t* twin,
                                                          const float* len32, uint32_t* rec, int32_t* arity, uint32_t* queue, uint32_t* ea,
                                                          uint32_t* eb, uint32_t* sa, uint32_t* sb, double* len, uint8_t* flag,
                                                          uint8_t* alive) {
  const uint32_t lane = threadIdx.x;
  const uint32_t cs = crit_start[blockIdx.x], ce = crit_start[blockIdx.x + 1];
  if (ce < cs + 2u) return;
  // start: the smallest terminal
  uint32_t kstart = FOREST_NONE;
  for (uint32_t k = cs + lane; k < ce; k += 64u) {
    const uint32_t v = crit[k];
    if (v < nverts && row_start[v + 1] - row_start[v] == 1u && k < kstart) kstart = k;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const uint32_t o = __shfl_xor(kstart, d);
    if (o < kstart) kstart = o;
  }
  if (kstart == FOREST_NONE) return;
  // the contracted tree oriented from start: a lane per queue entry; the children of the entries of one round follow the queue's
  // end in lane order (a tree: every critical vertex is reached once)
  if (lane == 0) {
    queue[cs] = crit[kstart];
    sb[cs] = FOREST_NONE;
    flag[cs] = 0;
  }
  __syncthreads();
  uint32_t head = cs, tail = cs + 1u;
  while (head < tail) {
    const uint32_t n = tail - head < 64u ? tail - head : 64u;
    uint32_t u = 0, r0 = 0, r1 = 0, via = FOREST_NONE, cnt = 0;
    if (lane < n) {
      u = queue[head + lane];
      via = sb[head + lane];
      r0 = row_start[u];
      r1 = row_start[u + 1];
      cnt = (r1 - r0) - (via != FOREST_NONE ? 1u : 0u);
    }
    uint32_t incl = cnt;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t t = __shfl_up(incl, d);
      if ((int)lane >= d) incl += t;
    }
    const uint32_t total = __shfl(incl, 63);
    uint32_t pos = tail + (incl - cnt);
    if (lane < n) {
      for (uint32_t s = r0; s < r1; s++) {
        if (s == via) continue;
        if (pos >= ce) break;
        const uint32_t child = far[s], back = twin[s];
        queue[pos] = child;
        ea[pos] = u;
        eb[pos] = child;
        sa[pos] = s;
        sb[pos] = back;
        len[pos] = (double)len32[s];                  // float32 from the end nearer start, outward; then widened
        const bool terminal = r1 - r0 == 1u || row_start[child + 1] - row_start[child] == 1u;
        flag[pos] = terminal ? (SE_LIVE | SE_REMOVABLE) : SE_LIVE;
        rec[s] = pos;
        rec[back] = pos;
        pos++;
      }
    }
    head += n;
    tail = tail + total < ce ? tail + total : ce;
    __syncthreads();
  }
  const TickTables T = {row_start, nbr, nverts, rec, arity, ea, eb, sa, sb, len, flag, alive, cs + 1u, tail};
  uint32_t nlive = tail - cs - 1u;
  while (nlive > 1u) {
    TickKey best = {~0ull, ~0ull, FOREST_NONE};
    for (uint32_t i = cs + 1u + lane; i < tail; i += 64u) {
      if (flag[i] != (SE_LIVE | SE_REMOVABLE)) continue;
      const uint32_t a = ea[i], b = eb[i];
      const TickKey k = {(unsigned long long)__double_as_longlong(len[i]),
                         ((unsigned long long)(a > b ? a : b) << 32) | (unsigned long long)(a > b ? b : a), i};
      if (best.rec == FOREST_NONE || tick_less(k, best)) best = k;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      TickKey o;
      o.len = __shfl_xor(best.len, d);
      o.ends = __shfl_xor(best.ends, d);
      o.rec = __shfl_xor(best.rec, d);
      if (o.rec != FOREST_NONE && (best.rec == FOREST_NONE || tick_less(o, best))) best = o;
    }
    best.len = __shfl(best.len, 0);                   // one answer for the wave, also where a malformed table holds a key twice
    best.ends = __shfl(best.ends, 0);
    best.rec = __shfl(best.rec, 0);
    if (best.rec == FOREST_NONE) break;
    const uint32_t a = (uint32_t)(best.ends >> 32), b = (uint32_t)best.ends;
    if ((arity[a] == 1 && arity[b] == 1) || __longlong_as_double((long long)best.len) >= threshold) break;
    uint32_t left = nlive - 1u;
    if (lane == 0) {
      tick_delete_path(T, ea[best.rec], sa[best.rec], eb[best.rec]);
      flag[best.rec] = 0;
      arity[a] -= 1;
      arity[b] -= 1;
      if (arity[a] == 2 && tick_fuse(T, a)) left--;
      if (arity[b] == 2 && tick_fuse(T, b)) left--;
    }
    nlive = __shfl(left, 0);
    __syncthreads();
  }
}

}  // namespace kh

using namespace kh;

static bool forest_sizes_ok(int64_t nverts, int64_t nedges) { return nverts >= 0 && nverts < (1ll << 31) && nedges >= 0 && nedges < (1ll << 31); }

extern "C" int kh_forest_components(const uint32_t* edges, int64_t nverts, int64_t nedges, uint32_t* comp, void* stream) {
  if (int rc = require_device()) return rc;
  if (!forest_sizes_ok(nverts, nedges)) {
    set_error("kh_forest_components: 0 <= nverts < 2^31, 0 <= nedges < 2^31");
    return KH_EINVAL;
  }
  if (nverts == 0) return KH_OK;
  if (!comp || (nedges > 0 && !edges)) {
    set_error("kh_forest_components: null pointer");
    return KH_EINVAL;
  }
  const unsigned n = (unsigned)nverts, m = (unsigned)nedges;
  hipLaunchKernelGGL(forest_identity_kernel, dim3((n + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, comp, n);
  KH_LAUNCH_CHECK();
  if (m > 0) {
    hipLaunchKernelGGL(forest_union_kernel, dim3((m + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, edges, m, n, comp);
    KH_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(forest_flatten_kernel, dim3((n + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, comp, n);
  KH_LAUNCH_CHECK();
  return KH_OK;
}

extern "C" int kh_forest_measure(const float* xyz, const uint32_t* edges, const uint32_t* comp, int64_t nverts, int64_t nedges,
                                 double* cable, uint32_t* nv, uint32_t* ne, uint32_t* degree, void* stream) {
  if (int rc = require_device()) return rc;
  if (!forest_sizes_ok(nverts, nedges)) {
    set_error("kh_forest_measure: 0 <= nverts < 2^31, 0 <= nedges < 2^31");
    return KH_EINVAL;
  }
  if (nverts == 0) return KH_OK;
  if (!xyz || !comp || !cable || !nv || !ne || !degree || (nedges > 0 && !edges)) {
    set_error("kh_forest_measure: null pointer");
    return KH_EINVAL;
  }
  const unsigned n = (unsigned)nverts, m = (unsigned)nedges;
  hipLaunchKernelGGL(forest_zero_kernel, dim3((n + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, cable, nv, ne, degree, n);
  KH_LAUNCH_CHECK();
  hipLaunchKernelGGL(forest_count_vertices_kernel, dim3((n + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, comp, n, nv);
  KH_LAUNCH_CHECK();
  if (m > 0) {
    hipLaunchKernelGGL(forest_measure_edges_kernel, dim3((m + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, xyz, edges, comp, n, m, cable,
                       ne, degree);
    KH_LAUNCH_CHECK();
  }
  return KH_OK;
}

extern "C" int kh_forest_ticks(const float* xyz, const uint32_t* row_start, const uint32_t* nbr, const uint32_t* crit,
                               const uint32_t* crit_start, int64_t nverts, int64_t nslots, int64_t ncrit, int64_t ncomps,
                               double threshold, uint32_t* slot_scratch, int32_t* arity, uint32_t* rec_scratch, double* rec_len,
                               uint8_t* rec_flag, uint8_t* alive, void* stream) {
  if (int rc = require_device()) return rc;
  if (nverts < 0 || nverts >= (1ll << 31) || nslots < 0 || nslots >= (1ll << 32) || ncrit < 0 || ncrit > nverts || ncomps < 0 ||
      ncomps > ncrit) {
    set_error("kh_forest_ticks: 0 <= nverts < 2^31, 0 <= nslots < 2^32, 0 <= ncomps <= ncrit <= nverts");
    return KH_EINVAL;
  }
  if (nverts == 0) return KH_OK;
  if (!row_start || !arity || (nslots > 0 && (!nbr || !alive || !slot_scratch)) ||
      (ncomps > 0 && (!xyz || !crit || !crit_start || !rec_scratch || !rec_len || !rec_flag || nslots == 0))) {
    set_error("kh_forest_ticks: null pointer");
    return KH_EINVAL;
  }
  const unsigned n = (unsigned)nverts, ns = (unsigned)nslots, nc = (unsigned)ncrit;
  const unsigned most = n > ns ? n : ns;
  hipLaunchKernelGGL(forest_ticks_init_kernel, dim3((most + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, row_start, n, ns, arity, alive);
  KH_LAUNCH_CHECK();
  if (ncomps == 0) return KH_OK;
  uint32_t* far = slot_scratch;
  uint32_t* twin = slot_scratch + (size_t)ns;
  float* len32 = (float*)(slot_scratch + 2 * (size_t)ns);
  uint32_t* rec = slot_scratch + 3 * (size_t)ns;
  hipLaunchKernelGGL(forest_chains_kernel, dim3((nc + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, xyz, row_start, nbr, crit, nc, n, ns,
                     far, twin, len32);
  KH_LAUNCH_CHECK();
  uint32_t* r = rec_scratch;
  hipLaunchKernelGGL(forest_ticks_kernel, dim3((unsigned)ncomps), dim3(64), 0, (hipStream_t)stream, row_start, nbr, crit, crit_start, n,
                     threshold, far, twin, len32, rec, arity, r, r + (size_t)nc, r + 2 * (size_t)nc, r + 3 * (size_t)nc, r + 4 * (size_t)nc,
                     rec_len, rec_flag, alive);
  KH_LAUNCH_CHECK();
  return KH_OK;
}
