// walk.hip -- Skeleton.paths() and the section normals of utility._xs_occurrences for every tree of a call at once, on the forest
// form (gfx950).
//
//   kh_walk_orient   per listed tree: the root (the vertex farthest in hops from the component's smallest vertex, the smallest index
//                    among equally far ones), parent and depth of every vertex oriented from it, and the leaves in the order a
//                    depth-first walk that takes neighbours in ascending index reaches them, each with the length of its path.
//   kh_walk_emit     per path root .. leaf: its vertices in that order, and the unit normals of utility._xs_occurrences along it.
//
// The work per component is bounded by its critical vertices, not by its depth: a thread per critical vertex walks the chains that
// leave it (walk_chains_kernel), ONE WAVE per component works on the contracted tree (walk_orient_kernel), and a thread per
// superedge writes parent / depth along its chain (walk_fill_kernel).  A vertex is critical when its degree is 1 or >= 3, or when it
// is the smallest vertex of its component (comp[v] == v): the hops are counted from there, so the chains stop there.
// No atomics: a component belongs to one wave, a chain to one thread, a path to one thread.
#include "common.h"

#include <math.h>

namespace kh {

static constexpr uint32_t WALK_NONE = 0xFFFFFFFFu;

__device__ __forceinline__ bool walk_critical(const uint32_t* __restrict__ row_start, const uint32_t* __restrict__ comp, uint32_t v) {
  return row_start[v + 1] - row_start[v] != 2u || comp[v] == v;
}

__global__ __launch_bounds__(256) void walk_init_kernel(uint32_t* __restrict__ parent, uint32_t* __restrict__ depth, uint32_t nverts,
                                                        uint32_t* __restrict__ path_leaf, uint32_t* __restrict__ path_len,
                                                        uint32_t npaths, uint32_t* __restrict__ qv, uint32_t ncrit) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i < nverts) {
    parent[i] = WALK_NONE;
    depth[i] = 0u;
  }
  if (i < npaths) {
    path_leaf[i] = WALK_NONE;
    path_len[i] = 0u;
  }
  if (i < ncrit) qv[i] = WALK_NONE;
}

// Per slot s of a critical vertex c: far[s] the critical vertex the chain that leaves c through s arrives at, twin[s] the slot of
// that vertex through which it arrives, hops[s] the chain's edges.
__global__ __launch_bounds__(256) void walk_chains_kernel(const uint32_t* __restrict__ row_start, const uint32_t* __restrict__ nbr,
                                                          const uint32_t* __restrict__ comp, const uint32_t* __restrict__ crit,
                                                          uint32_t ncrit, uint32_t nverts, uint32_t nslots, uint32_t* __restrict__ far,
                                                          uint32_t* __restrict__ twin, uint32_t* __restrict__ hops) {
  const uint32_t k = blockIdx.x * 256u + threadIdx.x;
  if (k >= ncrit) return;
  const uint32_t c = crit[k];
  if (c >= nverts) return;
  const uint32_t c0 = row_start[c], c1 = row_start[c + 1];
  for (uint32_t s = c0; s < c1 && s < nslots; s++) {
    uint32_t prev = c, cur = nbr[s], h = 1u;
    far[s] = c;                               // (what a malformed adjacency leaves behind stays inside the arrays)
    twin[s] = s;
    hops[s] = 0u;
    if (cur >= nverts) continue;
    uint32_t r0 = row_start[cur], r1 = row_start[cur + 1];
    for (uint32_t guard = 0; r1 - r0 == 2u && comp[cur] != cur && guard < nverts; guard++) {
      if (r1 > nslots) break;
      const uint32_t n0 = nbr[r0], n1 = nbr[r0 + 1];
      const uint32_t next = n0 == prev ? n1 : n0;
      if (next >= nverts) break;
      prev = cur;
      cur = next;
      h++;
      r0 = row_start[cur];
      r1 = row_start[cur + 1];
    }
    if (r1 > nslots || r0 >= r1) continue;
    uint32_t t = r0;
    for (uint32_t q = r0; q < r1; q++)
      if (nbr[q] == prev) t = q;
    far[s] = cur;
    twin[s] = t;
    hops[s] = h;
  }
}

struct WalkQueue {
  uint32_t *qv, *qvia, *qdep, *qcb, *qcc, *qbatch;      // per record: vertex, the slot back to its parent, depth, children [qcb, qcb + qcc)
};

// The contracted tree oriented from `start`: a lane per queue entry, rounds of at most 64; the children of the entries of one round
// follow the queue's end in lane order, each entry's in slot order (ascending neighbour).  qbatch[cs + b] is the first entry of round
// b; the children of an entry lie behind its round.  Returns the queue's end; nbatch: the rounds.
__device__ uint32_t walk_orient_from(const uint32_t* __restrict__ row_start, const uint32_t* far, const uint32_t* twin,
                                     const uint32_t* hops, const WalkQueue& Q, uint32_t start, uint32_t cs, uint32_t ce,
                                     uint32_t& nbatch) {
  const uint32_t lane = threadIdx.x;
  if (lane == 0) {
    Q.qv[cs] = start;
    Q.qvia[cs] = WALK_NONE;
    Q.qdep[cs] = 0u;
  }
  __syncthreads();
  uint32_t head = cs, tail = cs + 1u;
  nbatch = 0u;
  while (head < tail) {
    const uint32_t n = tail - head < 64u ? tail - head : 64u;
    uint32_t r0 = 0, r1 = 0, via = WALK_NONE, cnt = 0, dep = 0;
    if (lane == 0) Q.qbatch[cs + nbatch] = head;
    if (lane < n) {
      const uint32_t u = Q.qv[head + lane];
      via = Q.qvia[head + lane];
      dep = Q.qdep[head + lane];
      r0 = row_start[u];
      r1 = row_start[u + 1];
      cnt = (r1 - r0) - (via != WALK_NONE ? 1u : 0u);
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
      const uint32_t first = pos < ce ? pos : ce;
      for (uint32_t s = r0; s < r1; s++) {
        if (s == via) continue;
        if (pos >= ce) break;
        Q.qv[pos] = far[s];
        Q.qvia[pos] = twin[s];
        Q.qdep[pos] = dep + hops[s];
        pos++;
      }
      Q.qcb[head + lane] = first;
      Q.qcc[head + lane] = (pos < ce ? pos : ce) - first;
    }
    nbatch++;
    head += n;
    tail = tail + total < ce ? tail + total : ce;
    __syncthreads();
  }
  return tail;
}

// One wave per listed component.  crit[cs .. ce) are its critical vertices, ascending (crit[cs] is its smallest vertex); the records
// [cs, ce) of the tables are its queue.
__global__ __launch_bounds__(64) void walk_orient_kernel(const uint32_t* __restrict__ row_start, const uint32_t* __restrict__ crit,
                                                         const uint32_t* __restrict__ crit_start, const uint32_t* __restrict__ leaf_start,
                                                         uint32_t nverts, uint32_t npaths, const uint32_t* far, const uint32_t* twin,
                                                         const uint32_t* hops, uint32_t* qv, uint32_t* qvia, uint32_t* qdep, uint32_t* qcb,
                                                         uint32_t* qcc, uint32_t* qbatch, uint32_t* qcnt, uint32_t* qoff,
                                                         uint32_t* path_leaf, uint32_t* path_len) {
  const uint32_t lane = threadIdx.x;
  const uint32_t cs = crit_start[blockIdx.x], ce = crit_start[blockIdx.x + 1];
  if (ce < cs + 2u) return;
  const uint32_t v0 = crit[cs];
  if (v0 >= nverts) return;
  const WalkQueue Q = {qv, qvia, qdep, qcb, qcc, qbatch};
  uint32_t nbatch;
  uint32_t tail = walk_orient_from(row_start, far, twin, hops, Q, v0, cs, ce, nbatch);
  // the root: the degree-1 vertex of most hops, the smallest among those
  unsigned long long best = 0ull;
  for (uint32_t i = cs + lane; i < tail; i += 64u) {
    const uint32_t v = qv[i];
    if (v >= nverts || row_start[v + 1] - row_start[v] != 1u) continue;
    const unsigned long long key = ((unsigned long long)qdep[i] << 32) | (unsigned long long)(WALK_NONE - v);
    if (key > best) best = key;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const unsigned long long o = __shfl_xor(best, d);
    if (o > best) best = o;
  }
  best = __shfl(best, 0);
  if (best == 0ull) return;
  const uint32_t root = WALK_NONE - (uint32_t)best;
  __syncthreads();
  tail = walk_orient_from(row_start, far, twin, hops, Q, root, cs, ce, nbatch);
  // leaves below every entry, bottom-up over the rounds: an entry's children lie behind its round
  for (uint32_t b = nbatch; b-- > 0u;) {
    const uint32_t lo = qbatch[cs + b], hi = b + 1u < nbatch ? qbatch[cs + b + 1u] : tail;
    const uint32_t i = lo + lane;
    if (i < hi) {
      const uint32_t c0 = qcb[i], cc = qcc[i];
      uint32_t sum = cc == 0u ? 1u : 0u;
      for (uint32_t j = c0; j < c0 + cc; j++) sum += qcnt[j];
      qcnt[i] = sum;
    }
    __syncthreads();
  }
  // ... and the place of every leaf among the component's leaves, top-down: an earlier child's leaves come first
  if (lane == 0) qoff[cs] = 0u;
  __syncthreads();
  const uint32_t p0 = leaf_start[blockIdx.x], p1 = leaf_start[blockIdx.x + 1];
  for (uint32_t b = 0; b < nbatch; b++) {
    const uint32_t lo = qbatch[cs + b], hi = b + 1u < nbatch ? qbatch[cs + b + 1u] : tail;
    const uint32_t i = lo + lane;
    if (i < hi) {
      const uint32_t c0 = qcb[i], cc = qcc[i];
      uint32_t off = qoff[i];
      for (uint32_t j = c0; j < c0 + cc; j++) {
        qoff[j] = off;
        off += qcnt[j];
      }
      if (cc == 0u && i != cs) {
        const uint32_t p = p0 + off;
        if (p >= p0 && p < p1 && p < npaths) {
          path_leaf[p] = qv[i];
          path_len[p] = qdep[i] + 1u;
        }
      }
    }
    __syncthreads();
  }
}

// A thread per record: parent and depth along the chain from the record's vertex up to the critical vertex it was reached from.
__global__ __launch_bounds__(256) void walk_fill_kernel(const uint32_t* __restrict__ row_start, const uint32_t* __restrict__ nbr,
                                                        const uint32_t* __restrict__ comp, const uint32_t* __restrict__ qv,
                                                        const uint32_t* __restrict__ qvia, const uint32_t* __restrict__ qdep,
                                                        uint32_t ncrit, uint32_t nverts, uint32_t nslots, uint32_t* __restrict__ parent,
                                                        uint32_t* __restrict__ depth) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= ncrit) return;
  uint32_t cur = qv[i], slot = qvia[i], d = qdep[i];
  if (cur >= nverts || slot >= nslots) return;          // no record, or the root: parent NONE, depth 0 (walk_init_kernel)
  for (uint32_t guard = 0; guard < nverts; guard++) {
    const uint32_t next = nbr[slot];
    if (next >= nverts) return;
    parent[cur] = next;
    depth[cur] = d;
    if (d == 0u || walk_critical(row_start, comp, next)) return;
    const uint32_t r0 = row_start[next];
    if (r0 + 1u >= nslots) return;
    slot = nbr[r0] == cur ? r0 + 1u : r0;
    cur = next;
    d--;
  }
}

// ---- emit ---------------------------------------------------------------------------------------------------------------------------
// A thread per path: its vertices, written from the leaf upward.
__global__ __launch_bounds__(256) void walk_paths_kernel(const uint32_t* __restrict__ parent, const uint32_t* __restrict__ path_leaf,
                                                         const long long* __restrict__ pstart, uint32_t npaths, uint32_t nverts,
                                                         long long m, uint32_t* __restrict__ occ_vertex) {
  const uint32_t p = blockIdx.x * 256u + threadIdx.x;
  if (p >= npaths) return;
  long long a = pstart[p], b = pstart[p + 1];
  if (a < 0) a = 0;
  if (b > m) b = m;
  uint32_t cur = path_leaf[p];
  for (long long k = b; k-- > a;) {
    occ_vertex[k] = cur;
    cur = cur < nverts ? parent[cur] : WALK_NONE;
  }
}

__device__ __forceinline__ void walk_diff(const int32_t* __restrict__ vox, const uint32_t* occ, uint32_t nverts, long long a, long long len,
                                          long long j, long long d[3]) {
  // d_j = vox[next] - vox[this]; the last vertex repeats the last difference (a path has two vertices at least)
  if (j >= len - 1) j = len - 2;
  d[0] = d[1] = d[2] = 0;
  if (j < 0) return;
  const uint32_t u = occ[a + j], v = occ[a + j + 1];
  if (u >= nverts || v >= nverts) return;
#pragma unroll
  for (int c = 0; c < 3; c++) d[c] = (long long)vox[3 * (size_t)v + c] - (long long)vox[3 * (size_t)u + c];
}

// window 1: a thread per occurrence, float32 as numpy has it there, then widened
__global__ __launch_bounds__(256) void walk_normals1_kernel(const int32_t* __restrict__ vox, const uint32_t* __restrict__ occ_vertex,
                                                            const long long* __restrict__ pstart, uint32_t npaths, uint32_t nverts,
                                                            long long m, double* __restrict__ normal) {
  const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
  if (k >= m) return;
  uint32_t lo = 0, hi = npaths;                       // the path of k: the last p with pstart[p] <= k
  while (hi - lo > 1u) {
    const uint32_t mid = lo + (hi - lo) / 2u;
    if (pstart[mid] <= k) lo = mid;
    else hi = mid;
  }
  const long long a = pstart[lo], len = pstart[lo + 1] - a;
  long long d[3] = {0, 0, 0};
  if (a >= 0 && a <= k && a + len <= m) walk_diff(vox, occ_vertex, nverts, a, len, k - a, d);
  const float x = (float)d[0], y = (float)d[1], z = (float)d[2];
  const float norm = sqrtf(((x * x) + (y * y)) + (z * z));      // sqrtf and / are correctly rounded in this build; the __f*_rn
  normal[3 * k] = (double)(x / norm);                           // intrinsics map to the native approximations
  normal[3 * k + 1] = (double)(y / norm);
  normal[3 * k + 2] = (double)(z / norm);
}

// np.pad(mode="symmetric"): reflection with period 2 * len
__device__ __forceinline__ long long walk_reflect(long long j, long long len) {
  long long r = j % (2 * len);
  if (r < 0) r += 2 * len;
  return r < len ? r : 2 * len - 1 - r;
}

// window n > 1: a thread per path, everything f64, both moving averages in numpy's order (utility.moving_average): the first over
// integers (exact in any order), the second over the reversed result as the DIFFERENCE OF TWO SEQUENTIAL RUNNING SUMS in padded
// order.  first f64 [m, 3] holds the first pass.
__global__ __launch_bounds__(64) void walk_normals_kernel(const int32_t* __restrict__ vox, const uint32_t* __restrict__ occ_vertex,
                                                          const long long* __restrict__ pstart, uint32_t npaths, uint32_t nverts,
                                                          long long m, int window, double* first, double* __restrict__ normal) {
  const uint32_t p = blockIdx.x * 64u + threadIdx.x;
  if (p >= npaths) return;
  const long long a = pstart[p], len = pstart[p + 1] - a, n = window;
  if (a < 0 || len < 2 || a + len > m) {
    for (long long k = a < 0 ? 0 : a; k < a + len && k < m; k++) normal[3 * k] = normal[3 * k + 1] = normal[3 * k + 2] = 0.0;
    return;
  }
  const double dn = (double)window;
  // first pass: out[i] = (the sum of the padded input over (i - n, i]) / n
  long long sum[3] = {0, 0, 0}, d[3];
  for (long long j = 1 - n; j <= 0; j++) {
    walk_diff(vox, occ_vertex, nverts, a, len, walk_reflect(j, len), d);
    sum[0] += d[0], sum[1] += d[1], sum[2] += d[2];
  }
  for (long long i = 0; i < len; i++) {
    if (i > 0) {
      walk_diff(vox, occ_vertex, nverts, a, len, walk_reflect(i, len), d);
      sum[0] += d[0], sum[1] += d[1], sum[2] += d[2];
      walk_diff(vox, occ_vertex, nverts, a, len, walk_reflect(i - n, len), d);
      sum[0] -= d[0], sum[1] -= d[1], sum[2] -= d[2];
    }
#pragma unroll
    for (int c = 0; c < 3; c++) first[3 * (a + i) + c] = (double)sum[c] / dn;
  }
  // second pass over b[i] = first[len - 1 - i]: padded P[q] = b[reflect(q - n)], R[q] = P[0] + ... + P[q] one addition at a time;
  // out[i] = (R[n + i] - R[i]) / n goes to position len - 1 - i.  Two cursors run the same sums, n entries apart.
  double lead[3] = {0.0, 0.0, 0.0}, lag[3] = {0.0, 0.0, 0.0};
  for (long long q = 0; q < n; q++) {
    const long long src = a + (len - 1 - walk_reflect(q - n, len));
#pragma unroll
    for (int c = 0; c < 3; c++) lead[c] = q == 0 ? first[3 * src + c] : lead[c] + first[3 * src + c];
  }
  for (long long i = 0; i < len; i++) {
    const long long src_lead = a + (len - 1 - walk_reflect(i, len));            // P[n + i]
    const long long src_lag = a + (len - 1 - walk_reflect(i - n, len));         // P[i]
    double v[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
      lead[c] = lead[c] + first[3 * src_lead + c];
      lag[c] = i == 0 ? first[3 * src_lag + c] : lag[c] + first[3 * src_lag + c];
      v[c] = (lead[c] - lag[c]) / dn;
    }
    const double norm = sqrt(((v[0] * v[0]) + (v[1] * v[1])) + (v[2] * v[2]));
    const long long k = a + (len - 1 - i);
#pragma unroll
    for (int c = 0; c < 3; c++) normal[3 * k + c] = v[c] / norm;
  }
}

}  // namespace kh

using namespace kh;

extern "C" int kh_walk_orient(const uint32_t* row_start, const uint32_t* nbr, const uint32_t* comp, const uint32_t* crit,
                              const uint32_t* crit_start, const uint32_t* leaf_start, int64_t nverts, int64_t nslots, int64_t ncrit,
                              int64_t ncomps, int64_t npaths, uint32_t* slot_scratch, uint32_t* rec_scratch, uint32_t* parent,
                              uint32_t* depth, uint32_t* path_leaf, uint32_t* path_len, void* stream) {
  if (int rc = require_device()) return rc;
  if (nverts < 0 || nverts >= (1ll << 31) || nslots < 0 || nslots >= (1ll << 31) || ncrit < 0 || ncrit > nverts || ncomps < 0 ||
      ncomps > ncrit || npaths < 0 || npaths > ncrit) {
    set_error("kh_walk_orient: 0 <= nverts, nslots < 2^31, 0 <= ncomps <= ncrit <= nverts, 0 <= npaths <= ncrit");
    return KH_EINVAL;
  }
  if (nverts == 0) return KH_OK;
  if (!parent || !depth || (npaths > 0 && (!path_leaf || !path_len)) || (ncrit > 0 && !rec_scratch) ||
      (ncomps > 0 && (!row_start || !nbr || !comp || !crit || !crit_start || !leaf_start || !slot_scratch || nslots == 0))) {
    set_error("kh_walk_orient: null pointer");
    return KH_EINVAL;
  }
  const unsigned n = (unsigned)nverts, ns = (unsigned)nslots, nc = (unsigned)ncrit, np = (unsigned)npaths;
  uint32_t* r = rec_scratch;
  uint32_t *qv = r, *qvia = r + (size_t)nc, *qdep = r + 2 * (size_t)nc, *qcb = r + 3 * (size_t)nc, *qcc = r + 4 * (size_t)nc,
           *qbatch = r + 5 * (size_t)nc, *qcnt = r + 6 * (size_t)nc, *qoff = r + 7 * (size_t)nc;
  hipLaunchKernelGGL(walk_init_kernel, dim3((n + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, parent, depth, n, path_leaf, path_len, np,
                     qv, nc);
  KH_LAUNCH_CHECK();
  if (ncomps == 0) return KH_OK;
  uint32_t *far = slot_scratch, *twin = slot_scratch + (size_t)ns, *hops = slot_scratch + 2 * (size_t)ns;
  hipLaunchKernelGGL(walk_chains_kernel, dim3((nc + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, row_start, nbr, comp, crit, nc, n, ns,
                     far, twin, hops);
  KH_LAUNCH_CHECK();
  hipLaunchKernelGGL(walk_orient_kernel, dim3((unsigned)ncomps), dim3(64), 0, (hipStream_t)stream, row_start, crit, crit_start, leaf_start,
                     n, np, far, twin, hops, qv, qvia, qdep, qcb, qcc, qbatch, qcnt, qoff, path_leaf, path_len);
  KH_LAUNCH_CHECK();
  hipLaunchKernelGGL(walk_fill_kernel, dim3((nc + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, row_start, nbr, comp, qv, qvia, qdep, nc,
                     n, ns, parent, depth);
  KH_LAUNCH_CHECK();
  return KH_OK;
}

extern "C" int kh_walk_emit(const uint32_t* parent, const uint32_t* path_leaf, const int64_t* pstart, const int32_t* vox, int64_t nverts,
                            int64_t npaths, int64_t nocc, int window, uint32_t* occ_vertex, double* normal, double* first,
                            void* stream) {
  if (int rc = require_device()) return rc;
  if (nverts < 0 || nverts >= (1ll << 31) || npaths < 0 || npaths > nverts || nocc < 0 || nocc >= (1ll << 31) || window < 0) {
    set_error("kh_walk_emit: 0 <= nverts, nocc < 2^31, 0 <= npaths <= nverts, window >= 0");
    return KH_EINVAL;
  }
  if (npaths == 0 || nocc == 0) return KH_OK;
  if (!parent || !path_leaf || !pstart || !occ_vertex || (window > 0 && (!vox || !normal)) || (window > 1 && !first)) {
    set_error("kh_walk_emit: null pointer");
    return KH_EINVAL;
  }
  const unsigned n = (unsigned)nverts, np = (unsigned)npaths;
  const long long* ps = (const long long*)pstart;
  hipLaunchKernelGGL(walk_paths_kernel, dim3((np + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, parent, path_leaf, ps, np, n,
                     (long long)nocc, occ_vertex);
  KH_LAUNCH_CHECK();
  if (window == 1) {
    hipLaunchKernelGGL(walk_normals1_kernel, dim3((unsigned)((nocc + 255) / 256)), dim3(256), 0, (hipStream_t)stream, vox, occ_vertex, ps, np,
                       n, (long long)nocc, normal);
    KH_LAUNCH_CHECK();
  } else if (window > 1) {
    hipLaunchKernelGGL(walk_normals_kernel, dim3((np + 63u) / 64u), dim3(64), 0, (hipStream_t)stream, vox, occ_vertex, ps, np, n,
                       (long long)nocc, window, first, normal);
    KH_LAUNCH_CHECK();
  }
  return KH_OK;
}
