// trace.hip -- the kernels and entry points of the per-label TEASAR searches for gfx950: one workgroup per label (512 threads by
// default for the distance fields, 256 -- or 128 / 64 by flag -- for the path loop).  ONE translation unit: the machines the
// kernels are made of live in headers of their own and are compiled here, together (the sweep's out-of-line functions inherit
// the register bound of the kernels that reach them, see invalidate_ball_kernel).
//
//   kh_edf_batch    a4  dijkstra3d.euclidean_distance_field   (kimimaro/trace.py:139-145, 302-307)
//   kh_trace_paths  a6-a11 compute_paths loop                 (kimimaro/trace.py:196-267):
//                     target finder   skeletontricks.pyx:995-1045
//                     railroad        dijkstra3d.railroad, trace.py:240-242
//                     invalidation    skeletontricks.pyx:373-418 -> dijkstra_invalidation.hpp:239-332
//                     rail edits      trace.py:220, 261-263
//   kh_invalidate_ball, kh_path_search, kh_parental_field, kh_path_from_parents, kh_invalidate_cube, kh_level_keys
//                   a7-a10 one at a time, on the same device routines
//
//   search_state.h  Ctl, Queues, the membership flags and the L2 loads / stores every machine shares
//   rows27.h        the 27 words around a voxel as nine rows of three (searches and sweep)
//   sssp.h          Search = label-correcting relaxation with a near/far split (delta-stepping with an adaptive threshold): one
//                   thread per frontier voxel, distances are float bit patterns, the offers of a batch are combined by an LDS
//                   atomic min and written by one thread each, the work lists hold voxel indices only (membership bits in `qstate`
//                   keep every list bounded by the label size).  The distances converge to the unique Bellman fixpoint
//                   d[v] = min_u fl(d[u] + w), so they equal the oracle's heap Dijkstra bit for bit regardless of the relaxation
//                   order.  Three counters say which parts of a search a call went through -- n_retries (a flush round repeated
//                   because an offer found the combine table full), n_spills (a near-list round that began with entries beyond the
//                   LDS part) and n_splits (far-list splits); the kernels add them to kh_label_t.stat_search_*, and
//                   tests/test_gpu_search_regimes.py asserts them before it compares results.
//   backtrack.h     paths are recovered with the canonical predecessor rule of oracle/kimi_oracle.c (ko_pred / ko_walk), 26 lanes
//                   looking at the 26 neighbours at once.
//   heap.h          The invalidation flood is order dependent down to the tie order of std::priority_queue, so it
//                   is run as an exact emulation of the libstdc++ binary heap in which the 64 lanes of the label's first wave
//                   cooperate on every push and pop, with the 26 neighbour tests of each popped voxel evaluated by 26 lanes.
//   sweep.h         the order-free evaluation of the same flood, which certifies most calls without the heap
//   invalidate.h    one invalidation call: sweep first, heap emulation as the fall-back; scratch pool, ghosts
//
// No MFMA: irregular, latency/atomic bound integer+f32 work (north_star).  Labels are independent, so the chip is filled by running
// every label's workgroup concurrently; KH_TRACE_BIG_LDS_HEAP keeps two chunks of every label's heap in LDS (Heap<2>).
#include <stdlib.h>

#include "common.h"
#include "sweep.h"
#include "search_state.h"
#include "rows27.h"
#include "sssp.h"
#include "heap.h"
#include "backtrack.h"
#include "invalidate.h"

namespace kh {

__global__ __launch_bounds__(1024) void edf_batch_kernel(kh_label_t* tasks, int mode, const uint32_t* __restrict__ lists,
                                                        const uint32_t* __restrict__ nbrmask, Geometry g, float* field,
                                                        uint8_t* qstate, uint32_t* queues, float delta_floor) {
  __shared__ Ctl ctl;
  extern __shared__ __attribute__((aligned(16))) unsigned char search_lds[];     // KH_SSSP_LDS_BYTES per thread
  kh_label_t* task = &tasks[blockIdx.x];
  const int tid = threadIdx.x;
  if (mode == 1 && task->root != 0xFFFFFFFFu) return;
  const uint32_t source = (mode == 2) ? task->root : task->source;
  if (tid == 0) { ctl.status = 0; ctl.n_retries = ctl.n_spills = ctl.n_splits = 0; ctl.g = g; }
  __syncthreads();
  const Queues q = task_queues(task, queues);
  edf_label(&ctl, task, mode, lists + task->list_offset, task->count, nbrmask, field, qstate, q, delta_floor, source, search_lds,
            KH_SSSP_LDS_BYTES * blockDim.x);
  if (tid == 0) {
    task->status |= ctl.status;
    search_stats(task, ctl);
  }
}

// The second half of dijkstra3d.railroad (trace.py:240-242), by the whole workgroup right after sssp<1> from `src`: the walk back
// from the nearest rail (out[0] = the rail end; wave 0, its length in ctl.u0, 0 on failure), then dist = +inf and the queue flags
// cleared again on everything the search touched.  Returns ctl.u0 as it stands after the walk.  LOOP: the path loop's form --
// ctl.u0 starts at 0 here and the voxels the search touched are added to ctl.u2 (kh_label_t.stat_settled).
// (The sssp<1> call itself stays with the callers: made from in here, the copy of `q` it passes takes another stack slot.)
template <bool LOOP>
__device__ __forceinline__ uint32_t rail_walk(Ctl& ctl, const uint32_t* __restrict__ nbrmask, const float* pdrf, float* dist,
                                              uint8_t* qstate, uint32_t src, const Queues& q, uint32_t* out, uint32_t cap, bool graph,
                                              int nthr) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned long long br = ctl.best_rail;
  if (LOOP) {
    if (tid == 0) { ctl.u0 = 0; ctl.u2 += ctl.n_touched; }
    __syncthreads();
  }
  if (br == NONE64) {
    if (tid == 0) atomicOr(&ctl.status, KH_ST_NO_RAIL);
  } else if (wave == 0) {
    const uint32_t n = backtrack<true>(ctl.g, nbrmask, pdrf, dist, (uint32_t)br, src, out, cap, q.a, q.b, q.cap, qstate, &ctl.status, graph);
    if (lane == 0) ctl.u0 = n;
  }
  __syncthreads();
  const uint32_t plen = ctl.u0;
  // restore dist = +inf and the queue flags on everything the search touched
  const uint32_t nt = ctl.n_touched < q.cap ? ctl.n_touched : q.cap;
  for (uint32_t i = tid; i < nt; i += nthr) {
    const uint32_t v = q.touched[i];
    st_f32_l2(&dist[v], KH_INF);
    qstate[v] = 0;
  }
  return plen;
}

template <bool PROF, int TOPL>
#ifndef KH_TRACE_WAVES_PER_EU
#define KH_TRACE_WAVES_PER_EU 3   /* 168 VGPRs; 4 -> 128 VGPRs with 66 of them spilled */
#endif
__global__ __launch_bounds__(256, KH_TRACE_WAVES_PER_EU) void trace_paths_kernel(kh_label_t* tasks, const uint32_t* __restrict__ lists,
                                                          float* list_daf,
                                                          const uint32_t* __restrict__ nbrmask, Geometry g,
                                                          const float* __restrict__ dbf, float* pdrf, float* dist,
                                                          uint8_t* alive, uint8_t* qstate,
                                                          const uint32_t* __restrict__ manual_targets,
                                                          float scale, float constant, uint32_t* queues, hnode_t* heap_nodes,
                                                          uint32_t* path_vertices,
                                                          uint32_t* path_lengths, int fix_branching, SweepGlobal sg,
                                                          uint32_t* journal_buf, float* rail_save, uint32_t ghost_mode,
                                                          const uint8_t* __restrict__ corner_gate, uint32_t lds_bytes) {
  __shared__ Ctl ctl;
  __shared__ Sweep sw;
  __shared__ SweepShared swsh;
  __shared__ uint32_t sweep_stats[5];
  // Heap<TOPL>::LDS_BYTES for the heap emulation (TOP + 3 nodes, the key mirror); the sweep's level words and lists use the same bytes
  extern __shared__ __attribute__((aligned(16))) unsigned char heap_top[];
  kh_label_t* task = &tasks[blockIdx.x];
  const int tid = threadIdx.x;
  const int nthr = blockDim.x, nwav = nthr >> 6;
  const int lane = tid & 63, wave = tid >> 6;
  const uint32_t* list = lists + task->list_offset;
  float* ldaf = list_daf + task->list_offset;
  const uint32_t nf = task->count;
  const Queues q = task_queues(task, queues);
  Heap<TOPL> heap;
  hnode_t* const pool = (ghost_mode & 8u) ? heap_nodes : nullptr;      // KH_TRACE_SCRATCH_POOL: heap and journal on demand
  heap.node = pool ? nullptr : heap_nodes + task->heap_offset;
  heap.top = (lds_hnode_t*)heap_top;
  heap.cap = task->heap_capacity < Heap<TOPL>::MAX_N ? task->heap_capacity : Heap<TOPL>::MAX_N;   // beyond: KH_ST_HEAP_OVERFLOW
  heap.n = 0;
  heap_init_lane(heap, lane);
  uint32_t* pverts = path_vertices + task->path_offset;
  uint32_t* plens = path_lengths + task->path_offset;
  float* psave = rail_save ? rail_save + task->path_offset : nullptr;        // the weight a path vertex had before it became a rail
  uint32_t* journal = (journal_buf && !pool) ? journal_buf + (uint64_t)task->q_offset * 2 : nullptr;   // 2 * q_capacity entries; pool: on demand
  bool journal_off = false;            // the pool could not serve this label's journal: its ghost calls are rolled back at once
  const uint32_t pcap = task->path_capacity;
  uint32_t root = task->root;          // (0xFFFFFFFF with KH_TRACE_FUSED_EDF: found below, trace.py:291-308)
  uint32_t daf_loc = 0xFFFFFFFFu;      // KH_TRACE_FUSED_EDF: the voxel farthest from the root (the implicit first target, trace.py:160-172)
  const uint32_t* before = manual_targets + task->tgt_offset;
  const uint32_t* after = before + task->n_before;
  const bool soma = task->soma_mode != 0;
  const bool implicit = task->n_before == 0 && !soma;   // trace.py:160-172
  uint32_t nb = implicit ? 1u : task->n_before;
  uint32_t na = task->n_after;
  uint32_t valid = nf;
  uint32_t npaths = 0, nverts = 0;
  unsigned long long t_target = 0, t_rail = 0, t_inval = 0, t0 = 0;
  // ghost mode: bit 0 = on, bit 1 = every call that makes a ghost is rolled back at once (tests of the roll-back itself)
  const bool ghosts_on = (ghost_mode & 1u) != 0u && (journal != nullptr || pool != nullptr) && (psave != nullptr || !fix_branching) &&
                         sg.on != 0u && sg.sched != nullptr;
  const bool paranoid = (ghost_mode & 2u) != 0u;
  const bool graph = (ghost_mode & 4u) != 0u;     // the neighbour masks carry a voxel graph: predecessor edges are one-way
  GhostState gs = {0u, 0u, 0u, 0u, 0u, 0u, 0u};
  uint32_t n_ghost_calls = 0, n_rollbacks = 0;
  if (tid == 0) {
    ctl.status = 0; ctl.u2 = 0; ctl.u3 = 0; ctl.cyc3[0] = ctl.cyc3[1] = ctl.cyc3[2] = 0; ctl.g = g;
    ctl.n_retries = ctl.n_spills = ctl.n_splits = 0;
    for (int i = 0; i < 5; i++) sweep_stats[i] = 0;
    sweep_setup(sw, &swsh, &ctl, sg, task, nbrmask, alive, q, q.a, nf, heap_top, corner_gate);
  }
  __syncthreads();
  // the spill table of the sweep starts all-free (the arena is uninitialised memory)
  for (uint32_t i = tid; i < sw.spcap; i += nthr) { sw.spk[i] = 0u; sw.spc[i] = 0ull; }
  __syncthreads();
  if (ghost_mode & 16u) {
    // KH_TRACE_FUSED_EDF (round 6): the label's two distance-field searches and its PDRF run HERE, by the label's own workgroup,
    // instead of as three launches over all labels in front of this kernel -- with volumes in flight every launch waits for the
    // slots the others' path workgroups hold, and the chain of a volume (its largest label that needs the heap emulation) could
    // only start once the searches of ALL its labels were through: 2.3 s into a 8.6 s round of twenty volumes.
    // find_root (trace.py:291-308), DAF from the root (:139-145) into `dist` (+inf again afterwards), then per voxel of the list:
    // the DAF for the target finder and compute_pdrf (:315-356, the repeated-squaring branch), every operation rounded to f32.
    const float delta_floor = 2.0f * fminf(g.wx, fminf(g.wy, g.wz));
    if (root == 0xFFFFFFFFu) {
      edf_label(&ctl, task, 1, list, nf, nbrmask, dist, qstate, q, delta_floor, task->source, heap_top, lds_bytes);
      root = 0xFFFFFFFFu - (uint32_t)ctl.red64[0];         // (every thread: the record was written by thread 0 only)
      __syncthreads();
    }
    edf_label(&ctl, task, 2, list, nf, nbrmask, dist, qstate, q, delta_floor, root, heap_top, lds_bytes);
    const float max_daf = __uint_as_float((uint32_t)(ctl.red64[0] >> 32));
    daf_loc = 0xFFFFFFFFu - (uint32_t)ctl.red64[0];
    const float M = task->M, pscale = task->pdrf_scale;
    const int nsq = (int)task->pdrf_log2e;
    __syncthreads();
    for (uint32_t i = tid; i < nf; i += nthr) {
      const uint32_t v = list[i];
      float d = ld_f32_l2(&dist[v]);
      ldaf[i] = d;
      float p = dbf[v] * M;        // np.multiply(DBF, M)            trace.py:341
      p = 1.0f - p;                // np.subtract(f(1), PDRF)        trace.py:342
      for (int sq = 0; sq < nsq; sq++) p = p * p;   //              trace.py:343-345
      p = p * pscale;              // PDRF *= f(pdrf_scale)          trace.py:349
      if (d == KH_INF) d = 0.0f;   // inf2zero                       trace.py:146
      if (max_daf != 0.0f) {
        const float inv = 1.0f / max_daf;   // (1 / max_daf) in float32 (numpy 2 scalar)  trace.py:353
        d = d * inv;
        p = p + d;                 //                                trace.py:354
      }
      pdrf[v] = p;
      st_f32_l2(&dist[v], KH_INF);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __syncthreads();
  }
  if (soma) {
    // trace.py:160-168: one-off invalidation around the soma centre, before valid_labels is counted (:211)
    if (tid == 0) pverts[0] = root;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __syncthreads();
    valid -= invalidate<PROF, Heap<TOPL>>(&ctl, &sw, task, nbrmask, dbf, alive, pverts, 1, task->soma_scale, task->soma_const,
                                          heap, list, nf, sweep_stats, sg.heap_prio, q.a, false, false, true, corner_gate, pool);   // trace.py:211 counts what is left
  }
  const uint32_t max_paths = task->max_paths ? task->max_paths : valid;  // trace.py:214-215
  if (nb + na >= max_paths) {                           // trace.py:217-218
    if (tid == 0) {
      task->n_paths = 0; task->n_vertices = 0; task->status |= ctl.status;
      search_stats(task, ctl);
    }
    return;
  }
  if (fix_branching) {
    if (tid == 0) pdrf[root] = 0.0f;                    // trace.py:220 (initial rail)
  } else {
    // trace.py:155: one weighted Dijkstra from the root; every path is then a predecessor walk
    sssp<2>(ctl.g, nbrmask, pdrf, dist, qstate, root, q, &ctl, 0.0f, heap_top, lds_bytes);
  }
  __syncthreads();
  bool redo = false;      // this iteration redoes the invalidation of path `npaths` by the heap emulation (after a roll-back)
  for (;;) {
    if (npaths >= max_paths) break;
    bool rollback = false;
    uint32_t plen = 0;
    uint32_t* out = pverts + nverts;
    if (gs.nghost > 0 && (valid == 0 || paranoid || journal_off)) rollback = true;   // nothing certainly valid is left, but ghosts are
    if (!rollback && !redo) {
      if (!(valid > 0 || nb > 0 || na > 0)) break;
      // ---- target selection, trace.py:225-230
      t0 = clock64();
      uint32_t target;
      if (nb > 0) { nb--; target = implicit ? (daf_loc != 0xFFFFFFFFu ? daf_loc : task->max_loc) : before[nb]; }
      else if (valid == 0) { na--; target = after[na]; }
      else {
        // CachedTargetFinder.find_target: the valid voxel with the largest DAF (ties: largest index)
        unsigned long long best = 0;
        for (uint32_t i = tid; i < nf; i += nthr) {
          const uint32_t v = list[i];
          if (!alive[v]) continue;
          const unsigned long long key = ((unsigned long long)__float_as_uint(ldaf[i]) << 32) | v;
          if (key >= best) best = key;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
          const unsigned long long ob = __shfl_xor(best, o);
          if (ob > best) best = ob;
        }
        if (lane == 0) ctl.red64[wave] = best;
        __syncthreads();
        best = ctl.red64[0];
        for (int i = 1; i < nwav; i++) if (ctl.red64[i] > best) best = ctl.red64[i];
        target = (uint32_t)best;
        __syncthreads();
        if (gs.nghost > 0 && alive[target] == SW_GHOST) rollback = true;   // a ghost could be the target: its status decides
      }
      if (!rollback) {
      // ---- railroad, trace.py:240-242
      t_target += clock64() - t0; t0 = clock64();
      if (nverts >= pcap || npaths >= pcap) {
        if (tid == 0) atomicOr(&ctl.status, KH_ST_PATH_OVERFLOW);
        __syncthreads();
        break;
      }
      if (!fix_branching) {
        // dijkstra3d.path_from_parents (trace.py:244): walk target -> root, return root -> target
        if (tid == 0) ctl.u0 = 0;
        __syncthreads();
        if (wave == 0) {
          const uint32_t n = backtrack<false>(ctl.g, nbrmask, pdrf, dist, target, root, out, pcap - nverts, q.a, q.b, q.cap,
                                              qstate, &ctl.status, graph);
          for (uint32_t i = lane; i < n / 2; i += 64) { const uint32_t a = out[i]; out[i] = out[n - 1 - i]; out[n - 1 - i] = a; }
          if (lane == 0) ctl.u0 = n;
        }
        __syncthreads();
        plen = ctl.u0;
        if (plen == 0) break;
      } else if (pdrf[target] == 0.0f) {
        if (tid == 0) out[0] = target;
        plen = 1;
      } else {
        sssp<1>(ctl.g, nbrmask, pdrf, dist, qstate, target, q, &ctl, 0.0f, heap_top, lds_bytes);
        plen = rail_walk<true>(ctl, nbrmask, pdrf, dist, qstate, target, q, out, pcap - nverts, graph, nthr);
        __syncthreads();
        if (plen == 0) break;
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
      __syncthreads();
      if (soma) {
        // trace.py:246-251: path = concat(path[:1], path[dist_to_soma_root > soma_radius]) -- path[0] is kept
        // unconditionally AND again if it passes the test itself (the reference duplicates it then).  The
        // distance is float64 like numpy's (float32 anisotropy * int64 offsets -> float64, norm in float64).
        uint32_t* tmp = q.touched;  // free between searches; capacity >= Nf + 64 > plen + 1
        if (wave == 0) {
          const uint32_t sxu = (uint32_t)ctl.g.sx, sxy = (uint32_t)ctl.g.sxy;
          const uint32_t rz = root / sxy, rr = root - rz * sxy, ry = rr / sxu, rx = rr - ry * sxu;
          const double sr = (double)task->soma_radius;
          uint32_t kept = 1;
          if (lane == 0) tmp[0] = out[0];
          for (uint32_t b0 = 0; b0 < plen; b0 += 64) {
            const uint32_t i = b0 + lane;
            bool keep = false;
            uint32_t v = 0;
            if (i < plen) {
              v = out[i];
              const uint32_t z = v / sxy, r = v - z * sxy, y = r / sxu, x = r - y * sxu;
              const double ax = (double)ctl.g.wx * (double)((long long)x - (long long)rx);
              const double ay = (double)ctl.g.wy * (double)((long long)y - (long long)ry);
              const double az = (double)ctl.g.wz * (double)((long long)z - (long long)rz);
              const double d = sqrt(ax * ax + ay * ay + az * az);
              keep = d > sr;
            }
            const unsigned long long m = __ballot(keep);
            if (keep) tmp[kept + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = v;
            kept += (uint32_t)__popcll(m);
          }
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
          if (kept > pcap - nverts) { if (lane == 0) atomicOr(&ctl.status, KH_ST_PATH_OVERFLOW); kept = 0; }
          for (uint32_t i = lane; i < kept; i += 64) out[i] = tmp[i];
          if (lane == 0) ctl.u0 = kept;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __syncthreads();
        plen = ctl.u0;
        __syncthreads();
        if (plen == 0) break;
      }
      t_rail += clock64() - t0;
      }
    } else if (!rollback) {
      plen = __hip_atomic_load(&plens[npaths], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // the path whose invalidation is redone
    }
    // ---- invalidation, trace.py:253-259
    t0 = clock64();
    if (!rollback && valid > 0) {
      if (gs.nghost == 0) {           // (the state a roll-back returns to, should this call make the first ghost)
        gs.jpos = 0; gs.paths = npaths; gs.verts = nverts; gs.valid = valid; gs.nb = nb; gs.na = na;
      }
      const bool go_ghost = ghosts_on && !redo;
      // the call's kill log: the journal once it exists and a ghost is alive; else the first work list (a call that makes the
      // FIRST ghost has its log copied to the journal below -- most labels never need one)
      const bool to_journal = go_ghost && journal != nullptr;
      const uint32_t killed = invalidate<PROF, Heap<TOPL>>(&ctl, &sw, task, nbrmask, dbf, alive, out, plen, scale, constant, heap,
                                                          list, nf, sweep_stats, sg.heap_prio, to_journal ? journal + gs.jpos : q.a,
                                                          go_ghost, redo, gs.nghost == 0, corner_gate, pool);
      if (ctl.u0 != 0u) {
        rollback = true;                                   // the sweep abandoned the call while ghosts exist
      } else {
        const uint32_t made = swsh.nghost, gkilled = swsh.nkg;
        valid -= killed + made;                            // the voxels that are certainly valid
        if (go_ghost) {
          if (made != 0u && journal == nullptr) {
            // the label's first ghost: its journal comes out of the pool now and takes this call's log over
            const uint32_t nlog = killed + gkilled + made;
            __syncthreads();
            journal = journal_off ? nullptr : reinterpret_cast<uint32_t*>(pool_take(pool, (2u * q.cap + 3u) / 4u, &ctl));
            if (journal != nullptr) {
              for (uint32_t i = tid; i < nlog; i += nthr) journal[i] = q.a[i];
            } else {
              journal = q.a;                               // no room: this call is rolled back from its own log, at the top of the
              journal_off = true;                          // next iteration (its path has to be on record first: plens[npaths])
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            __syncthreads();
          }
          gs.nghost += made;
          gs.nghost -= gkilled;
          gs.jpos = gs.nghost ? gs.jpos + killed + gkilled + made : 0u;
          if (made) n_ghost_calls++;
        }
      }
      __syncthreads();                                     // (swsh / ctl are rewritten by the next call)
    }
    t_inval += clock64() - t0;
    if (rollback) {
      // every voxel the journal holds is alive again, the rails of the later paths get their weights back
      for (uint32_t i = tid; i < gs.jpos; i += nthr) {
        const uint32_t v = journal[i];
        alive[v] = 1;
        if (sg.sched != nullptr) sg.sched[v] = SW_SCHED_NONE;
      }
      const uint32_t keep = gs.verts + __hip_atomic_load(&plens[gs.paths], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // the path of the call being redone stays a rail
      if (fix_branching) for (uint32_t i = keep + tid; i < nverts; i += nthr) { const float w = psave[i]; if (w != 0.0f) pdrf[pverts[i]] = w; }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
      __syncthreads();
      npaths = gs.paths; nverts = gs.verts; valid = gs.valid; nb = gs.nb; na = gs.na;
      gs.nghost = 0; gs.jpos = 0;
      if (journal_off) journal = nullptr;
      n_rollbacks++;
      redo = true;
      continue;
    }
    redo = false;
    // ---- rails, trace.py:261-263
    if (fix_branching) for (uint32_t i = tid; i < plen; i += nthr) {
      const uint32_t v = out[i];
      if (psave) psave[nverts + i] = pdrf[v];
      pdrf[v] = 0.0f;
    }
    if (tid == 0) plens[npaths] = plen;
    npaths++;
    nverts += plen;
    __syncthreads();
    if (ctl.status) break;
  }
  __syncthreads();
  if (!fix_branching) {  // leave dist = +inf behind
    for (uint32_t i = tid; i < nf; i += nthr) st_f32_l2(&dist[list[i]], KH_INF);
  }
  if (tid == 0) {
    task->n_paths = npaths;
    task->n_vertices = nverts;
    task->status |= ctl.status;
    search_stats(task, ctl);
    task->stat_settled = ctl.u2;
    task->stat_heap_pushes = ctl.u3;
    task->cyc_target = (uint32_t)(t_target >> 10);
    task->cyc_rail = (uint32_t)(t_rail >> 10);
    task->cyc_inval = (uint32_t)(t_inval >> 10);
    if (PROF) task->cyc_pop = (uint32_t)(ctl.cyc3[0] >> 10);
    if (PROF) task->cyc_push = (uint32_t)(ctl.cyc3[1] >> 10);
    task->cyc_fire = (uint32_t)(ctl.cyc3[2] >> 10);
    sweep_stats_store(task, sweep_stats);
    task->stat_ghost_calls = n_ghost_calls;
    task->stat_rollbacks = n_rollbacks;
  }
}

// ------------------------------------------------------------------------------------------------
// a9 on its own: roll_invalidation_ball_inside_component (skeletontricks.pyx:373-418) for ONE object, the same device
// routine the path loop uses (order-free sweep, heap emulation as the fall-back).
// (the same register bound as the path kernel: the sweep's out-of-line functions are shared, and they inherit the bound of their
// callers only when every kernel that reaches them has it)
__global__ __launch_bounds__(256, KH_TRACE_WAVES_PER_EU) void invalidate_ball_kernel(kh_label_t* task, const uint32_t* __restrict__ lists,
                                                              const uint32_t* __restrict__ nbrmask, Geometry g,
                                                              const float* __restrict__ dbf, uint8_t* alive, uint32_t* queues,
                                                              hnode_t* heap_nodes, const uint32_t* __restrict__ path, uint32_t npath,
                                                              float scale, float constant, SweepGlobal sg, long long* invalidated,
                                                              const uint8_t* __restrict__ corner_gate) {
  __shared__ Ctl ctl;
  __shared__ Sweep sw;
  __shared__ SweepShared swsh;
  __shared__ uint32_t sweep_stats[5];
  extern __shared__ __attribute__((aligned(16))) unsigned char heap_top[];
  const int tid = threadIdx.x, lane = tid & 63;
  const uint32_t nf = task->count;
  Heap<1> heap;
  heap.node = heap_nodes + task->heap_offset;
  heap.top = (lds_hnode_t*)heap_top;
  heap.cap = task->heap_capacity < Heap<1>::MAX_N ? task->heap_capacity : Heap<1>::MAX_N;
  heap.n = 0;
  heap_init_lane(heap, lane);
  if (tid == 0) {
    ctl.status = 0; ctl.u1 = 0; ctl.u3 = 0; ctl.cyc3[0] = ctl.cyc3[1] = ctl.cyc3[2] = 0; ctl.g = g;
    for (int i = 0; i < 5; i++) sweep_stats[i] = 0;
    const Queues q = task_queues(task, queues);
    sweep_setup(sw, &swsh, &ctl, sg, task, nbrmask, alive, q, q.a, nf, heap_top, corner_gate);
  }
  __syncthreads();
  for (uint32_t i = tid; i < sw.spcap; i += blockDim.x) { sw.spk[i] = 0u; sw.spc[i] = 0ull; }   // (the arena is uninitialised memory)
  // the filter words say which voxels of the caller's mask are dead (kh_trace_paths keeps them up to date itself)
  if (sw.sched != nullptr) sweep_reset_words(*(const KH_AS_LDS Sweep*)&sw, lists + task->list_offset, nf);
  __syncthreads();
  const uint32_t c = invalidate<false, Heap<1>>(&ctl, &sw, task, nbrmask, dbf, alive, path, npath, scale, constant, heap,
                                               lists + task->list_offset, nf, sweep_stats, sg.heap_prio,
                                               queues + (uint64_t)task->q_offset * 4, false, false, true, corner_gate);
  if (tid == 0) {
    *invalidated = (long long)c;
    task->status |= ctl.status;
    task->stat_heap_pushes = ctl.u3;
    sweep_stats_store(task, sweep_stats);
  }
}

// ------------------------------------------------------------------------------------------------
// a7 / a8 on their own (the path loop has them inside trace_paths_kernel): one object, one search.
//   mode 0  dijkstra3d.railroad(field, source): search from `src` over the field to the nearest zero-weight voxel,
//           path written rail end first (trace.py:240-242); dist is +inf again on exit.
//   mode 1  the search of dijkstra3d.parental_field(field, source) (trace.py:155): leaves the distance field in `dist`.
//   mode 2  dijkstra3d.path_from_parents (trace.py:244) on that distance field: path src(root) -> dst(target).
__global__ __launch_bounds__(256, KH_TRACE_WAVES_PER_EU) void path_search_kernel(kh_label_t* task, int mode, const uint32_t* __restrict__ lists,
                                                          const uint32_t* __restrict__ nbrmask, Geometry g, const float* pdrf,
                                                          float* dist, uint8_t* qstate, uint32_t* queues, uint32_t src, uint32_t dst,
                                                          uint32_t* out, uint32_t cap, uint32_t* out_n, int graph) {
  __shared__ Ctl ctl;
  __shared__ __attribute__((aligned(16))) unsigned char search_lds[KH_SSSP_LDS_BYTES * 256];
  const int tid = threadIdx.x, nthr = blockDim.x, lane = tid & 63, wave = tid >> 6;
  const Queues q = task_queues(task, queues);
  if (tid == 0) { ctl.status = 0; ctl.u0 = 0; ctl.n_retries = ctl.n_spills = ctl.n_splits = 0; ctl.g = g; }
  __syncthreads();
  if (mode == 1) {
    sssp<2>(ctl.g, nbrmask, pdrf, dist, qstate, src, q, &ctl, 0.0f, search_lds, (uint32_t)sizeof(search_lds));
  } else if (mode == 2) {
    if (wave == 0) {
      const uint32_t n = backtrack<false>(ctl.g, nbrmask, pdrf, dist, dst, src, out, cap, q.a, q.b, q.cap, qstate, &ctl.status, graph != 0);
      for (uint32_t i = lane; i < n / 2; i += 64) { const uint32_t a = out[i]; out[i] = out[n - 1 - i]; out[n - 1 - i] = a; }
      if (lane == 0) ctl.u0 = n;
    }
  } else if (pdrf[src] == 0.0f) {
    if (tid == 0) { out[0] = src; ctl.u0 = 1; }
  } else {
    sssp<1>(ctl.g, nbrmask, pdrf, dist, qstate, src, q, &ctl, 0.0f, search_lds, (uint32_t)sizeof(search_lds));
    rail_walk<false>(ctl, nbrmask, pdrf, dist, qstate, src, q, out, cap, graph != 0, nthr);
  }
  __syncthreads();
  if (tid == 0) {
    *out_n = ctl.u0; task->status |= ctl.status;
    search_stats(task, ctl);
  }
}

// ------------------------------------------------------------------------------------------------
// a7 as arrays: dijkstra3d.parental_field(field, source) returns a parents ARRAY (linear index of the predecessor + 1, 0 = none)
// which trace.py edits (`parents[tuple(root)] = 0`, kimimaro/trace.py:220) and hands to path_from_parents (:244).
// parents_kernel: after the search of path_search_kernel mode 1 has left the distances in `dist`, one thread per voxel of the
// object applies the canonical predecessor rule (oracle ko_pred: the neighbour u with fl(d[u] + f[v]) == d[v] minimising
// (d[u], index of u)).  A voxel all of whose achieving neighbours lie at ITS OWN distance (a float-absorption plateau) has no
// parent that a pointer chase could follow without cycles: KH_ST_PLATEAU, like the oracle's KO_EPLATEAU (the fused path loop and
// kh_path_search mode 2 cross such plateaus by a breadth-first search; a parents array cannot say that).
__global__ __launch_bounds__(256) void parents_kernel(kh_label_t* task, const uint32_t* __restrict__ lists,
                                                      const uint32_t* __restrict__ nbrmask, Geometry g,
                                                      const float* __restrict__ field, const float* __restrict__ dist,
                                                      uint32_t source, uint32_t* parents, int graph) {
  const uint32_t nf = task->count;
  const uint32_t* list = lists + task->list_offset;
  const uint32_t sx = (uint32_t)g.sx, sxy = (uint32_t)g.sxy;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < nf; i += gridDim.x * blockDim.x) {
    const uint32_t v = list[i];
    const float dv = dist[v];
    if (v == source || dv == KH_INF) { parents[v] = 0u; continue; }
    const float fv = field[v];
    const uint32_t nm = nbrmask[v];
    const uint32_t z = v / sxy, r = v - z * sxy, y = r / sx, x = r - y * sx;
    unsigned long long best = NONE64;
    for (int k = 0; k < 26; k++) {
      int dx, dy, dz;
      sweep_dir(k, dx, dy, dz);
      const int nx = (int)x + dx, ny = (int)y + dy, nz = (int)z + dz;
      if (nx < 0 || ny < 0 || nz < 0 || nx >= g.sx || ny >= g.sy || nz >= g.sz) continue;
      const uint32_t u = v + (uint32_t)(dx + (int)sx * dy + (int)sxy * dz);
      bool edge;
      if (!graph) {
        edge = ((nm >> k) & 1u) != 0u;           // symmetric masks: v's own word serves
      } else {
        int opp = 0;                              // the step u -> v is gated by u's word (one-way edges)
        for (int j = 0; j < 26; j++) {
          int ex, ey, ez;
          sweep_dir(j, ex, ey, ez);
          if (ex == -dx && ey == -dy && ez == -dz) opp = j;
        }
        edge = ((nbrmask[u] >> opp) & 1u) != 0u;
      }
      if (!edge) continue;
      const float du = dist[u];
      if (du == KH_INF || du + fv != dv) continue;
      const unsigned long long key = pack(du, u);
      if (key < best) best = key;
    }
    if (best == NONE64) { parents[v] = 0u; continue; }
    if (!(__uint_as_float((uint32_t)(best >> 32)) < dv)) { atomicOr(&task->status, KH_ST_PLATEAU); parents[v] = 0u; continue; }
    parents[v] = (uint32_t)best + 1u;
  }
}

// dijkstra3d.path_from_parents(parents, target) (kimimaro/trace.py:244): a pointer chase target -> source, returned source first.
// One wave: lane 0 chases (a chain of dependent loads by nature), the wave reverses.
__global__ __launch_bounds__(64) void path_from_parents_kernel(const uint32_t* __restrict__ parents, uint32_t nvox, uint32_t target,
                                                               uint32_t* out, uint32_t cap, uint32_t* out_n) {
  __shared__ uint32_t n_sh;
  const int lane = threadIdx.x;
  if (lane == 0) {
    uint32_t n = 0, v = target;
    for (;;) {
      if (n >= cap) { n = 0; break; }             // no room (or a cycle in a caller-edited array): empty path
      out[n++] = v;
      const uint32_t p = parents[v];
      if (p == 0u || p > nvox) break;
      v = p - 1u;
    }
    n_sh = n;
  }
  __syncthreads();
  const uint32_t n = n_sh;
  for (uint32_t i = lane; i < n / 2; i += 64) { const uint32_t a = out[i]; out[i] = out[n - 1 - i]; out[n - 1 - i] = a; }
  if (lane == 0) *out_n = n;
}

// ------------------------------------------------------------------------------------------------
// a10: roll_invalidation_cube.  One workgroup per path vertex; bytes are cleared with a 32-bit
// atomicAnd so each voxel is counted exactly once however many boxes overlap.
__global__ __launch_bounds__(256) void invalidate_cube_kernel(uint8_t* mask, const float* __restrict__ dbf, int sx, int sy,
                                                              int sz, float wx, float wy, float wz,
                                                              const uint64_t* __restrict__ path, float scale,
                                                              float constant, unsigned long long* invalidated) {
  const uint64_t loc = path[blockIdx.x];
  const int64_t sxy = (int64_t)sx * sy;
  float radius = scale * dbf[loc];
  radius = radius + constant;
  const int64_t z = (int64_t)(loc / (uint64_t)sxy), r = (int64_t)(loc % (uint64_t)sxy), y = r / sx, x = r % sx;
  const float rr[3] = {radius / wx, radius / wy, radius / wz};
  const int64_t c[3] = {x, y, z};
  const int64_t s[3] = {sx, sy, sz};
  int64_t lo[3], hi[3];
#pragma unroll
  for (int a = 0; a < 3; a++) {
    const float fl = (float)c[a] - rr[a];              // skeletontricks.hpp:97-102
    int64_t l = (int64_t)fl;
    if (l < 0) l = 0;
    const float fh = (float)c[a] + rr[a];
    const double dh = 0.5 + (double)fh;
    int64_t h = (int64_t)dh;
    if (h > s[a] - 1) h = s[a] - 1;
    lo[a] = l; hi[a] = h;
  }
  const int64_t nx = hi[0] - lo[0] + 1, ny = hi[1] - lo[1] + 1, nz = hi[2] - lo[2] + 1;
  unsigned long long cnt = 0;
  if (nx > 0 && ny > 0 && nz > 0) {
    const int64_t total = nx * ny * nz;
    for (int64_t i = threadIdx.x; i < total; i += 256) {
      const int64_t xx = lo[0] + i % nx, yy = lo[1] + (i / nx) % ny, zz = lo[2] + i / (nx * ny);
      const int64_t qi = xx + sx * yy + sxy * zz;
      uint32_t* word = reinterpret_cast<uint32_t*>(mask + (qi & ~3ll));
      const int sh = (int)(qi & 3) * 8;
      if ((*reinterpret_cast<volatile uint8_t*>(mask + qi)) == 0) continue;
      const uint32_t old = atomicAnd(word, ~(0xFFu << sh));
      if ((old >> sh) & 0xFFu) cnt++;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
  if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(invalidated, cnt);
}

}  // namespace kh

using namespace kh;

extern "C" int kh_edf_batch(kh_label_t* tasks, int ntasks, int mode, const uint32_t* lists, const uint32_t* nbrmask,
                            int64_t sx, int64_t sy, int64_t sz, float wx, float wy, float wz, float* field,
                            uint8_t* qstate, uint32_t* queues, void* stream) {
  if (int rc = require_device()) return rc;
  if (ntasks <= 0) return KH_OK;
  if (sx * sy * sz >= (1ll << 32)) { set_error("kh_edf_batch: volume must have < 2^32 voxels"); return KH_EINVAL; }
  if (((uintptr_t)qstate & 3) != 0) { set_error("kh_edf_batch: qstate must be 4-byte aligned"); return KH_EINVAL; }
  const int nthreads = (mode >> 8) ? (mode >> 8) : 512;
  mode &= 0xFF;
  if (mode < 0 || mode > 2 || nthreads < 64 || nthreads > 1024 || (nthreads & 63)) {
    set_error("kh_edf_batch: mode must be 0, 1 or 2 (+ threads per label << 8: a multiple of 64 up to 1024)");
    return KH_EINVAL;
  }
  Geometry g;
  make_geometry(g, sx, sy, sz, wx, wy, wz);
  float mn = wx < wy ? wx : wy;
  if (wz < mn) mn = wz;
  const float delta_floor = 2.0f * mn;
  // 512 threads per label: measured 0.176 / 0.135 / 0.131 s for the two runs at c3 with 256 / 512 / 1024 threads
  // (one volume alone; with volumes in flight the lanes ask for fewer: a workgroup needs all its waves' slots on one CU at
  // once, and next to thousands of one-wave path workgroups eight free slots rarely come together)
  hipLaunchKernelGGL(edf_batch_kernel, dim3(ntasks), dim3(nthreads), KH_SSSP_LDS_BYTES * nthreads, (hipStream_t)stream, tasks, mode, lists, nbrmask, g, field,
                     qstate, queues, delta_floor);
  KH_LAUNCH_CHECK();
  return KH_OK;
}

namespace kh {
// dynamic LDS of a workgroup that runs the sweep with `nlev` level words: chunk chain, free-chunk stack, level words, bitmap
static size_t sweep_lds_bytes(uint32_t nlev) {
  return ((size_t)SW_CHAIN + SW_RING + nlev + (nlev >> 5) + 2) * 4;
}
// The sweep's launch-wide arguments from the entry points' (level_rank, ra, rb, rc): a table of ranks [ra, rb, rc], or --
// level_rank == NULL and ra > 0 -- integer mode with (gx, gy, gz) = (ra, rb, rc): the squared voxel pitches divided by their
// greatest common divisor gq (checked here against wx, wy, wz).  Returns false on inconsistent arguments.
static bool sweep_global(SweepGlobal& sg, const uint32_t* level_rank, int64_t ra, int64_t rb, int64_t rc, float wx, float wy, float wz,
                         uint64_t* cstate, uint32_t* sched, void* event_arena, int64_t max_nlev) {
  sg.on = 0u; sg.gq = sg.gx = sg.gy = sg.gz = 0u;
  sg.rank = level_rank;
  sg.ra = (int)ra; sg.rb = (int)rb; sg.rc = (int)rc;
  sg.cstate = reinterpret_cast<unsigned long long*>(cstate);
  sg.sched = sched;
  sg.arena = reinterpret_cast<unsigned char*>(event_arena);
  sg.lds_levels = (uint32_t)max_nlev;
  sg.heap_prio = 0u;
  if (level_rank == nullptr && ra <= 0) return true;                    // sweep off
  if (!cstate || !sched || !event_arena || ra <= 0 || rb <= 0 || rc <= 0 || max_nlev < 0 || max_nlev > KH_SWEEP_LDS_LEVELS ||
      ((uintptr_t)event_arena & 255) != 0)
    return false;
  if (level_rank == nullptr) {
    const double qx = (double)wx * wx, qy = (double)wy * wy, qz = (double)wz * wz;
    const double gq = qx / (double)ra;
    if (!(gq >= 1.0) || gq != (double)(uint32_t)gq || gq * (double)rb != qy || gq * (double)rc != qz || qx > 4.0e9 || qy > 4.0e9 ||
        qz > 4.0e9)
      return false;
    sg.gq = (uint32_t)gq; sg.gx = (uint32_t)ra; sg.gy = (uint32_t)rb; sg.gz = (uint32_t)rc;
  }
  sg.on = 1u;
  return true;
}
static int sweep_args_error(const char* entry) {
  set_error("%s: sweep arguments (level table or integer-mode factors, cstate, sched, a 256-byte aligned event arena, max_nlev)", entry);
  return KH_EINVAL;
}
// Dynamic LDS of a launch of `kernel` whose workgroups run the heap emulation, the sweep and -- search_threads != 0 -- the searches
// in the same bytes: the largest of the heap's LDS part with its key mirror (heap_bytes), the sweep's words for max_nlev levels
// when the sweep is on, and the searches' scratch.  Allows the kernel that much as well.
static int trace_lds_bytes(const void* kernel, size_t heap_bytes, const SweepGlobal& sg, uint32_t max_nlev, unsigned search_threads,
                           size_t& lds) {
  lds = heap_bytes;
  const size_t swl = sweep_lds_bytes(max_nlev);
  if (sg.on && swl > lds) lds = swl;
  if ((size_t)KH_SSSP_LDS_BYTES * search_threads > lds) lds = (size_t)KH_SSSP_LDS_BYTES * search_threads;
  // More than 48 KiB of dynamic LDS has to be allowed per kernel.  The attribute belongs to the function, not to the
  // launch, and several host threads launch at once (kimimaro_amd/lanes.py): always the same value -- the largest a
  // launch can ask for -- so that a concurrent caller never lowers it under somebody else's launch.
  const size_t lds_max = sweep_lds_bytes(KH_SWEEP_LDS_LEVELS);
  KH_HIP_CHECK(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(lds_max > lds ? lds_max : lds)));
  return KH_OK;
}
// what trace_paths_kernel takes (in its order), and the launch's shape
struct TraceArgs {
  int count; unsigned nthreads; uint32_t max_nlev; hipStream_t st;
  kh_label_t* tasks; const uint32_t* lists; float* list_daf; const uint32_t* nbrmask; Geometry g; const float* dbf;
  float *pdrf, *dist; uint8_t *alive, *qstate; const uint32_t* manual_targets; float scale, constant; uint32_t* queues;
  hnode_t* heap_nodes; uint32_t *path_vertices, *path_lengths; int fix_branching; SweepGlobal sg; uint32_t* journal;
  float* rail_save; uint32_t ghost_mode; const uint8_t* corner_gate;
};
template <bool PROF, int TOPL = 1>
static int launch_trace(const TraceArgs& a) {
  if (a.count <= 0) return KH_OK;
  size_t lds;
  if (int rc = trace_lds_bytes(reinterpret_cast<const void*>(&trace_paths_kernel<PROF, TOPL>), Heap<TOPL>::LDS_BYTES, a.sg, a.max_nlev,
                               a.nthreads, lds))
    return rc;
  hipLaunchKernelGGL((trace_paths_kernel<PROF, TOPL>), dim3(a.count), dim3(a.nthreads), lds, a.st, a.tasks, a.lists, a.list_daf,
                     a.nbrmask, a.g, a.dbf, a.pdrf, a.dist, a.alive, a.qstate, a.manual_targets, a.scale, a.constant, a.queues,
                     a.heap_nodes, a.path_vertices, a.path_lengths, a.fix_branching, a.sg, a.journal, a.rail_save, a.ghost_mode,
                     a.corner_gate, (uint32_t)lds);
  KH_LAUNCH_CHECK();
  return KH_OK;
}

// key of the offset (a, b, c) exactly as the flood computes it (dijkstra_invalidation.hpp:310-316)
__global__ __launch_bounds__(256) void level_keys_kernel(int ra, int rb, int rc, float wx, float wy, float wz, float* keys) {
  const int64_t n = (int64_t)ra * rb * rc;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int a = (int)(i % ra), b = (int)((i / ra) % rb), c = (int)(i / ((int64_t)ra * rb));
  const float fa = wx * (float)a, fb = wy * (float)b, fc = wz * (float)c;
  float s = fa * fa;
  const float t = fb * fb;
  const float u = fc * fc;
  s = s + t;
  s = s + u;
  keys[i] = sqrtf(s);
}
}  // namespace kh

extern "C" int kh_level_keys(int64_t ra, int64_t rb, int64_t rc, float wx, float wy, float wz, float* keys, void* stream) {
  if (int rc2 = require_device()) return rc2;
  if (ra <= 0 || rb <= 0 || rc <= 0 || ra * rb * rc >= (1ll << 31)) { set_error("kh_level_keys: bad table size"); return KH_EINVAL; }
  const int64_t n = ra * rb * rc;
  hipLaunchKernelGGL(level_keys_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (int)ra, (int)rb,
                     (int)rc, wx, wy, wz, keys);
  KH_LAUNCH_CHECK();
  return KH_OK;
}

extern "C" int kh_trace_paths(kh_label_t* tasks, int ntasks, const uint32_t* lists, float* list_daf,
                              const uint32_t* nbrmask, int64_t sx, int64_t sy, int64_t sz, float wx, float wy, float wz,
                              const float* dbf, float* pdrf, float* dist, uint8_t* alive, uint8_t* qstate,
                              const uint32_t* manual_targets, float scale, float constant, uint32_t* queues,
                              void* heap_nodes, uint32_t* path_vertices, uint32_t* path_lengths,
                              const uint32_t* level_rank, int64_t ra, int64_t rb, int64_t rc, int64_t max_nlev,
                              uint64_t* cstate, uint32_t* sched, void* event_arena, uint32_t* journal, float* rail_save,
                              const uint8_t* corner_gate, int flags, int fix_branching, void* stream) {
  if (int rc2 = require_device()) return rc2;
  if (ntasks <= 0) return KH_OK;
  if (sx * sy * sz >= (1ll << 32)) { set_error("kh_trace_paths: volume must have < 2^32 voxels"); return KH_EINVAL; }
  if (((uintptr_t)qstate & 3) != 0) { set_error("kh_trace_paths: qstate must be 4-byte aligned"); return KH_EINVAL; }
  if (((uintptr_t)heap_nodes & 15) != 0) { set_error("kh_trace_paths: heap_nodes must be 16-byte aligned"); return KH_EINVAL; }
  if ((flags & ~(KH_TRACE_PROFILE | KH_TRACE_HEAP_PRIO | KH_TRACE_THREADS_64 | KH_TRACE_THREADS_128 | KH_TRACE_NO_GHOSTS |
                 KH_TRACE_GHOST_PARANOID | KH_TRACE_BIG_LDS_HEAP | KH_TRACE_VOXEL_GRAPH | KH_TRACE_SCRATCH_POOL | KH_TRACE_FUSED_EDF)) ||
      ((flags & KH_TRACE_THREADS_64) && (flags & KH_TRACE_THREADS_128))) {
    set_error("kh_trace_paths: unknown flags");
    return KH_EINVAL;
  }
  const unsigned nthreads = (flags & KH_TRACE_THREADS_64) ? 64u : (flags & KH_TRACE_THREADS_128) ? 128u : 256u;
  Geometry g;
  make_geometry(g, sx, sy, sz, wx, wy, wz);
  SweepGlobal sg;
  if (!sweep_global(sg, level_rank, ra, rb, rc, wx, wy, wz, cstate, sched, event_arena, max_nlev)) return sweep_args_error("kh_trace_paths");
  sg.heap_prio = (flags & KH_TRACE_HEAP_PRIO) ? 1u : 0u;
  // ghosts need the journal (and, with rails, the saved weights); bit 1: roll every ghost call back at once
  const bool use_pool = (flags & KH_TRACE_SCRATCH_POOL) != 0;
  const uint32_t ghost_mode = ((journal || use_pool) && !(flags & KH_TRACE_NO_GHOSTS) ? 1u : 0u) | ((flags & KH_TRACE_GHOST_PARANOID) ? 2u : 0u) |
                              ((flags & KH_TRACE_VOXEL_GRAPH) ? 4u : 0u) | (use_pool ? 8u : 0u) | ((flags & KH_TRACE_FUSED_EDF) ? 16u : 0u);
  const TraceArgs a = {ntasks, nthreads, (uint32_t)max_nlev, (hipStream_t)stream, tasks, lists, list_daf, nbrmask, g, dbf, pdrf, dist,
                       alive, qstate, manual_targets, scale, constant, queues, (hnode_t*)heap_nodes, path_vertices, path_lengths,
                       fix_branching, sg, journal, rail_save, ghost_mode, corner_gate};
  if (flags & KH_TRACE_BIG_LDS_HEAP) return launch_trace<false, 2>(a);
  if (flags & KH_TRACE_PROFILE) return launch_trace<true>(a);
  return launch_trace<false>(a);
}

extern "C" int kh_invalidate_ball(kh_label_t* task, const uint32_t* lists, const uint32_t* nbrmask, int64_t sx, int64_t sy,
                                  int64_t sz, float wx, float wy, float wz, const float* dbf, uint8_t* alive, uint32_t* queues,
                                  void* heap_nodes, const uint32_t* path, int64_t npath, float scale, float constant,
                                  const uint32_t* level_rank, int64_t ra, int64_t rb, int64_t rc, int64_t max_nlev,
                                  uint64_t* cstate, uint32_t* sched, void* event_arena, const uint8_t* corner_gate,
                                  int64_t* invalidated, void* stream) {
  if (int rc2 = require_device()) return rc2;
  if (!task || !lists || !nbrmask || !dbf || !alive || !queues || !heap_nodes || !path || !invalidated || npath < 0 ||
      npath >= (1ll << 32) || sx * sy * sz >= (1ll << 32) || ((uintptr_t)heap_nodes & 15) != 0) {
    set_error("kh_invalidate_ball: bad arguments");
    return KH_EINVAL;
  }
  Geometry g;
  make_geometry(g, sx, sy, sz, wx, wy, wz);
  SweepGlobal sg;
  if (!sweep_global(sg, level_rank, ra, rb, rc, wx, wy, wz, cstate, sched, event_arena, max_nlev)) return sweep_args_error("kh_invalidate_ball");
  size_t lds;
  if (int rc2 = trace_lds_bytes(reinterpret_cast<const void*>(&invalidate_ball_kernel), Heap<1>::LDS_BYTES, sg, (uint32_t)max_nlev, 0u, lds))
    return rc2;
  hipLaunchKernelGGL(invalidate_ball_kernel, dim3(1), dim3(256), lds, (hipStream_t)stream, task, lists, nbrmask, g, dbf, alive, queues,
                     (hnode_t*)heap_nodes, path, (uint32_t)npath, scale, constant, sg, (long long*)invalidated, corner_gate);
  KH_LAUNCH_CHECK();
  return KH_OK;
}

extern "C" int kh_path_search(kh_label_t* task, int mode, const uint32_t* lists, const uint32_t* nbrmask, int64_t sx, int64_t sy,
                              int64_t sz, float wx, float wy, float wz, const float* field, float* dist, uint8_t* qstate,
                              uint32_t* queues, uint64_t source, uint64_t target, uint32_t* path, int64_t path_capacity,
                              uint32_t* path_length, int voxel_graph, void* stream) {
  if (int rc2 = require_device()) return rc2;
  if (!task || !lists || !nbrmask || !field || !dist || !qstate || !queues || !path_length || mode < 0 || mode > 2 ||
      (mode != 1 && !path) || sx * sy * sz >= (1ll << 32) || path_capacity < 0 || path_capacity >= (1ll << 32) ||
      ((uintptr_t)qstate & 3) != 0) {
    set_error("kh_path_search: bad arguments");
    return KH_EINVAL;
  }
  Geometry g;
  make_geometry(g, sx, sy, sz, wx, wy, wz);
  hipLaunchKernelGGL(path_search_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, task, mode, lists, nbrmask, g, field, dist, qstate,
                     queues, (uint32_t)source, (uint32_t)target, path, (uint32_t)path_capacity, path_length, voxel_graph);
  KH_LAUNCH_CHECK();
  return KH_OK;
}

extern "C" int kh_invalidate_cube(uint8_t* mask, const float* dbf, int64_t sx, int64_t sy, int64_t sz, float wx, float wy,
                                  float wz, const uint64_t* path, int64_t npath, float scale, float constant,
                                  int64_t* invalidated, void* stream) {
  if (int rc = require_device()) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (((uintptr_t)mask & 3) != 0) { set_error("kh_invalidate_cube: mask must be 4-byte aligned"); return KH_EINVAL; }
  KH_HIP_CHECK(hipMemsetAsync(invalidated, 0, sizeof(int64_t), st));
  if (npath <= 0) return KH_OK;
  hipLaunchKernelGGL(invalidate_cube_kernel, dim3((unsigned)npath), dim3(256), 0, st, mask, dbf, (int)sx, (int)sy, (int)sz, wx,
                     wy, wz, path, scale, constant, (unsigned long long*)invalidated);
  KH_LAUNCH_CHECK();
  return KH_OK;
}

extern "C" int kh_parental_field(kh_label_t* task, const uint32_t* lists, const uint32_t* nbrmask, int64_t sx, int64_t sy, int64_t sz,
                                 const float* field, float* dist, uint8_t* qstate, uint32_t* queues, uint64_t source,
                                 uint32_t* parents, int voxel_graph, void* stream) {
  if (int rc2 = require_device()) return rc2;
  if (!task || !lists || !nbrmask || !field || !dist || !qstate || !queues || !parents || sx * sy * sz >= (1ll << 32) ||
      source >= (uint64_t)(sx * sy * sz) || ((uintptr_t)qstate & 3) != 0) {
    set_error("kh_parental_field: bad arguments");
    return KH_EINVAL;
  }
  Geometry g;
  make_geometry(g, sx, sy, sz, 1.0f, 1.0f, 1.0f);     // (field costs: the edge lengths are not used)
  hipStream_t st = (hipStream_t)stream;
  KH_HIP_CHECK(hipMemsetAsync(parents, 0, (size_t)(sx * sy * sz) * sizeof(uint32_t), st));
  hipLaunchKernelGGL(path_search_kernel, dim3(1), dim3(256), 0, st, task, 1, lists, nbrmask, g, field, dist, qstate, queues,
                     (uint32_t)source, 0u, (uint32_t*)nullptr, 0u, parents /* out_n: overwritten below */, voxel_graph);
  KH_LAUNCH_CHECK();
  hipLaunchKernelGGL(parents_kernel, dim3(256), dim3(256), 0, st, task, lists, nbrmask, g, field, dist, (uint32_t)source, parents,
                     voxel_graph);
  KH_LAUNCH_CHECK();
  return KH_OK;
}

extern "C" int kh_path_from_parents(const uint32_t* parents, int64_t nvox, uint64_t target, uint32_t* path, int64_t path_capacity,
                                    uint32_t* path_length, void* stream) {
  if (int rc2 = require_device()) return rc2;
  if (!parents || !path || !path_length || nvox <= 0 || nvox >= (1ll << 32) || target >= (uint64_t)nvox || path_capacity <= 0 ||
      path_capacity >= (1ll << 32)) {
    set_error("kh_path_from_parents: bad arguments");
    return KH_EINVAL;
  }
  hipLaunchKernelGGL(path_from_parents_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, parents, (uint32_t)nvox, (uint32_t)target,
                     path, (uint32_t)path_capacity, path_length);
  KH_LAUNCH_CHECK();
  return KH_OK;
}
