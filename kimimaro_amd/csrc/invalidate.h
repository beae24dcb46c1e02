// invalidate.h -- one invalidation call of a label: the glue between the order-free sweep (sweep.h) and the heap emulation
// (heap.h) -- SweepGlobal, the scratch pool, invalidate, sweep_setup, the sweep counters' write-back and the ghosts' state.
// Needs sweep.h, heap.h and search_state.h (Ctl, Queues).
#pragma once
#include "heap.h"
#include "search_state.h"
#include "sweep.h"

namespace kh {

// everything the order-free sweep needs besides the per-label task record
struct SweepGlobal {
  uint32_t on;                  // 0 = sweep disabled (every invalidation runs as the heap emulation)
  uint32_t gq, gx, gy, gz;      // integer mode (sweep.h): key^2 = gq * (gx a^2 + gy b^2 + gz c^2); gq == 0: table mode
  const uint32_t* rank;         // table mode: level table [ra * rb * rc]
  int ra, rb, rc;
  unsigned long long* cstate;   // one word per voxel, all zero on entry and on exit
  uint32_t* sched;              // one word per voxel (sweep.h, pending-deadline filter), SW_SCHED_NONE for live voxels; nullable
  unsigned char* arena;         // event arenas (per label: kh_label_t.ev_offset, in units of 256 bytes)
  uint32_t lds_levels;          // labels with more levels keep their level words in the arena instead of LDS
  uint32_t heap_prio;           // != 0: the wave that runs the heap emulation raises its issue priority (s_setprio 3)
};

// Scratch on demand (round 6).  The heap of the exact emulation (16 B x 1.5 nodes per voxel) and the ghosts' journal (8 B per voxel)
// were reserved for every label of a launch; 141 of c3's 3 402 labels ever run the emulation and 360 ever hold a ghost -- 4.6 GB per
// volume in flight for 0.4 GB of use, and the volumes in flight are bounded by memory.  With KH_TRACE_SCRATCH_POOL `heap_nodes` is
// ONE pool for the launch: node 0 = {nodes handed out so far (starts at 1), nodes in the pool}; a label takes what it needs when it
// first needs it (one atomic add by one thread).  A label the pool cannot serve ends with KH_ST_HEAP_OVERFLOW (heap) -- the host
// traces it again with scratch of its own, like every other overflow -- or goes on without ghosts (journal).
// Whole workgroup; returns nullptr when the pool is exhausted.
__device__ __forceinline__ hnode_t* pool_take(hnode_t* pool, uint32_t nodes, Ctl* ctl) {
  if (threadIdx.x == 0) {
    uint32_t* hdr = reinterpret_cast<uint32_t*>(pool);
    const uint32_t cap = hdr[1];
    uint32_t base = 0u;
    if (nodes != 0u && nodes < cap) {
      base = atomicAdd(&hdr[0], nodes);
      if (base + nodes > cap || base + nodes < base) base = 0u;
    }
    ctl->pool_base = base;
  }
  __syncthreads();
  const uint32_t b = ctl->pool_base;
  __syncthreads();
  return b ? pool + b : nullptr;
}

// One invalidation call by the whole workgroup: the order-free sweep when the label has a level table and the sweep
// certifies the call, the heap emulation (wave 0) otherwise.  Returns the number of voxels invalidated (ghosts that were killed
// not counted: sw->sh->nkg; ghosts made: sw->sh->nghost -- both zero unless allow_ghosts).
//   kill_log      where the sweep logs the voxels it kills (+ the ghosts it makes): the label's journal in ghost mode
//   allow_ghosts  a call that leaves voxels undecided ends as certified, the voxels become ghosts (sweep.h)
//   force_heap    skip the sweep (the redo of a call after a roll-back)
//   heap_ok       false while ghosts exist: the heap emulation needs the exact mask, so a call the sweep abandons cannot be
//                 redone here -- ctl->u0 = 1 tells the caller to roll back (nothing has been changed)
template <bool PROF, class H>
__device__ __forceinline__ uint32_t invalidate(Ctl* ctl, Sweep* sw, kh_label_t* task, const uint32_t* __restrict__ nbrmask,
                                               const float* __restrict__ dbf, uint8_t* alive, const uint32_t* path, uint32_t npath,
                                               float scale, float constant, H& heap, const uint32_t* list, uint32_t nf,
                                               uint32_t* sweep_stats, uint32_t heap_prio, uint32_t* kill_log,
                                               bool allow_ghosts = false, bool force_heap = false, bool heap_ok = true,
                                               const uint8_t* __restrict__ corner_gate = nullptr, hnode_t* pool = nullptr) {
  const int tid = threadIdx.x;
  bool ok = false;
  if (tid == 0) {
    sw->killed = (KH_AS_GLOBAL uint32_t*)kill_log;
    sw->sh->nkg = 0u; sw->sh->nghost = 0u;
    ctl->u0 = 0u;
  }
  __syncthreads();
  if (!force_heap && sw->nlev != 0u && npath > 0 && npath <= 32766u && npath <= nf) {
    const long long got = sweep_ball(*(const KH_AS_LDS Sweep*)sw, path, npath, dbf, scale, constant, task->sweep_rmax, list, nf, allow_ghosts);
    ok = got >= 0;
    const uint32_t cnt = ok ? (uint32_t)got : 0u;
    if (tid == 0) {
      sweep_stats[0]++;
      sweep_stats[2] += sw->sh->levels;
      sweep_stats[3] += sw->sh->events;
#ifdef KH_SWEEP_PROBE
      if (blockIdx.x == 0 || blockIdx.x == 100 || blockIdx.x == 1000 || blockIdx.x == 2500)
        printf("SWCYC blk=%u nf=%u ok=%d lev=%u ev=%u commit=%llu next=%llu A=%llu cascA=%llu B=%llu cascB=%llu pairs=%llu "
               "dn=%llu d_own=%llu d_alive=%llu d_rank=%llu d_sched=%llu d_casc=%llu d_push=%llu\n", blockIdx.x, nf, (int)ok,
               sw->sh->levels, sw->sh->events, sw->sh->cyc[0], sw->sh->cyc[1], sw->sh->cyc[2], sw->sh->cyc[3], sw->sh->cyc[6],
               sw->sh->cyc[4], sw->sh->cyc[5], sw->sh->cyd[7], sw->sh->cyd[0], sw->sh->cyd[1], sw->sh->cyd[2], sw->sh->cyd[3],
               sw->sh->cyd[4], sw->sh->cyd[5]);
#endif
      if (!ok) { sweep_stats[1]++; sweep_stats[4] |= sw->sh->bail; sw->sh->nkg = 0u; sw->sh->nghost = 0u; }
      if (sw->sh->maxnev > task->cyc_pop) task->cyc_pop = sw->sh->maxnev;   // diagnostic: busiest level
      if (sw->sh->bump > task->cyc_push) task->cyc_push = sw->sh->bump;      // diagnostic: arena blocks used
      ctl->u1 = cnt;
    }
  } else if (tid == 0 && force_heap) {
    sweep_stats[1]++; sweep_stats[4] |= SW_BAIL_M;       // a call redone by the heap emulation after a roll-back
  }
  if (!ok && !heap_ok) {
    if (tid == 0) { ctl->u0 = 1u; ctl->u1 = 0u; }
    __syncthreads();
    return 0u;
  }
  if (!ok && heap.node == nullptr) {
    // the label's first call of the heap emulation: its heap comes out of the launch's pool now
    heap.node = pool != nullptr ? pool_take(pool, heap.cap, ctl) : nullptr;
    if (heap.node == nullptr) {
      if (tid == 0) { ctl->status |= KH_ST_HEAP_OVERFLOW; ctl->u1 = 0u; }
      __syncthreads();
      return 0u;
    }
  }
  if (!ok) {
    __syncthreads();
    if (tid < 64) {
      // The heap emulation is ONE sequential chain (a third of its time is instruction issue, the rest its own dependent
      // loads) and it sets the wall clock of the label; the waves it shares its SIMD with -- other labels' sweeps and
      // searches -- are throughput work.  With several volumes in flight they compete for issue slots all the time.
      if (heap_prio) __builtin_amdgcn_s_setprio(3);
      const uint32_t c = invalidate_ball<PROF, H>(ctl->g, task, nbrmask, dbf, alive, path, npath, scale, constant, heap,
                                                  &ctl->status, &ctl->u3, ctl->cyc3, corner_gate);
      if (heap_prio) __builtin_amdgcn_s_setprio(0);
      if (tid == 0) ctl->u1 = c;
    }
    // the sweep reads "dead" from the filter words: bring them in line with the mask the heap emulation has edited (a pass over the
    // label's voxels by the whole workgroup, once per such call -- a store per kill inside the emulation would sit on its chain)
    if (sw->sched != nullptr && sw->nlev != 0u) {
      __syncthreads();
      sweep_reset_words(*(const KH_AS_LDS Sweep*)sw, list, nf);
    }
  }
  __syncthreads();
  const uint32_t c = ctl->u1;
  __syncthreads();
  return c;
}

// thread 0, at the end of a kernel: the five counters `invalidate` keeps per label (calls, bails, levels, events, why)
__device__ __forceinline__ void sweep_stats_store(kh_label_t* task, const uint32_t* sweep_stats) {
  task->stat_sweep_calls = sweep_stats[0];
  task->stat_sweep_bails = sweep_stats[1];
  task->stat_sweep_levels = sweep_stats[2];
  task->stat_sweep_events = sweep_stats[3];
  task->stat_sweep_why = sweep_stats[4];
}

// thread 0: fill the workgroup's Sweep record for `task` (LDS carve-out `lds` = the dynamic shared memory).  The kernel's
// pointers get their address spaces here (sweep.h works on typed pointers only).
__device__ __forceinline__ void sweep_setup(Sweep& sw, SweepShared* swsh, Ctl* ctl, const SweepGlobal& sg, const kh_label_t* task,
                                            const uint32_t* nbrmask, uint8_t* alive, const Queues& q, uint32_t* killed,
                                            uint32_t nf, unsigned char* lds, const uint8_t* corner_gate = nullptr) {
  typedef KH_AS_GLOBAL unsigned char gbyte_t;
  uint32_t nlev = (sg.on && sg.sched != nullptr) ? task->nlev : 0u;
  sw.g = (const KH_AS_LDS Geometry*)&ctl->g;
  sw.nbrmask = (const KH_AS_GLOBAL uint32_t*)nbrmask;
  sw.alive = (KH_AS_GLOBAL uint8_t*)alive;
  sw.cstate = (KH_AS_GLOBAL unsigned long long*)sg.cstate;
  sw.sched = (KH_AS_GLOBAL uint32_t*)sg.sched;
  sw.gq = sg.gq; sw.gx = sg.gx; sw.gy = sg.gy; sw.gz = sg.gz;
  sw.rank = (const KH_AS_GLOBAL uint32_t*)sg.rank;
  sw.ra = sg.ra; sw.rb = sg.rb;
  // The searches' work lists (four of q.cap >= nf + 64 words) are free while an invalidation runs: the first is the kill log, the
  // fourth (`touched`) holds the source records, the two between them the three lists of the level being processed (20 bytes per
  // entry of each; a list that runs over abandons the call, SW_BAIL_LIST; so do more path vertices than records fit).  Round 5 kept
  // all of this in the label's heap slice, which since round 6 only exists once the label needs the heap emulation.
  {
    const uintptr_t t0 = ((uintptr_t)q.touched + 15u) & ~(uintptr_t)15u;
    sw.srcs = (KH_AS_GLOBAL u32x4_t*)(gbyte_t*)t0;
    sw.srcs_cap = (uint32_t)(((uintptr_t)(q.touched + q.cap) - t0) / 16u);
    const uintptr_t b0 = ((uintptr_t)q.b + 7u) & ~(uintptr_t)7u;
    sw.ncap = (uint32_t)(((uintptr_t)(q.b + 2u * (size_t)q.cap) - b0) / 20u);
    sw.wa = (KH_AS_GLOBAL unsigned long long*)(gbyte_t*)b0;
    sw.np = sw.wa + sw.ncap;
    sw.wb = (KH_AS_GLOBAL uint32_t*)(sw.np + sw.ncap);
  }
  // level words + non-empty bitmap live in LDS: a window of them (kh_label_t.lev_window), or one per level when that fits the
  // launch's allotment; a label for which neither does runs without the sweep (heap emulation only)
  const uint32_t win = task->lev_window;
  const bool windowed = win >= 64u && (win & (win - 1u)) == 0u && win <= sg.lds_levels;   // round-robin words
  if (!windowed && nlev > sg.lds_levels) nlev = 0u;
  sw.nslots = windowed ? win : nlev;
  sw.wmask = windowed ? win - 1u : 0xFFFFFFFFu;
  // arena: [spill table: ev_spill candidate words (u64) + ev_spill keys (u32)][(free stack of rounds 4-5: unused)][chunks]
  gbyte_t* fsp = (gbyte_t*)(sg.arena + (size_t)task->ev_offset * 256u);
  const uint32_t spcap = task->ev_spill;          // 0 or a power of two
  sw.spcap = (spcap & (spcap - 1u)) == 0u ? spcap : 0u;
  sw.spc = (KH_AS_GLOBAL unsigned long long*)fsp;
  sw.spk = (KH_AS_GLOBAL uint32_t*)(fsp + (size_t)sw.spcap * 8u);
  fsp += (((size_t)sw.spcap * 12u) + 255u) & ~(size_t)255u;
  sw.chunks = (KH_AS_GLOBAL u32x2_t*)(fsp + ((((size_t)task->ev_chunks * 4u) + 255u) & ~(size_t)255u));
  sw.chcap = task->ev_chunks;
  sw.shift = (int)task->ev_shift;
  sw.killed = (KH_AS_GLOBAL uint32_t*)killed;              // the search work lists are free during an invalidation
  sw.nlev = nlev;                                          // 0: this label's invalidations run as the heap emulation
  sw.chain = (KH_AS_LDS uint32_t*)lds;
  sw.fs = sw.chain + SW_CHAIN;
  sw.words = sw.fs + SW_RING;
  sw.lvbits = sw.words + sw.nslots;
  sw.sh = (KH_AS_LDS SweepShared*)swsh;
  sw.gate = (const KH_AS_GLOBAL uint8_t*)corner_gate;
  sw.xmin = task->xmin; sw.xmax = task->xmax;
}

// Ghosts and roll-back.  A call of the sweep that leaves voxels undecided no longer runs the heap emulation
// at once: the voxels become ghosts (sweep.h) and the loop goes on -- everything the later calls decide holds under either status
// of a ghost, and most ghosts are killed for certain by a later ball.  The loop itself must never act on a ghost: when a ghost
// could be the next target, when no certainly-valid voxel is left while ghosts are, or when a later call would need the heap
// emulation (which needs the exact mask), the label ROLLS BACK to the call that made the first ghost -- the journal holds every
// voxel that changed since (killed or made a ghost: all alive again), the rails of the later paths get their weights back -- and
// that call is redone by the exact heap emulation; then the loop continues from there, without ghosts.
struct GhostState {
  uint32_t nghost;       // ghosts alive now
  uint32_t jpos;         // journal entries (0 whenever no ghost exists)
  uint32_t paths, verts, valid, nb, na;   // the state before the call that made the first ghost
};

}  // namespace kh
