// search_state.h -- what every per-label machine of trace.hip shares: the workgroup's control record (Ctl), the label's work
// lists (Queues), the membership-flag helpers and the agent-scope (L2) loads and stores of words that atomics change.
// Needs common.h only (Geometry, kh_label_t, the address-space macros).
#pragma once
#include "common.h"

namespace kh {

static constexpr uint32_t INF_BITS = 0x7f800000u;
static constexpr unsigned long long NONE64 = ~0ull;

__device__ __forceinline__ float ld_f32_l2(const float* p) {
  // dist words are modified by L2 atomics; read them at agent scope (bypasses the per-CU L1)
  return __uint_as_float(__hip_atomic_load(reinterpret_cast<const uint32_t*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}
__device__ __forceinline__ void st_f32_l2(float* p, float v) {
  __hip_atomic_store(reinterpret_cast<uint32_t*>(p), __float_as_uint(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ unsigned long long pack(float d, uint32_t v) {
  return ((unsigned long long)__float_as_uint(d) << 32) | v;
}
__device__ __forceinline__ float next_up(float x) { return __uint_as_float(__float_as_uint(x) + 1u); }
// read lane `l` (wave-uniform index) of a 32-bit value: v_readlane instead of a ds_bpermute round trip
__device__ __forceinline__ uint32_t rdlane_u32(uint32_t v, int l) {
  return (uint32_t)__builtin_amdgcn_readlane((int)v, __builtin_amdgcn_readfirstlane(l));
}
struct Ctl {
  unsigned long long best_rail;
  unsigned long long red64[16];
  uint32_t n_cur, n_next, n_far, n_far2, n_touched;
  uint32_t status;
  float red_min[16];
  float red_sum[16];
  uint32_t red_cnt[16];
  float T;
  uint32_t u0, u1, u2, u3;
  uint32_t retry[2];     // sssp: a frontier voxel of this batch could not place an offer (parity of the batch)
  uint32_t pool_base;
  uint32_t n_retries, n_spills, n_splits;   // sssp's regime counters (kh_label_t.stat_search_*): zeroed by the kernel, thread 0 counts
  unsigned long long cyc3[3];
  Geometry g;  // the 26 offsets / edge lengths are indexed per lane: keep them in LDS, not in SGPRs
};
// thread 0, at the end of a kernel: the regime counters of the searches it ran
__device__ __forceinline__ void search_stats(kh_label_t* task, const Ctl& ctl) {
  task->stat_search_retries += ctl.n_retries; task->stat_search_spills += ctl.n_spills; task->stat_search_splits += ctl.n_splits;
}

// work lists hold voxel indices only; membership is tracked by two bits per voxel in `qstate`
// (bit0: queued in the near list being built, bit1: queued in the far list), so a voxel is in each
// list at most once and every list is bounded by the label size Nf.
struct Queues {
  uint32_t* a;
  uint32_t* b;
  uint32_t* c;
  uint32_t* touched;
  uint32_t cap;
};
// the label's four work lists of q_capacity words each, carved out of the launch's `queues`
__device__ __forceinline__ Queues task_queues(const kh_label_t* task, uint32_t* queues) {
  Queues q;
  q.cap = task->q_capacity;
  q.a = queues + (uint64_t)task->q_offset * 4;
  q.b = q.a + q.cap;
  q.c = q.b + q.cap;
  q.touched = q.c + q.cap;
  return q;
}

__device__ __forceinline__ uint32_t flag_or(uint8_t* base, uint32_t v, uint32_t bit) {
  uint32_t* w = reinterpret_cast<uint32_t*>(base + (v & ~3u));
  const int sh = (int)(v & 3u) * 8;
  return (atomicOr(w, bit << sh) >> sh) & 0xFFu;
}
__device__ __forceinline__ void flag_clear(uint8_t* base, uint32_t v, uint32_t bit) {
  uint32_t* w = reinterpret_cast<uint32_t*>(base + (v & ~3u));
  const int sh = (int)(v & 3u) * 8;
  atomicAnd(w, ~(bit << sh));
}

// typed-pointer forms (KH_AS_GLOBAL / KH_AS_LDS: common.h) for the searches
typedef KH_AS_GLOBAL uint32_t gu32_t;
typedef KH_AS_GLOBAL float gf32_t;
__device__ __forceinline__ uint32_t gld_l2(const gu32_t* p) {       // agent-scope load: the word is modified by L2 atomics
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint32_t gflag_or(gu32_t* qs, uint32_t v, uint32_t bit) {
  const int sh = (int)(v & 3u) * 8;
  return (__hip_atomic_fetch_or(qs + (v >> 2), bit << sh, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >> sh) & 0xFFu;
}
__device__ __forceinline__ void gflag_clear(gu32_t* qs, uint32_t v, uint32_t bit) {
  const int sh = (int)(v & 3u) * 8;
  __hip_atomic_fetch_and(qs + (v >> 2), ~(bit << sh), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint32_t uni32(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ uintptr_t uni64(uintptr_t v) { return ((uintptr_t)uni32((uint32_t)(v >> 32)) << 32) | uni32((uint32_t)v); }
typedef KH_AS_GLOBAL uint8_t gu8_t;
__device__ __forceinline__ uint32_t gld8_l2(const gu8_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void gst8_l2(gu8_t* p, uint32_t v) { __hip_atomic_store(p, (uint8_t)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// slot of this lane among the lanes of its wave with p set (all lanes of the wave call this): base from one LDS atomic
__device__ __forceinline__ uint32_t wave_slot(bool p, KH_AS_LDS uint32_t* counter, int lane) {
  const unsigned long long m = __builtin_amdgcn_ballot_w64(p);
  if (m == 0ull) return 0u;
  const int leader = __ffsll((long long)m) - 1;
  uint32_t base = 0u;
  if (lane == leader) base = __hip_atomic_fetch_add(counter, (uint32_t)__popcll(m), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  base = (uint32_t)__builtin_amdgcn_readlane((int)base, leader);
  return base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
}

}  // namespace kh
