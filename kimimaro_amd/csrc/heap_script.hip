// heap_script.hip -- kh_heap_script: the invalidation heap of heap.h (Heap<TOPL>, push, pop, the key mirror) driven by a script
// of operations, one wave, nothing else of the flood around it.  For tests: the product never calls it.  The batched append
// of invalidate_ball is part of the flood's loop and not a function of its own, so no script op reaches it.
// A translation unit of its own, so that nothing here can change the code of the kernels of trace.hip.
#include "common.h"
#include "search_state.h"
#include "heap.h"

namespace kh {

// Record encoding and output formats: include/kimi_hip.h (kh_heap_script).
static constexpr uint32_t HS_PUSH = 0u, HS_POP = 1u, HS_DUMP = 2u;

template <int TOPL>
__global__ __launch_bounds__(64) void heap_script_kernel(const uint32_t* __restrict__ ops, uint32_t nops, hnode_t* nodes,
                                                         uint32_t capacity, uint32_t* pops, unsigned long long pops_cap,
                                                         uint32_t* dumps, unsigned long long dumps_cap, uint32_t* state) {
  typedef Heap<TOPL> H;
  extern __shared__ __attribute__((aligned(16))) unsigned char heap_top[];
  const int lane = threadIdx.x & 63;
  H h;
  h.node = nodes;
  h.top = (lds_hnode_t*)heap_top;
  h.cap = capacity < H::MAX_N ? capacity : H::MAX_N;
  h.n = 0;
  heap_init_lane(h, lane);
  uint32_t refused = 0, errors = 0, unfit = 0;
  unsigned long long ppos = 0, dpos = 0;      // words written to pops / dumps
  for (uint32_t i = 0; i < nops; i++) {
    const uint32_t op = ops[4ull * i], a = ops[4ull * i + 1], b = ops[4ull * i + 2], c = ops[4ull * i + 3];
    if (op == HS_PUSH) {
      if (!heap_push_wave(h, a, b, c, lane)) refused++;
    } else if (op == HS_POP) {
      if (h.n == 0u) { errors++; continue; }
      if (ppos + 4ull <= pops_cap) {
        const hnode_t top = h.top[0];
        if (lane == 0) { pops[ppos] = top.x; pops[ppos + 1] = top.y; pops[ppos + 2] = top.z; pops[ppos + 3] = h.n; }
        ppos += 4ull;
      } else unfit++;
      heap_pop_wave(h, lane);
    } else if (op == HS_DUMP) {
      const uint32_t n = h.n;
      const uint32_t mend = n < H::MIR_END ? n : H::MIR_END;
      const uint32_t nmir = (H::MIRL > 0 && mend > H::TOP) ? mend - H::TOP : 0u;
      const unsigned long long need = (a & 1u) ? 2ull : 2ull + 4ull * n + nmir;
      if (dpos + need > dumps_cap) { unfit++; continue; }
      if (lane == 0) { dumps[dpos] = n; dumps[dpos + 1] = i; }
      if (!(a & 1u)) {
        uint32_t* out = dumps + dpos + 2ull;
        for (uint32_t s = (uint32_t)lane; s < n; s += 64u) {
          const hnode_t v = s < H::TOP ? h.top[s] : h.node[s];
          out[4ull * s] = v.x; out[4ull * s + 1] = v.y; out[4ull * s + 2] = v.z; out[4ull * s + 3] = v.w;
        }
        if constexpr (H::MIRL > 0) {
          uint32_t* mout = out + 4ull * n;
          for (uint32_t s = (uint32_t)lane; s < nmir; s += 64u) mout[s] = h.mir()[s];
        }
      }
      dpos += need;
    } else {
      errors++;
    }
  }
  if (lane == 0) { state[0] = h.n; state[1] = refused; state[2] = errors; state[3] = unfit; }
}

template <int TOPL>
static int launch_heap_script(const uint32_t* ops, int64_t nops, void* nodes, uint32_t capacity, uint32_t* pops, int64_t pops_capacity,
                              uint32_t* dumps, int64_t dumps_capacity, uint32_t* state, hipStream_t st) {
  // The attribute belongs to the function and not to the launch: always the same value (trace.hip, trace_lds_bytes).
  const void* kernel = reinterpret_cast<const void*>(&heap_script_kernel<TOPL>);
  KH_HIP_CHECK(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)Heap<2>::LDS_BYTES));
  hipLaunchKernelGGL((heap_script_kernel<TOPL>), dim3(1), dim3(64), Heap<TOPL>::LDS_BYTES, st, ops, (uint32_t)nops, (hnode_t*)nodes,
                     capacity, pops, (unsigned long long)pops_capacity, dumps, (unsigned long long)dumps_capacity, state);
  KH_LAUNCH_CHECK();
  return KH_OK;
}
}  // namespace kh

extern "C" int kh_heap_script(int topl, const uint32_t* ops, int64_t nops, void* nodes, int64_t nodes_allocated, uint32_t capacity,
                              uint32_t* pops, int64_t pops_capacity, uint32_t* dumps, int64_t dumps_capacity, uint32_t* state,
                              void* stream) {
  using namespace kh;
  if (int rc = require_device()) return rc;
  if (topl != 1 && topl != 2) { set_error("kh_heap_script: topl must be 1 or 2"); return KH_EINVAL; }
  const int64_t top = topl == 1 ? (int64_t)Heap<1>::TOP : (int64_t)Heap<2>::TOP;
  const int64_t need = (int64_t)capacity > top + 1 ? (int64_t)capacity : top + 1;
  if (!nodes || ((uintptr_t)nodes & 15) != 0 || nodes_allocated < need || nops < 0 || nops >= (1ll << 30) || (nops > 0 && !ops) ||
      pops_capacity < 0 || dumps_capacity < 0 || (pops_capacity > 0 && !pops) || (dumps_capacity > 0 && !dumps) || !state) {
    set_error("kh_heap_script: bad arguments (nodes 16-byte aligned with max(capacity, TOP + 1) allocated, capacities >= 0)");
    return KH_EINVAL;
  }
  if (topl == 1) return launch_heap_script<1>(ops, nops, nodes, capacity, pops, pops_capacity, dumps, dumps_capacity, state, (hipStream_t)stream);
  return launch_heap_script<2>(ops, nops, nodes, capacity, pops, pops_capacity, dumps, dumps_capacity, state, (hipStream_t)stream);
}
