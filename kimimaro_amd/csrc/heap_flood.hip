// heap_flood.hip -- kh_heap_flood: ONE call of the invalidation flood of heap.h (invalidate_ball<PROF, Heap<TOPL>>) by one wave, in
// each of its four forms, nothing else of the path loop around it: no sweep, no ghosts, no pool.  For tests: the product never calls
// it.  What kh_heap_script cannot reach -- the batched leaf append, whose parent key comes from LDS or from memory -- runs here on
// Heap<2> as well, which otherwise exists only inside trace_paths_kernel<false, 2>, and in the profiled build.
// A translation unit of its own, so that nothing here can change the code of the kernels of trace.hip.
#include "common.h"
#include "search_state.h"
#include "heap.h"

namespace kh {

// Arguments and output formats: include/kimi_hip.h (kh_heap_flood).
template <bool PROF, int TOPL>
__global__ __launch_bounds__(64) void heap_flood_kernel(Geometry g, const uint32_t* __restrict__ nbrmask,
                                                        const uint8_t* __restrict__ corner_gate, const float* __restrict__ dbf,
                                                        uint8_t* alive, const uint32_t* path, uint32_t npath, float scale, float constant,
                                                        uint32_t xmin, uint32_t xmax, hnode_t* nodes, uint32_t capacity, uint32_t* state,
                                                        unsigned long long* cyc3) {
  typedef Heap<TOPL> H;
  extern __shared__ __attribute__((aligned(16))) unsigned char heap_top[];
  // as the path kernel holds them: geometry, label record and the call's counters in LDS
  __shared__ Geometry geo;
  __shared__ kh_label_t task;
  __shared__ uint32_t status, pushes;
  __shared__ unsigned long long cyc[3];
  const int lane = threadIdx.x & 63;
  if (lane == 0) {
    geo = g;
    task.xmin = xmin; task.xmax = xmax;
    status = 0u; pushes = 0u;
    cyc[0] = cyc[1] = cyc[2] = 0ull;
  }
  __syncthreads();
  H h;
  h.node = nodes;
  h.top = (lds_hnode_t*)heap_top;
  h.cap = capacity < H::MAX_N ? capacity : H::MAX_N;
  h.n = 0;
  heap_init_lane(h, lane);
  const uint32_t count = invalidate_ball<PROF, H>(geo, &task, nbrmask, dbf, alive, path, npath, scale, constant, h, &status, &pushes, cyc,
                                                  corner_gate);
  __syncthreads();
  if (lane == 0) {
    state[0] = count; state[1] = pushes; state[2] = status;
    cyc3[0] = cyc[0]; cyc3[1] = cyc[1]; cyc3[2] = cyc[2];
  }
}

struct FloodArgs {
  Geometry g; const uint32_t* nbrmask; const uint8_t* corner_gate; const float* dbf; uint8_t* alive; const uint32_t* path;
  uint32_t npath; float scale, constant; uint32_t xmin, xmax; hnode_t* nodes; uint32_t capacity; uint32_t* state;
  unsigned long long* cyc3; hipStream_t st;
};
template <bool PROF, int TOPL>
static int launch_heap_flood(const FloodArgs& a) {
  // The attribute belongs to the function and not to the launch: always the same value (trace.hip, trace_lds_bytes).
  const void* kernel = reinterpret_cast<const void*>(&heap_flood_kernel<PROF, TOPL>);
  KH_HIP_CHECK(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)Heap<2>::LDS_BYTES));
  hipLaunchKernelGGL((heap_flood_kernel<PROF, TOPL>), dim3(1), dim3(64), Heap<TOPL>::LDS_BYTES, a.st, a.g, a.nbrmask, a.corner_gate, a.dbf,
                     a.alive, a.path, a.npath, a.scale, a.constant, a.xmin, a.xmax, a.nodes, a.capacity, a.state, a.cyc3);
  KH_LAUNCH_CHECK();
  return KH_OK;
}
}  // namespace kh

extern "C" int kh_heap_flood(int topl, int profile, int64_t sx, int64_t sy, int64_t sz, float wx, float wy, float wz,
                             const uint32_t* nbrmask, const uint8_t* corner_gate, const float* dbf, uint8_t* alive,
                             const uint32_t* path, int64_t npath, float scale, float constant, uint32_t xmin, uint32_t xmax,
                             void* nodes, int64_t nodes_allocated, uint32_t capacity, uint32_t* state, uint64_t* cyc3, void* stream) {
  using namespace kh;
  if (int rc = require_device()) return rc;
  if (topl != 1 && topl != 2) { set_error("kh_heap_flood: topl must be 1 or 2"); return KH_EINVAL; }
  if (profile != 0 && profile != 1) { set_error("kh_heap_flood: profile must be 0 or 1"); return KH_EINVAL; }
  const int64_t top = topl == 1 ? (int64_t)Heap<1>::TOP : (int64_t)Heap<2>::TOP;
  const int64_t need = (int64_t)capacity > top + 1 ? (int64_t)capacity : top + 1;
  if (!nodes || ((uintptr_t)nodes & 15) != 0 || nodes_allocated < need) {
    set_error("kh_heap_flood: bad arguments (nodes 16-byte aligned with max(capacity, TOP + 1) allocated)");
    return KH_EINVAL;
  }
  if (sx <= 0 || sy <= 0 || sz <= 0 || sx >= (1ll << 31) || sy >= (1ll << 31) || sz >= (1ll << 31) || sx * sy >= (1ll << 31) ||
      sx * sy * sz >= (1ll << 32) || !nbrmask || !dbf || !alive || npath < 0 || npath >= (1ll << 32) || (npath > 0 && !path) ||
      xmin > xmax || (int64_t)xmax >= sx || !state || !cyc3) {
    set_error("kh_heap_flood: bad arguments (a volume below 2^32 voxels, 0 <= xmin <= xmax < sx, 0 <= npath < 2^32, no NULL array)");
    return KH_EINVAL;
  }
  FloodArgs a;
  make_geometry(a.g, sx, sy, sz, wx, wy, wz);
  a.nbrmask = nbrmask; a.corner_gate = corner_gate; a.dbf = dbf; a.alive = alive; a.path = path; a.npath = (uint32_t)npath;
  a.scale = scale; a.constant = constant; a.xmin = xmin; a.xmax = xmax; a.nodes = (hnode_t*)nodes; a.capacity = capacity;
  a.state = state; a.cyc3 = reinterpret_cast<unsigned long long*>(cyc3); a.st = (hipStream_t)stream;
  if (topl == 1) return profile ? launch_heap_flood<true, 1>(a) : launch_heap_flood<false, 1>(a);
  return profile ? launch_heap_flood<true, 2>(a) : launch_heap_flood<false, 2>(a);
}
