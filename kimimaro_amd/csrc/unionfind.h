// unionfind.h -- the lock-free union-find of kh_part_clusters (join.hip) and kh_forest_components (forest.hip): the parent array IS the
// output.  parent[x] <= x always: a root is hooked under a smaller root only, by one integer CAS that succeeds only while it still is a
// root, so the trees never form a cycle and, once every pair has been united, the root of a tree is the smallest member of its set --
// whatever order the unions arrived in.  A parent word only ever moves to another ancestor of its node, so a reader that sees an older
// value still walks to the root.  32-bit integer atomics only; no floating-point value goes through them.
#pragma once
#include "common.h"

namespace kh {

__device__ __forceinline__ uint32_t uf_load(const uint32_t* parent, uint32_t x) {
  return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ uint32_t uf_find(uint32_t* parent, uint32_t x) {      // with path halving
  for (;;) {
    const uint32_t p = uf_load(parent, x);
    if (p == x) return x;
    const uint32_t gp = uf_load(parent, p);
    if (gp != p) __hip_atomic_store(parent + x, gp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    x = gp;
  }
}

__device__ __forceinline__ void uf_unite(uint32_t* parent, uint32_t a, uint32_t b) {
  for (;;) {
    a = uf_find(parent, a);
    b = uf_find(parent, b);
    if (a == b) return;
    if (a < b) {
      const uint32_t s = a;
      a = b;
      b = s;
    }
    if (atomicCAS(parent + a, a, b) == a) return;      // the larger root under the smaller; it was hooked meanwhile: walk on from both
  }
}

}  // namespace kh
