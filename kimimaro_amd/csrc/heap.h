// heap.h -- the invalidation heap: the wave-cooperative emulation of libstdc++'s std::priority_queue (Heap<TOPL>, push, pop, the
// LDS key mirror) and the flood that runs on it (invalidate_ball).  Needs search_state.h (INF_BITS, rdlane_u32) and common.h.
#pragma once
#include "search_state.h"

namespace kh {

// ------------------------------------------------------------------------------------------------
// The invalidation heap: an exact emulation of std::priority_queue<HeapDistanceNode, vector, Compare>
// with Compare = `t1.dist >= t2.dist` (dijkstra_invalidation.hpp:233-237, 262-264) as libstdc++
// implements it (bits/stl_heap.h), because the pop order among equal keys decides which source owns
// a voxel.  The array layout after every operation is identical to libstdc++'s:
//   push  = __push_heap: the new key climbs over every ancestor with key >= it.  The ancestors of the
//           new leaf are known up front, so the wave loads them all at once (lane g = generation g),
//           a ballot gives the climb length and the lanes shift the chain down in one step.
//   pop   = __pop_heap/__adjust_heap: libstdc++ walks the hole to a leaf along the smaller child
//           (ties: left) and then pushes the last element up again.  Because keys never decrease
//           from parent to child this lands exactly where the text-book early-exit sift-down lands
//           (verified against the libstdc++ form in oracle/ tests), so the wave descends 6 levels
//           per memory round trip: 126 speculative child nodes are fetched by the 64 lanes, the path
//           is resolved from registers, and the nodes on it are moved up in one parallel step.
// Nodes are 16-byte records {key bits, voxel, source index, -} in the label's slice of HBM scratch, so
// a node is one dwordx4 load or store.  Keys are non-negative floats: they are compared as their bit
// patterns (unsigned), which lets "ties go left" be written as k < sibling + (1 on left lanes).
// LDS mirrors, both ways.  A write-through mirror of WHOLE NODES of heap levels 0-12 was tried twice in the first rounds
// (one volume alone) and measured 10-15 % slower: alone the pop's global trips hit the L2 and the pop is bound by the
// instruction issue of its single wave.  The KEY mirror of levels 7-10 below is a different trade (4 bytes per slot, one
// global trip less per pop).  Measured with twenty volumes in flight (BENCH_NOTES.md, "Heap key mirror"): bit exact, the longest
// chain under load 11 789 -> 11 354 Mcyc (median of the lanes, -3.7 %), the step time 370.1 -> 368.4 ms (medians of three, the
// parent's own spread 13.6 ms): NOT a gain beyond the spread -- the trip it removes is not what doubles the chain under load.
// No new spills in invalidate_ball, +57 instructions.  -DKH_HEAP_MIRROR_LEVELS=0 is the code without it.
// a native LLVM vector (HIP's uint4 is a struct around a union, which ends up in scratch memory here)
typedef uint32_t hnode_t __attribute__((ext_vector_type(4)));
// LDS pointers keep their address space in the type, so LDS and HBM accesses can never be merged into flat_* ones
typedef __attribute__((address_space(3))) hnode_t lds_hnode_t;

// Heap slots 0..TOP-1 live in LDS and nowhere else; slots >= TOP live in the label's slice of HBM scratch.
// TOPL = 1: the root and the first 6-level chunk under it (127 slots, 2 KiB) -- every label affords that.
// TOPL = 2: two chunks (8191 slots, 128 KiB): one such workgroup fits on a CU, so it is reserved for the few
// largest labels, whose sequential chain is the critical path of the whole launch.  Every pop starts in the
// LDS part, so the top read and the first TOPL chunks cost LDS round trips instead of L2 ones.
//
// The key mirror (TOPL = 1 only).  Behind the 130 LDS nodes lie the KEYS of the next KH_HEAP_MIRROR_LEVELS heap levels (default 4:
// levels 7-10, slots 127..2046, 7 680 B).  The nodes of those slots stay in HBM and HBM is the truth; every store to such a slot
// writes its key through (heap_store, the pop's moves).  A pop decides its path through those levels from the keys alone and
// fetches the (at most 4) whole nodes on it together with the 6 levels under them: a heap below 131 072 nodes costs a pop one
// global round trip instead of two.  The mirror is never initialised: a slot is read only below `len`, and it was written when
// it was filled.  The bytes are the workgroup's dynamic LDS, which the sweep and the searches use between the heap's calls.
// 0 compiles the stage out.
#ifndef KH_HEAP_MIRROR_LEVELS
#define KH_HEAP_MIRROR_LEVELS 4
#endif
static_assert(KH_HEAP_MIRROR_LEVELS >= 0 && KH_HEAP_MIRROR_LEVELS <= 5, "the mirror stage resolves at most 62 nodes (one per lane)");
typedef __attribute__((address_space(3))) uint32_t lds_key_t;

template <int TOPL_>
struct Heap {
  static constexpr int TOPL = TOPL_;
  static constexpr uint32_t TOP = TOPL_ == 1 ? 127u : 8191u;
  static constexpr int MIRL = TOPL_ == 1 ? KH_HEAP_MIRROR_LEVELS : 0;     // mirrored levels under the LDS part
  static constexpr uint32_t MIR_END = ((TOP + 1u) << MIRL) - 1u;          // slots TOP .. MIR_END-1 have their key in LDS too
  static constexpr size_t LDS_BYTES = (size_t)(TOP + 3u) * 16u + (size_t)(MIR_END - TOP) * 4u;
  // pop: nested 6-level chunks (the LDS ones included).  32-bit index math needs every hole at level <= 24:
  // without the mirror the holes sit at levels 0, 6, .., 24 (30 levels), with it at 0, 6 | 6+MIRL, .., 18+MIRL (<= 29 levels)
  static constexpr int CHUNKS = MIRL ? 4 : 5;
  static constexpr uint32_t MAX_N = MIRL ? (1u << (6 * CHUNKS + MIRL + 1)) - 1u : 0x7FFFFFFFu;   // the nodes a pop can descend through
  hnode_t* node;   // HBM scratch of this label (L2 resident in practice); slots < TOP unused
  lds_hnode_t* top;  // LDS, TOP + 3 entries (the last LDS chunk's lanes 62/63 read two slots past the end); then the key mirror
  uint32_t cap, n;
  __device__ __forceinline__ lds_key_t* mir() const { return (lds_key_t*)(top + (TOP + 3u)); }   // key of slot i: mir()[i - TOP]
  // per-lane constants of the 126-node speculative sub-tree (children of node m: 2m+2, 2m+3; parent of
  // m >= 2: (m-2)>>1).  Lane l holds node m = l ("slot 0", depths 1..6) and m = l+64 ("slot 1", depth 6).
  unsigned long long am0, am1;  // slot-0 ballot bits of the node's ancestors (am0 including itself)
  uint32_t sh0, j0, j1;         // heap index of my slot-0 node = ((hole+1) << sh0) - 1 + j0, slot 1: << 6, + j1
  uint32_t lf;                  // 1 on even lanes (left children), 0 on odd lanes
};

__device__ __forceinline__ unsigned long long ballot64(bool p) { return __builtin_amdgcn_ballot_w64(p); }
// value of lane l^1 (the sibling node): DPP quad_perm [1,0,3,2], no LDS crossbar round trip
__device__ __forceinline__ uint32_t sibling_u32(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0xB1, 0xF, 0xF, true);
}

template <class H>
__device__ __forceinline__ void heap_init_lane(H& h, int lane) {
  unsigned long long a0 = 0, a1 = 0;
  for (int m = lane; ; m = (m - 2) >> 1) { a0 |= 1ull << m; if (m < 2) break; }
  if (lane + 64 < 126) for (int m = (lane + 62) >> 1; ; m = (m - 2) >> 1) { a1 |= 1ull << m; if (m < 2) break; }
  h.am0 = a0;
  h.am1 = a1;
  const int d0 = 31 - __clz(lane + 2);
  h.sh0 = (uint32_t)d0;
  h.j0 = (uint32_t)(lane + 2 - (1 << d0));
  h.j1 = (uint32_t)(lane + 2);
  h.lf = (lane & 1) ? 0u : 1u;
}

// store of a whole node to slot i, wherever it lives (the mirror's key written through)
template <class H>
__device__ __forceinline__ void heap_store(const H& h, uint32_t i, hnode_t v) {
  if (i < H::TOP) h.top[i] = v;
  else {
    h.node[i] = v;
    if constexpr (H::MIRL > 0) { if (i < H::MIR_END) h.mir()[i - H::TOP] = v.x; }
  }
}

// all 64 lanes of the wave call this with uniform arguments.  One memory round trip: lane g loads
// the whole node of ancestor generation g+1 (from LDS or HBM, whichever holds that slot), a ballot gives
// the climb length m (the ancestors with key >= k form a prefix because keys never decrease from parent
// to child), lanes < m write their ancestor one generation down and lane m drops the new node into
// generation m's slot.
template <class H>
__device__ __forceinline__ bool heap_push_wave(H& h, uint32_t kbits, uint32_t vox, uint32_t src, int lane) {
  if (h.n >= h.cap) return false;
  const uint32_t pos = h.n++;
  const int sh = lane + 1 < 32 ? lane + 1 : 31;
  const uint32_t q = (pos + 1u) >> sh;
  const bool valid = (lane < 31) && q >= 1u;
  const uint32_t ai = q - 1u;
  hnode_t a;
  if (pos < H::TOP) {                     // wave uniform: the whole chain is in LDS
    a = h.top[valid ? ai : 0u];
  } else {
    const bool lo = !valid || ai < H::TOP;
    const hnode_t ag = h.node[lo ? H::TOP : ai];
    const hnode_t al = h.top[lo && valid ? ai : 0u];
    a = lo ? al : ag;
  }
  const unsigned long long climb = ballot64(valid && a.x >= kbits);
  const int m = __ffsll((long long)~climb) - 1;  // length of the leading run of set bits (lane 63 never set)
  const uint32_t dest = ((pos + 1u) >> (lane < 31 ? lane : 31)) - 1u;  // slot of generation `lane` (lane 0: the new leaf)
  const hnode_t fresh = {kbits, vox, src, 0u};
  const hnode_t val = lane < m ? a : fresh;
  if (lane <= m) heap_store(h, dest, val);
  return true;
}

// removes the top; precondition h.n > 0.  libstdc++'s __adjust_heap walks the hole to a leaf along the
// smaller child (ties: left) and then pushes the former last element up again; the result is: the path
// nodes with key < last.key move up one level and `last` takes the slot of the deepest of them.
// The wave fetches 6 levels (126 whole nodes, 2 per lane) per round trip.  A node is on the path iff it
// and all its ancestors in the sub-tree beat their siblings: one sibling compare per lane, one ballot,
// one mask test against the lane's constant ancestor mask.  The chunks nest (chunk c+1 runs inside
// chunk c, which keeps its two nodes in registers) and every write is issued on the way back up, so the
// load of `last` overlaps the whole descent.  Loads are unconditional (index clamped, key masked
// to +inf): no divergent branches in the descent.  Chunk 0 is exactly the LDS part of the heap.
// 32-bit index math is safe: the hole of chunk c sits at level 6c <= 24, so (hole+1) << 6 < 2^31.
// With the key mirror (H::MIRL > 0) the keys-only stage heap_pop_mirror sits between the LDS part and the first global chunk.
template <int C, class H>
__device__ __forceinline__ void heap_pop_mirror(const H& h, uint32_t hole, uint32_t len, uint32_t vk, int lane,
                                                uint32_t& deepest, bool& found);
template <int C, class H>
__device__ __forceinline__ void heap_pop_chunk(const H& h, uint32_t hole, uint32_t len, uint32_t vk, int lane,
                                               uint32_t& deepest, bool& found) {
  const uint32_t i0 = ((hole + 1u) << h.sh0) - 1u + h.j0;
  const uint32_t i1 = ((hole + 1u) << 6) - 1u + h.j1;
  const bool e0 = i0 < len, e1 = (lane < 62) && (i1 < len);
  hnode_t n0, n1;
  if constexpr (C < H::TOPL) { n0 = h.top[i0]; n1 = h.top[i1]; }   // an LDS chunk: i0, i1 < TOP + 3 by construction
  else { n0 = h.node[e0 ? i0 : H::TOP]; n1 = h.node[e1 ? i1 : H::TOP]; }
  const uint32_t k0 = e0 ? n0.x : INF_BITS, k1 = e1 ? n1.x : INF_BITS;
  // a node beats its sibling if it is the left one and left.key <= right.key, or the right one and
  // right.key < left.key (comp(right, left) of dijkstra_invalidation.hpp:233-237: ties go left)
  const bool w0 = e0 & (k0 < sibling_u32(k0) + h.lf);
  const bool w1 = e1 & (k1 < sibling_u32(k1) + h.lf);
  const unsigned long long W0 = ballot64(w0);
  const bool on0 = (W0 & h.am0) == h.am0;
  const bool on1 = w1 && ((W0 & h.am1) == h.am1);
  if constexpr (C + 1 < H::CHUNKS) {
    // next hole = the depth-6 node of the path, if the path got that deep and that node has children
    const unsigned long long P0 = ballot64(on0), P1 = ballot64(on1);
    uint32_t nh = 0;
    if (P1) nh = rdlane_u32(i1, __ffsll((long long)P1) - 1);
    else if (P0 >> 62) nh = rdlane_u32(i0, (P0 >> 63) ? 63 : 62);
    if (nh != 0u && 2u * nh + 1u < len) {
      if constexpr (H::MIRL > 0 && C + 1 == H::TOPL) heap_pop_mirror<C + 1, H>(h, nh, len, vk, lane, deepest, found);
      else heap_pop_chunk<C + 1, H>(h, nh, len, vk, lane, deepest, found);
    }
  }
  // every path node with key < last.key moves to its parent's slot; `last` lands in the slot of the
  // deepest such node (or the root).  Path keys are non-decreasing with depth.
  const bool mv0 = on0 && k0 < vk;
  const bool mv1 = on1 && k1 < vk;
  const uint32_t q0 = (i0 - 1u) >> 1, q1 = (i1 - 1u) >> 1;
  if constexpr (C < H::TOPL) {
    if (mv0) h.top[q0] = n0;
    if (mv1) h.top[q1] = n1;
  } else if constexpr (C == H::TOPL && H::MIRL > 0) {
    // the parent of this chunk's two depth-1 nodes (lanes 0, 1) is the hole: a slot of the deepest mirrored level
    if (mv0) { h.node[q0] = n0; if (lane < 2) h.mir()[hole - H::TOP] = k0; }
    if (mv1) h.node[q1] = n1;
  } else if constexpr (C == H::TOPL) {
    // the parent of this chunk's two depth-1 nodes (lanes 0, 1) is the hole: a leaf of the LDS part
    if (mv0) { if (lane < 2) h.top[hole] = n0; else h.node[q0] = n0; }
    if (mv1) h.node[q1] = n1;
  } else {
    if (mv0) h.node[q0] = n0;
    if (mv1) h.node[q1] = n1;
  }
  if (!found) {
    const unsigned long long M0 = ballot64(mv0), M1 = ballot64(mv1);
    if (M1) { deepest = rdlane_u32(i1, __ffsll((long long)M1) - 1); found = true; }
    else if (M0) { deepest = rdlane_u32(i0, 63 - __clzll((long long)M0)); found = true; }
  }
}

// The keys-only stage under the hole at the last LDS level: the speculative sub-tree of MIRL levels is 2^(MIRL+1) - 2 slots (30),
// lane l holds its node l exactly as in a chunk's slot 0.  The key comes from the mirror; sibling compare, ballot and ancestor
// masks are the chunk's.  Then the lanes on the path fetch their whole node from HBM (the moves need {voxel, source}) -- every
// lane loads, the others the clamp slot -- and the first global chunk starts under the hole at the deepest mirrored level: both
// are in flight together, one round trip.  Writes on the way back up, as in a chunk.
template <int C, class H>
__device__ __forceinline__ void heap_pop_mirror(const H& h, uint32_t hole, uint32_t len, uint32_t vk, int lane,
                                                uint32_t& deepest, bool& found) {
  constexpr int NN = (2 << H::MIRL) - 2;           // nodes of the sub-tree
  constexpr int D0 = (1 << H::MIRL) - 2;           // its first node of the deepest level
  const uint32_t i0 = ((hole + 1u) << h.sh0) - 1u + h.j0;
  const bool e0 = (lane < NN) && (i0 < len);
  const uint32_t km = h.mir()[e0 ? i0 - H::TOP : 0u];
  const uint32_t k0 = e0 ? km : INF_BITS;
  const bool w0 = e0 & (k0 < sibling_u32(k0) + h.lf);
  const unsigned long long W0 = ballot64(w0);
  const bool on0 = (W0 & h.am0) == h.am0;
  const hnode_t n0 = h.node[on0 ? i0 : H::TOP];
  {
    const unsigned long long PD = ballot64(on0) >> D0;
    const uint32_t nh = PD ? rdlane_u32(i0, D0 + __ffsll((long long)PD) - 1) : 0u;
    if (nh != 0u && 2u * nh + 1u < len) heap_pop_chunk<C, H>(h, nh, len, vk, lane, deepest, found);
  }
  const bool mv0 = on0 && k0 < vk;
  const uint32_t q0 = (i0 - 1u) >> 1;
  if (mv0) {
    if (lane < 2) h.top[hole] = n0;      // the hole is a leaf of the LDS part
    else { h.node[q0] = n0; h.mir()[q0 - H::TOP] = k0; }
  }
  if (!found) {
    const unsigned long long M0 = ballot64(mv0);
    if (M0) { deepest = rdlane_u32(i0, 63 - __clzll((long long)M0)); found = true; }
  }
}

template <class H>
__device__ __forceinline__ void heap_pop_wave(H& h, int lane) {
  const uint32_t len = h.n - 1u;
  h.n = len;
  if (len == 0) return;
  const hnode_t last = len < H::TOP ? h.top[len] : h.node[len];  // consumed only after the descent
  uint32_t deepest = 0;
  bool found = false;
  if (len > 1u) heap_pop_chunk<0, H>(h, 0u, len, last.x, lane, deepest, found);
  if (lane == 0) heap_store(h, deepest, last);
}

// wave 0 only.  Returns the number of voxels invalidated.  PROF adds the pop / push / neighbour-test
// cycle split (s_memtime waits on the scalar memory counter, so the production kernel leaves it out).
// Out of line, the heap record by value: the emulation is ONE chain of dependent operations per call and every instruction the
// register allocator adds to its loops (a reloaded pointer, a lane written to a spill register) is on that chain; as a function of
// its own it is allocated for itself (inlined, 47 spilled VGPRs of the kernel cost it 8 %).
template <bool PROF, class H>
__device__ __attribute__((noinline)) uint32_t invalidate_ball(const Geometry& g, const kh_label_t* task, const uint32_t* __restrict__ nbrmask,
                                    const float* __restrict__ dbf, uint8_t* alive, const uint32_t* path, uint32_t npath,
                                    float scale, float constant, H h, uint32_t* status, uint32_t* pushes,
                                    unsigned long long* cyc3, const uint8_t* __restrict__ corner_gate = nullptr) {
  const int lane = threadIdx.x & 63;
  unsigned long long c_pop = 0, c_push = 0, c_fire = 0, tt = 0;
  h.n = 0;
  uint32_t npush = 0;
  bool ovf = false;
  for (uint32_t i = 0; i < npath; i++) {
    if (!heap_push_wave(h, 0u, path[i], i, lane)) ovf = true;
    npush++;
  }
  const uint32_t sx = (uint32_t)g.sx, sxy = (uint32_t)g.sxy;
  const uint32_t xmin = task->xmin, xmax = task->xmax;
  int dx, dy, dz;
  dir_delta(lane < 26 ? lane : 0, dx, dy, dz);
  uint32_t count = 0;
  while (h.n > 0) {
    const hnode_t top = h.top[0];
    const uint32_t vox = top.y, si = top.z;
    const uint8_t live = alive[vox];   // issued before the pop so its latency overlaps the sift-down
    if (PROF) tt = clock64();
    heap_pop_wave(h, lane);
    if (PROF) c_pop += clock64() - tt;
    if (!live) continue;
    if (PROF) tt = clock64();
    if (lane == 0) alive[vox] = 0;
    count++;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    const uint32_t src = path[si];
    float maxd = scale * dbf[src];   // skeletontricks.pyx:393-395, f32 ops
    maxd = maxd + constant;
    const uint32_t z = vox / sxy, r = vox - z * sxy, y = r / sx, x = r - y * sx;
    const uint32_t oz = src / sxy, orr = src - oz * sxy, oy = orr / sx, ox = orr - oy * sx;
    // neighbour enumeration of dijkstra_invalidation.hpp:60-124 seen from the label's bounding box:
    // a corner entry (k >= 18) whose x step leaves the box degenerates into the yz diagonal.
    bool want = false;
    uint32_t q = 0;
    float nd = 0.0f;
    if (lane < 26) {
      int k = lane;
      int ex = dx;
      const bool xout = (dx < 0 && x == xmin) || (dx > 0 && x == xmax);
      if (xout) {
        if (lane >= 18) { ex = 0; k = 10 + (dy > 0 ? 2 : 0) + (dz > 0 ? 1 : 0); }
        else k = -1;
      }
      // with a voxel_connectivity_graph a degenerate corner entry is gated by the corner's bit, not the diagonal's
      const bool open = k < 0 ? false
                      : (xout && lane >= 18 && corner_gate != nullptr) ? ((corner_gate[vox] >> (lane - 18)) & 1u) != 0u
                                                                       : ((nbrmask[vox] >> k) & 1u) != 0u;
      if (open) {
        q = vox + (uint32_t)(ex + (int)sx * dy + (int)sxy * dz);
        if (alive[q]) {
          const int qx = (int)x + ex, qy = (int)y + dy, qz = (int)z + dz;
          const float a = g.wx * (float)(qx - (int)ox);
          const float b = g.wy * (float)(qy - (int)oy);
          const float c = g.wz * (float)(qz - (int)oz);
          float s = a * a;
          const float t = b * b;
          const float u = c * c;
          s = s + t;
          s = s + u;
          nd = sqrtf(s);
          want = nd < maxd;
        }
      }
    }
    unsigned long long m = ballot64(want);
    if (PROF) { c_fire += clock64() - tt; tt = clock64(); }
    const uint32_t ndb = __float_as_uint(nd);
    // The pushes of one fired voxel go to consecutive leaves, in direction order.  About three quarters of them do
    // not climb (measured: 76 % on the largest label of the bench volume): such a push writes its own leaf and
    // nothing else, and whether it climbs depends on its parent only.  So every pending lane looks at the parent
    // of the leaf it would get, the leading run of non-climbing pushes is appended with one store per lane, the
    // first climbing one goes through the ordinary push, and the rest is looked at again (its parents may have
    // changed).  A new leaf is nobody's parent here because the heap is larger than the batch.
    while (m) {
      const uint32_t base = h.n;
      const uint32_t cnt = (uint32_t)__popcll(m);
      if (base < 64u || base + cnt > h.cap) {   // small heap (new leaves could be parents) or no room: one by one
        const int k = __ffsll((long long)m) - 1;
        m &= m - 1;
        if (!heap_push_wave(h, rdlane_u32(ndb, k), rdlane_u32(q, k), si, lane)) ovf = true;
        npush++;
        continue;
      }
      const bool mine = (m >> lane) & 1ull;
      const uint32_t leaf = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
      const uint32_t par = (leaf - 1u) >> 1;
      const bool plo = !mine || par < H::TOP;
      const uint32_t kg = h.node[plo ? H::TOP : par].x;
      const uint32_t kl = h.top[plo && mine ? par : 0u].x;
      const bool stay = mine && (plo ? kl : kg) < ndb;          // __push_heap climbs while parent.key >= key
      const unsigned long long climbers = m & ~ballot64(stay);
      const int c = climbers ? __ffsll((long long)climbers) - 1 : 64;   // first lane whose push climbs
      const unsigned long long run = c < 64 ? (m & ((1ull << c) - 1ull)) : m;
      if ((run >> lane) & 1ull) {
        const hnode_t fresh = {ndb, q, si, 0u};
        heap_store(h, leaf, fresh);
      }
      const uint32_t nrun = (uint32_t)__popcll(run);
      h.n = base + nrun;
      npush += nrun;
      m &= ~run;
      if (c < 64) {
        m &= ~(1ull << c);
        if (!heap_push_wave(h, rdlane_u32(ndb, c), rdlane_u32(q, c), si, lane)) ovf = true;
        npush++;
      }
    }
    if (PROF) c_push += clock64() - tt;
  }
  if (lane == 0) {
    if (ovf) atomicOr(status, KH_ST_HEAP_OVERFLOW);
    *pushes += npush;
    if (PROF) { cyc3[0] += c_pop; cyc3[1] += c_push; cyc3[2] += c_fire; }
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  return count;
}

}  // namespace kh
