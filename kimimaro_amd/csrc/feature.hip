// feature.hip -- skeleton-seeded geodesic Voronoi labels over the WHOLE volume (kimimaro.oversegment, kimimaro/utility.py:562-644;
// dijkstra3d.euclidean_distance_field(..., return_feature_map=True) from many sources), DESIGN.md 3.10.
//
//   kh_geodesic_seed     dist = +inf, feature = none everywhere; then dist = 0 and feature = the smallest vertex number at every seed
//   kh_geodesic_relax    phase 1: d(v) = min over same-label 26-neighbours u of fl(d(u) + w(u, v)), to its fixpoint
//   kh_feature_relax     phase 2, on the FINAL d: f(v) = min f(u) over the achieving neighbours (fl(d(u) + w) == d(v))
//   kh_first_appearance  smallest linear index of every number (the renumbering by first appearance in the raster)
//   kh_remap_u32         feature[v] = map[feature[v]]
//
// A dataset that is relaxed box by box (kimimaro_amd.post.oversegment_chunked) runs the same sweeps on a box at a time:
//   kh_geodesic_seed_at      the seeds alone, on a box whose dist / feature come from the stores
//   kh_box_shell_diff        which core voxels changed, towards which of the 26 neighbouring cores; the largest finite distance
//   kh_first_appearance_box  smallest DATASET raster index (64 bits) of every number, accumulated over the boxes
//
// Both relaxations are PULL sweeps in place: a thread owns a voxel, reads the neighbour words its mask names and stores with a plain
// 32-bit store if its value went down.  Values only ever decrease, so a stale read costs a sweep, never a result: the fixpoint is
// unique and the loop ends when a sweep changed nothing.  Two phases, not one packed (distance, feature) key: see
// DESIGN.md 5.
//
// Activity bricks (KH_BRICK_X x KH_BRICK_Y x KH_BRICK_Z voxels, one workgroup each): sweep s visits a brick only if the brick or one
// of its 26 brick neighbours changed in sweep s - 1.  Invariant: a brick that holds a voxel that could still go down at the end of
// sweep s has a brick in its neighbourhood that changed DURING sweep s (a visited brick recomputed every voxel from values read during
// s; an unvisited one was settled before s by the same argument) -- so nothing is ever missed, across faces, edges or corners.
// Three planes of flags, used round robin: sweep s reads plane s % 3, writes plane (s + 1) % 3 and clears its own byte of plane
// (s + 2) % 3 (the one sweep s + 1 will write).
#include "common.h"

namespace kh {

static constexpr uint32_t KH_NO_FEATURE = 0xFFFFFFFFu;

__global__ __launch_bounds__(256) void geodesic_init_kernel(float* __restrict__ dist, uint32_t* __restrict__ feature, int64_t nvox) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nvox; i += (int64_t)gridDim.x * 256) {
    dist[i] = KH_INF;
    feature[i] = KH_NO_FEATURE;
  }
}

template <typename LT>
__global__ __launch_bounds__(256) void geodesic_seed_kernel(const uint32_t* __restrict__ seed_voxel,
                                                            const uint32_t* __restrict__ seed_number, int64_t nseeds,
                                                            const LT* __restrict__ lab, const uint32_t* __restrict__ seed_label,
                                                            int64_t nvox, float* dist, uint32_t* feature) {
  for (int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x; s < nseeds; s += (int64_t)gridDim.x * 256) {
    const uint32_t v = seed_voxel[s];
    if ((int64_t)v >= nvox) continue;                            // (the host drops these already)
    const uint32_t L = seed_label[s];
    if (L == 0 || (uint32_t)lab[v] != L) continue;               // a vertex off its label seeds nothing
    if (dist) dist[v] = 0.0f;
    if (feature) atomicMin(&feature[v], seed_number[s]);         // several vertices on one voxel: the smallest number
  }
}

// one workgroup = one brick: lanes along x, one wave per z plane of the brick, KH_BRICK_Y rows per thread
template <bool FEATURE>
__global__ __launch_bounds__(256) void relax_kernel(const uint32_t* __restrict__ nbr, const Geometry g, int nbx, int nby, int nbz,
                                                    float* dist, uint32_t* feature, const uint8_t* __restrict__ flags_read,
                                                    uint8_t* flags_write, uint8_t* flags_clear, uint32_t* counters) {
  const int b = (int)blockIdx.x;
  const int bx = b % nbx, by = (b / nbx) % nby, bz = b / (nbx * nby);
  // awake? (the brick itself or one of its 26 neighbours changed in the previous sweep)
  int awake = 0;
  if (threadIdx.x < 27) {
    const int t = (int)threadIdx.x;
    const int qx = bx + t % 3 - 1, qy = by + (t / 3) % 3 - 1, qz = bz + t / 9 - 1;
    if (qx >= 0 && qy >= 0 && qz >= 0 && qx < nbx && qy < nby && qz < nbz) awake = flags_read[qx + nbx * (qy + nby * qz)];
  }
  if (threadIdx.x == 0) flags_clear[b] = 0;
  awake = __syncthreads_or(awake);
  if (!awake) return;

  const int x = bx * KH_BRICK_X + (int)(threadIdx.x & 63);
  const int z = bz * KH_BRICK_Z + (int)(threadIdx.x >> 6);
  int changed = 0;
  if (x < g.sx && z < g.sz) {
    for (int yy = 0; yy < KH_BRICK_Y; yy++) {
      const int y = by * KH_BRICK_Y + yy;
      if (y >= g.sy) break;
      const int64_t i = (int64_t)x + (int64_t)g.sx * y + (int64_t)g.sxy * z;
      const uint32_t m = nbr[i];      // bit k: neighbour k is inside the volume and carries the same non-zero label
      if (m == 0) continue;
      const float dv = dist[i];
      if (!FEATURE) {
        float best = dv;
#pragma unroll
        for (int k = 0; k < 26; k++) {
          if ((m >> k) & 1u) {
            const float c = dist[i + g.off[k]] + g.w[k];    // fl(d(u) + w), no contraction
            best = c < best ? c : best;
          }
        }
        if (best < dv) {
          dist[i] = best;
          changed = 1;
        }
      } else {
        if (!(dv > 0.0f) || dv == KH_INF) continue;         // a seed keeps its number; nothing reaches this voxel
        const uint32_t fv = feature[i];
        uint32_t best = fv;
#pragma unroll
        for (int k = 0; k < 26; k++) {
          if ((m >> k) & 1u) {
            const int64_t u = i + g.off[k];
            const float c = dist[u] + g.w[k];
            if (c == dv) {                                  // an achieving edge: d(u) < d(v)
              const uint32_t fu = feature[u];
              best = fu < best ? fu : best;
            }
          }
        }
        if (best < fv) {
          feature[i] = best;
          changed = 1;
        }
      }
    }
  }
  changed = __syncthreads_or(changed);
  if (threadIdx.x == 0) {
    atomicAdd(&counters[1], 1u);          // bricks visited
    if (changed) {
      flags_write[b] = 1;
      atomicAdd(&counters[0], 1u);        // bricks that changed
    }
  }
}

__global__ __launch_bounds__(256) void first_appearance_kernel(const uint32_t* __restrict__ feature, int64_t nvox, int64_t nnumbers,
                                                               uint32_t* first_of_number) {
  const int lane = threadIdx.x & 63;
  const int64_t nchunks = (nvox + 255) / 256;
  for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const int64_t i = c * 256 + threadIdx.x;
    const uint32_t f = i < nvox ? feature[i] : 0u;
    // lanes hold consecutive voxels: the first lane of a run of equal numbers holds the run's smallest index -- one atomic per run
    const uint32_t prev = __shfl_up(f, 1);
    if ((lane == 0 || f != prev) && f != 0 && (int64_t)f <= nnumbers) atomicMin(&first_of_number[f], (uint32_t)i);
  }
}

// ---- a dataset in boxes.  Both kernels walk the CORE of a box in pieces of 64 voxels of one x row: a wave takes a
// piece, its lanes lie along x.  piece p: row p / pieces_x (y fastest, then z), voxels 64 * (p % pieces_x) ... of that row.
struct BoxCore {
  int32_t bx, by;              // extents of the box (x, y)
  int32_t lo[3], n[3];         // the core inside the box: its low corner and its extents
  int32_t pieces_x;            // (n[0] + 63) / 64
  int64_t pieces;              // pieces_x * n[1] * n[2]
};

// the box-local coordinates of this lane's voxel of piece p; false: the lane lies past the end of the core row
__device__ inline bool core_voxel(const BoxCore& c, int64_t p, int lane, int& x, int& y, int& z) {
  const int64_t row = p / c.pieces_x;
  const int cx = (int)(p % c.pieces_x) * 64 + lane;
  x = c.lo[0] + cx;
  y = c.lo[1] + (int)(row % c.n[1]);
  z = c.lo[2] + (int)(row / c.n[1]);
  return cx < c.n[0];
}

__global__ __launch_bounds__(256) void box_shell_diff_kernel(const uint32_t* __restrict__ old, const uint32_t* __restrict__ now,
                                                             const BoxCore c, uint32_t* out) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), waves = (int64_t)gridDim.x * 4;
  uint32_t dirs = 0, count = 0, top = 0;
  for (int64_t p = wave; p < c.pieces; p += waves) {
    int x, y, z;
    if (!core_voxel(c, p, lane, x, y, z)) continue;
    const int64_t i = (int64_t)x + (int64_t)c.bx * ((int64_t)y + (int64_t)c.by * z);
    const uint32_t b = now[i];
    if (b < 0x7F800000u && b > top) top = b;                 // finite and not negative: the order of the words is the floats'
    if (old[i] == b) continue;
    count++;
    // the outermost layers this voxel lies in (an axis of extent 1: both)
    const int l[3] = {x == c.lo[0], y == c.lo[1], z == c.lo[2]};
    const int h[3] = {x == c.lo[0] + c.n[0] - 1, y == c.lo[1] + c.n[1] - 1, z == c.lo[2] + c.n[2] - 1};
    int k = 0;
#pragma unroll
    for (int dz = -1; dz <= 1; dz++)
#pragma unroll
      for (int dy = -1; dy <= 1; dy++)
#pragma unroll
        for (int dx = -1; dx <= 1; dx++) {
          if (dx == 0 && dy == 0 && dz == 0) continue;
          const int ok = (dx == 0 || (dx < 0 ? l[0] : h[0])) && (dy == 0 || (dy < 0 ? l[1] : h[1])) && (dz == 0 || (dz < 0 ? l[2] : h[2]));
          dirs |= (uint32_t)ok << k;
          k++;
        }
  }
  // the wave's result in lane 0, then one atomic of each kind per wave at most
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) {
    dirs |= __shfl_xor(dirs, s);
    count += __shfl_xor(count, s);
    const uint32_t other = __shfl_xor(top, s);
    top = other > top ? other : top;
  }
  if (lane == 0) {
    if (dirs) atomicOr(&out[0], dirs);
    if (count) atomicAdd(&out[1], count);
    if (top) atomicMax(&out[2], top);
  }
}

__global__ __launch_bounds__(256) void first_appearance_box_kernel(const uint32_t* __restrict__ feature, const BoxCore c, int64_t ox,
                                                                   int64_t oy, int64_t oz, int64_t SX, int64_t SY, int64_t nnumbers,
                                                                   unsigned long long* first_of_number) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), waves = (int64_t)gridDim.x * 4;
  for (int64_t p = wave; p < c.pieces; p += waves) {            // (p is the same in all lanes of a wave: the shuffle is uniform)
    int x, y, z;
    const bool in = core_voxel(c, p, lane, x, y, z);
    const uint32_t f = in ? feature[(int64_t)x + (int64_t)c.bx * ((int64_t)y + (int64_t)c.by * z)] : 0u;
    // first_appearance_kernel's trick: the first lane of a run of equal numbers holds the run's smallest index; a piece never leaves
    // its row, so a run ends where the core row does
    const uint32_t prev = __shfl_up(f, 1);
    if ((lane == 0 || f != prev) && f != 0 && (int64_t)f <= nnumbers)
      atomicMin(&first_of_number[f], (unsigned long long)((ox + x) + SX * ((oy + y) + SY * (oz + z))));
  }
}

__global__ __launch_bounds__(256) void remap_u32_kernel(uint32_t* __restrict__ feature, const uint32_t* __restrict__ map, int64_t nnumbers,
                                                        int64_t nvox) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nvox; i += (int64_t)gridDim.x * 256) {
    const uint32_t f = feature[i];
    feature[i] = (f != 0 && (int64_t)f <= nnumbers) ? map[f] : 0u;
  }
}

static inline unsigned blocks_for(int64_t n) {
  int64_t g = (n + 255) / 256;
  if (g > 8192) g = 8192;
  if (g < 1) g = 1;
  return (unsigned)g;
}

static int relax_impl(bool feature_phase, const uint32_t* nbrmask, int64_t sx, int64_t sy, int64_t sz, float wx, float wy, float wz,
                      float* dist, uint32_t* feature, uint8_t* brick_dirty, uint32_t* changed, int sweeps, int64_t first_sweep,
                      hipStream_t st) {
  if (sx <= 0 || sy <= 0 || sz <= 0 || sx * sy * sz >= (int64_t)1 << 32) {
    set_error("geodesic relax: the volume must hold between 1 and 2^32 - 1 voxels");
    return KH_EINVAL;
  }
  if (sweeps < 1 || first_sweep < 0) {
    set_error("geodesic relax: sweeps >= 1 and first_sweep >= 0");
    return KH_EINVAL;
  }
  Geometry g;
  make_geometry(g, sx, sy, sz, wx, wy, wz);
  const int nbx = (int)((sx + KH_BRICK_X - 1) / KH_BRICK_X), nby = (int)((sy + KH_BRICK_Y - 1) / KH_BRICK_Y),
            nbz = (int)((sz + KH_BRICK_Z - 1) / KH_BRICK_Z);
  const int64_t nbricks = (int64_t)nbx * nby * nbz;
  KH_HIP_CHECK(hipMemsetAsync(changed, 0, sizeof(uint32_t) * 2 * (size_t)sweeps, st));
  for (int j = 0; j < sweeps; j++) {
    const int64_t s = first_sweep + j;
    const uint8_t* fr = brick_dirty + (s % 3) * nbricks;
    uint8_t* fw = brick_dirty + ((s + 1) % 3) * nbricks;
    uint8_t* fc = brick_dirty + ((s + 2) % 3) * nbricks;
    if (feature_phase)
      hipLaunchKernelGGL((relax_kernel<true>), dim3((unsigned)nbricks), dim3(256), 0, st, nbrmask, g, nbx, nby, nbz, dist, feature, fr,
                         fw, fc, changed + 2 * j);
    else
      hipLaunchKernelGGL((relax_kernel<false>), dim3((unsigned)nbricks), dim3(256), 0, st, nbrmask, g, nbx, nby, nbz, dist, feature, fr,
                         fw, fc, changed + 2 * j);
    KH_LAUNCH_CHECK();
  }
  return KH_OK;
}

// dist / feature: either may be null (kh_geodesic_seed_at)
static int launch_seeds(const uint32_t* seed_voxel, const uint32_t* seed_number, int64_t nseeds, const void* labels, int label_bytes,
                        const uint32_t* seed_label, int64_t nvox, float* dist, uint32_t* feature, hipStream_t st) {
  if (nseeds == 0) return KH_OK;
  switch (label_bytes) {
    case 1:
      hipLaunchKernelGGL((geodesic_seed_kernel<uint8_t>), dim3(blocks_for(nseeds)), dim3(256), 0, st, seed_voxel, seed_number, nseeds,
                         (const uint8_t*)labels, seed_label, nvox, dist, feature);
      break;
    case 2:
      hipLaunchKernelGGL((geodesic_seed_kernel<uint16_t>), dim3(blocks_for(nseeds)), dim3(256), 0, st, seed_voxel, seed_number, nseeds,
                         (const uint16_t*)labels, seed_label, nvox, dist, feature);
      break;
    case 4:
      hipLaunchKernelGGL((geodesic_seed_kernel<uint32_t>), dim3(blocks_for(nseeds)), dim3(256), 0, st, seed_voxel, seed_number, nseeds,
                         (const uint32_t*)labels, seed_label, nvox, dist, feature);
      break;
    default:
      set_error("label_bytes must be 1, 2 or 4");
      return KH_EINVAL;
  }
  KH_LAUNCH_CHECK();
  return KH_OK;
}

// the core [core_lo, core_hi) of a box of bx x by x bz voxels as the kernels take it; false: not inside the box, or the box too large
static bool make_box_core(BoxCore& c, int64_t bx, int64_t by, int64_t bz, const int64_t* core_lo, const int64_t* core_hi) {
  const int64_t b[3] = {bx, by, bz};
  if (bx <= 0 || by <= 0 || bz <= 0 || bx * by * bz >= (int64_t)1 << 32 || !core_lo || !core_hi) return false;
  for (int a = 0; a < 3; a++) {
    if (core_lo[a] < 0 || core_lo[a] >= core_hi[a] || core_hi[a] > b[a]) return false;
    c.lo[a] = (int32_t)core_lo[a];
    c.n[a] = (int32_t)(core_hi[a] - core_lo[a]);
  }
  c.bx = (int32_t)bx;
  c.by = (int32_t)by;
  c.pieces_x = (c.n[0] + 63) / 64;
  c.pieces = (int64_t)c.pieces_x * c.n[1] * c.n[2];
  return true;
}

static inline unsigned blocks_for_pieces(int64_t pieces) { return blocks_for(pieces * 64); }      // four waves, four pieces per block

}  // namespace kh

using namespace kh;

extern "C" int kh_geodesic_seed(const uint32_t* seed_voxel, const uint32_t* seed_number, int64_t nseeds, const void* labels,
                                int label_bytes, const uint32_t* seed_label, int64_t nvox, float* dist, uint32_t* feature,
                                void* stream) {
  if (int rc = require_device()) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (nvox <= 0 || nvox >= (int64_t)1 << 32 || nseeds < 0) {
    set_error("kh_geodesic_seed: 0 < nvox < 2^32 and nseeds >= 0");
    return KH_EINVAL;
  }
  hipLaunchKernelGGL(geodesic_init_kernel, dim3(blocks_for(nvox)), dim3(256), 0, st, dist, feature, nvox);
  KH_LAUNCH_CHECK();
  return launch_seeds(seed_voxel, seed_number, nseeds, labels, label_bytes, seed_label, nvox, dist, feature, st);
}

extern "C" int kh_geodesic_seed_at(const uint32_t* seed_voxel, const uint32_t* seed_number, int64_t nseeds, const void* labels,
                                   int label_bytes, const uint32_t* seed_label, int64_t nvox, float* dist, uint32_t* feature,
                                   void* stream) {
  if (int rc = require_device()) return rc;
  if (nvox <= 0 || nvox >= (int64_t)1 << 32 || nseeds < 0) {
    set_error("kh_geodesic_seed_at: 0 < nvox < 2^32 and nseeds >= 0");
    return KH_EINVAL;
  }
  return launch_seeds(seed_voxel, seed_number, nseeds, labels, label_bytes, seed_label, nvox, dist, feature, (hipStream_t)stream);
}

extern "C" int kh_box_shell_diff(const uint32_t* old, const uint32_t* now, int64_t bx, int64_t by, int64_t bz, const int64_t* core_lo,
                                 const int64_t* core_hi, uint32_t* out, void* stream) {
  if (int rc = require_device()) return rc;
  hipStream_t st = (hipStream_t)stream;
  BoxCore c;
  if (!make_box_core(c, bx, by, bz, core_lo, core_hi)) {
    set_error("kh_box_shell_diff: a box of 1 .. 2^32 - 1 voxels and 0 <= core_lo < core_hi <= its extents");
    return KH_EINVAL;
  }
  KH_HIP_CHECK(hipMemsetAsync(out, 0, sizeof(uint32_t) * 3, st));
  hipLaunchKernelGGL(box_shell_diff_kernel, dim3(blocks_for_pieces(c.pieces)), dim3(256), 0, st, old, now, c, out);
  KH_LAUNCH_CHECK();
  return KH_OK;
}

extern "C" int kh_first_appearance_box(const uint32_t* feature, int64_t bx, int64_t by, int64_t bz, const int64_t* core_lo,
                                       const int64_t* core_hi, const int64_t* origin, int64_t SX, int64_t SY, int64_t nnumbers,
                                       uint64_t* first_of_number, void* stream) {
  if (int rc = require_device()) return rc;
  BoxCore c;
  if (!make_box_core(c, bx, by, bz, core_lo, core_hi) || !origin || origin[0] < 0 || origin[1] < 0 || origin[2] < 0 ||
      origin[0] + bx > SX || origin[1] + by > SY || nnumbers < 0 || nnumbers >= 0xFFFFFFFFll) {
    set_error("kh_first_appearance_box: a box of 1 .. 2^32 - 1 voxels inside the dataset's SX x SY rows, 0 <= core_lo < core_hi <= its "
              "extents and 0 <= nnumbers < 2^32 - 1");
    return KH_EINVAL;
  }
  hipLaunchKernelGGL(first_appearance_box_kernel, dim3(blocks_for_pieces(c.pieces)), dim3(256), 0, (hipStream_t)stream, feature, c,
                     origin[0], origin[1], origin[2], SX, SY, nnumbers, (unsigned long long*)first_of_number);
  KH_LAUNCH_CHECK();
  return KH_OK;
}

extern "C" int kh_geodesic_relax(const uint32_t* nbrmask, int64_t sx, int64_t sy, int64_t sz, float wx, float wy, float wz, float* dist,
                                 uint8_t* brick_dirty, uint32_t* changed, int sweeps, int64_t first_sweep, void* stream) {
  if (int rc = require_device()) return rc;
  return relax_impl(false, nbrmask, sx, sy, sz, wx, wy, wz, dist, nullptr, brick_dirty, changed, sweeps, first_sweep,
                    (hipStream_t)stream);
}

extern "C" int kh_feature_relax(const uint32_t* nbrmask, int64_t sx, int64_t sy, int64_t sz, float wx, float wy, float wz,
                                const float* dist, uint32_t* feature, uint8_t* brick_dirty, uint32_t* changed, int sweeps,
                                int64_t first_sweep, void* stream) {
  if (int rc = require_device()) return rc;
  return relax_impl(true, nbrmask, sx, sy, sz, wx, wy, wz, const_cast<float*>(dist), feature, brick_dirty, changed, sweeps, first_sweep,
                    (hipStream_t)stream);
}

extern "C" int kh_first_appearance(const uint32_t* feature, int64_t nvox, int64_t nnumbers, uint32_t* first_of_number, void* stream) {
  if (int rc = require_device()) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (nvox <= 0 || nvox >= (int64_t)1 << 32 || nnumbers < 0 || nnumbers >= 0xFFFFFFFFll) {
    set_error("kh_first_appearance: 0 < nvox < 2^32 and 0 <= nnumbers < 2^32 - 1");
    return KH_EINVAL;
  }
  KH_HIP_CHECK(hipMemsetAsync(first_of_number, 0xFF, sizeof(uint32_t) * (size_t)(nnumbers + 1), st));
  hipLaunchKernelGGL(first_appearance_kernel, dim3(blocks_for(nvox)), dim3(256), 0, st, feature, nvox, nnumbers, first_of_number);
  KH_LAUNCH_CHECK();
  return KH_OK;
}

extern "C" int kh_remap_u32(uint32_t* feature, const uint32_t* map, int64_t nnumbers, int64_t nvox, void* stream) {
  if (int rc = require_device()) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (nvox <= 0 || nnumbers < 0) {
    set_error("kh_remap_u32: nvox > 0 and nnumbers >= 0");
    return KH_EINVAL;
  }
  hipLaunchKernelGGL(remap_u32_kernel, dim3(blocks_for(nvox)), dim3(256), 0, st, feature, map, nnumbers, nvox);
  KH_LAUNCH_CHECK();
  return KH_OK;
}
