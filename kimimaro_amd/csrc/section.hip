// section.hip -- kimimaro.cross_sectional_area's inner call (xs3d.cross_sectional_area, kimimaro/utility.py:315-320, 494-499) for a
// whole batch of (seed voxel, normal, label) items in one launch (gfx950; DESIGN.md 3.12, PARITY UNPINNED).
//
// An item is a small planar flood through the label volume: the 26-connected component, among the voxels that the plane through the
// seed's centre cuts and that carry the item's label, that holds the seed.  Items are independent, there are hundreds of thousands
// of them, and their sizes are skewed (a soma's sections have thousands of voxels, a neurite's tens): ONE WAVE PER ITEM, items
// pulled from a global counter, no synchronisation between waves.
//
//   queue     every voxel the flood reaches, in arrival order; the first XS_LDS_QUEUE entries in LDS, the rest in the wave's spill
//             region of the scratch.  The wave walks it 64 entries at a time (a lane per voxel) and walks it once more to clear
//             the visited set -- no memset per item.
//   visited   four bits per COLUMN along the dominant axis w of the plane (the axis with the largest |n_w| a_w): along w the cut
//             voxels of a column are one run, and 2h / (|n_w| a_w) <= 3 bounds it by four voxels (three in exact arithmetic, one
//             for a rounding at each end), so bit (c_w & 3) of the column's nibble names a voxel.  The bitmap has one nibble per
//             column of the largest face of the volume, never a bit per voxel.  atomicOr's return value says which lane was first.
//   area      per voxel in closed form (below), float64, rounded to a 64-bit fixed point whose quantum the host chooses from the
//             largest possible sum: integer sums do not depend on the order in which the flood arrives.
//
// Membership is the statement of DESIGN.md 3.12, operation by operation (this library is built with -ffp-contract=off).
//
// The FILLED instantiation (kh_cross_sections_filled) cuts filled(L) = L u hole(L) instead of L: "carries the item's label" becomes
// "carries it, or lies in one of the regions (kh_regions6) that the item's sorted list names".  Only that test differs; an item
// with an empty list reads no region at all.
//
// The BOX instantiation (kh_cross_sections_box) is handed the box [o, o + b) of a dataset of extents d instead of a whole volume.
// The flood and the hot loop are the same statements: `touch` collects the faces of the ARRAY the flood reaches, as ever.  A face of
// the box either is a face of the dataset (o == 0, o + b == d) or a cut through it, a property of the launch and not of the voxel, so
// the epilogue splits the one accumulator by a mask: contact = touch & dataset_faces, clip = touch & ~dataset_faces.  The fixed
// point's quantum comes from the caller (the dataset's, kh_cross_sections_fixed_exponent), so that a section no cut clips sums to
// the same integer in every box and in the whole dataset.
//
// FILLED && BOX (kh_cross_sections_filled_box) is both at once and adds no statement: the region ids are those of
// the DATASET's region graph (the box of the region store), the lists name the dataset's hole regions that have voxels in the box.
#include <math.h>

#include "common.h"

namespace kh {

constexpr int XS_LDS_QUEUE = 2048;        // queue entries per wave in LDS: 8 KiB per wave, 32 KiB per block of four waves
constexpr int XS_WAVES_PER_BLOCK = 4;
constexpr int64_t XS_HEADER_BYTES = 256;  // scratch: [0] the item counter, [1] the overflow flag
// What a launch leaves in the scratch, and that every wave count gives the same bytes: DESIGN.md 3.12 "The scratch after a launch".

// d of DESIGN.md 3.12: ((nx ax) dx + (ny ay) dy) + (nz az) dz, left to right; h likewise
__host__ __device__ inline double xs_offset(double nax, double nay, double naz, int dx, int dy, int dz) {
  return (nax * (double)dx + nay * (double)dy) + naz * (double)dz;
}

__host__ __device__ inline double xs_half_width(double nx, double ny, double nz, double ax, double ay, double az) {
  return 0.5 * ((fabs(nx) * ax + fabs(ny) * ay) + fabs(nz) * az);
}

// the axis with the largest |n_i| a_i (the lowest among equals)
__host__ __device__ inline int xs_dominant(double nx, double ny, double nz, double ax, double ay, double az) {
  const double px = fabs(nx) * ax, py = fabs(ny) * ay, pz = fabs(nz) * az;
  int w = 0;
  double best = px;
  if (py > best) { w = 1; best = py; }
  if (pz > best) w = 2;
  return w;
}

// area of { (u, v) in [0, W] x [0, H] : alpha u + beta v <= s }, alpha, beta >= 0, A = alpha W <= B = beta H: nothing, a
// triangle, a trapezoid, the rectangle less a triangle, the rectangle -- no difference of nearly equal terms in any case
__host__ __device__ inline double xs_clipped_rect(double s, double alpha, double beta, double W, double H, double A, double B) {
  if (!(s > 0.0)) return 0.0;
  if (s >= A + B) return W * H;
  if (s <= A) return 0.5 * ((s / alpha) * (s / beta));
  if (s <= B) return W * ((s - 0.5 * A) / beta);
  const double r = (A + B) - s;
  return W * H - 0.5 * ((r / alpha) * (r / beta));
}

// Area of plane /\ voxel box: the box has edges (ax, ay, az), the plane the normal direction (nx, ny, nz) (any length > 0) and
// passes at n . x = -d from the box's centre, d in the units of xs_offset.  Projected along the dominant axis w the polygon is the
// part of the (u, v) face between two parallel lines, i.e. a difference of two clipped rectangles; the polygon is that over |n_w|.
__host__ __device__ inline double xs_voxel_area(double nx, double ny, double nz, double ax, double ay, double az, double d) {
  const double len = sqrt((nx * nx + ny * ny) + nz * nz);
  const double mx = fabs(nx) / len, my = fabs(ny) / len, mz = fabs(nz) / len;
  const int w = xs_dominant(nx, ny, nz, ax, ay, az);
  // (u, v): the two other axes, (y, z) / (x, z) / (x, y)
  double alpha = w == 0 ? my : mx, W = w == 0 ? ay : ax, beta = w == 2 ? my : mz, H = w == 2 ? ay : az;
  const double mw = w == 0 ? mx : (w == 1 ? my : mz), aw = w == 0 ? ax : (w == 1 ? ay : az);
  double A = alpha * W, B = beta * H;
  if (A > B) {
    double t;
    t = alpha; alpha = beta; beta = t;
    t = W; W = H; H = t;
    t = A; A = B; B = t;
  }
  const double C = mw * aw;
  const double mid = 0.5 * (A + B) - fabs(d) / len;
  const double P = xs_clipped_rect(mid + 0.5 * C, alpha, beta, W, H, A, B) - xs_clipped_rect(mid - 0.5 * C, alpha, beta, W, H, A, B);
  const double area = P / mw;
  return area > 0.0 ? area : 0.0;
}

struct XsArgs {
  int sx, sy, sz;
  double ax, ay, az;
  int64_t n_items;
  const uint32_t* seed;
  const uint32_t* want;
  const double* normals;
  float* area;
  uint8_t* contact;
  uint32_t* voxels;
  unsigned long long* header;    // [0] next item, [1] overflow flag
  uint32_t* bitmap;              // [n_waves][bitmap_words]
  uint32_t* spill;               // [n_waves][spill_cap]
  int64_t bitmap_words, spill_cap;
  int n_waves;
  double fixed_scale, fixed_inverse;   // 2^k and 2^-k of the fixed point
};

// the holes of the items' labels (FILLED): item i's regions are list[begin[i] .. begin[i] + count[i]), ascending
struct XsHoles {
  const uint32_t* region;        // [nvox]: kh_regions6
  const uint32_t* begin;
  const uint32_t* count;
  const uint32_t* list;
};

// is r among list[0 .. n) (ascending)?
__device__ inline bool xs_listed(const uint32_t* __restrict__ list, uint32_t n, uint32_t r) {
  uint32_t lo = 0, hi = n;       // the first entry >= r lies in [lo, hi]
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (list[mid] < r) lo = mid + 1;
    else hi = mid;
  }
  return lo < n && list[lo] == r;
}

// the box of a dataset (BOX): which faces of the label array are faces of the dataset (the bits of `contact`), and where the others go
struct XsBox {
  uint32_t dataset_faces;
  uint8_t* clip;
};

template <typename LT, bool FILLED, bool BOX>
__global__ __launch_bounds__(64 * XS_WAVES_PER_BLOCK) void cross_sections_kernel(const LT* __restrict__ lab, XsArgs p, XsHoles hs,
                                                                                 XsBox bx) {
  __shared__ uint32_t lds_queue[XS_WAVES_PER_BLOCK][XS_LDS_QUEUE];
  const int lane = (int)(threadIdx.x & 63);
  const int wave_in_block = (int)(threadIdx.x >> 6);
  const int wave = (int)blockIdx.x * XS_WAVES_PER_BLOCK + wave_in_block;
  if (wave >= p.n_waves) return;
  uint32_t* const lq = lds_queue[wave_in_block];
  uint32_t* const bitmap = p.bitmap + (int64_t)wave * p.bitmap_words;
  uint32_t* const spill = p.spill + (int64_t)wave * p.spill_cap;
  const int64_t cap = (int64_t)XS_LDS_QUEUE + p.spill_cap;
  const int64_t nvox = (int64_t)p.sx * p.sy * p.sz;

  for (;;) {
    unsigned long long item = 0;
    if (lane == 0) item = atomicAdd(&p.header[0], 1ull);
    item = __shfl(item, 0);
    if (item >= (unsigned long long)p.n_items) return;

    const uint32_t seed = p.seed[item];
    const uint32_t want = p.want[item];
    const double nx = p.normals[3 * item + 0], ny = p.normals[3 * item + 1], nz = p.normals[3 * item + 2];
    const double h = xs_half_width(nx, ny, nz, p.ax, p.ay, p.az);
    bool valid = (int64_t)seed < nvox && isfinite(nx) && isfinite(ny) && isfinite(nz) && h > 0.0 && isfinite(h);
    // (FILLED) the item's holes: n_holes == 0 is wave uniform and keeps every region load away
    const uint32_t* holes = nullptr;
    uint32_t n_holes = 0, hole_min = 0, hole_max = 0;
    if (FILLED) {
      n_holes = hs.count[item];
      if (n_holes) {
        holes = hs.list + hs.begin[item];
        hole_min = holes[0];
        hole_max = holes[n_holes - 1];
      }
    }
    auto in_hole = [&](uint32_t r) -> bool { return r >= hole_min && r <= hole_max && xs_listed(holes, n_holes, r); };
    if (valid) {
      valid = (uint32_t)lab[seed] == want;
      if (FILLED && !valid && n_holes) valid = in_hole(hs.region[seed]);
    }
    if (!valid) {       // (wave uniform)
      if (lane == 0) {
        p.area[item] = 0.0f;
        p.contact[item] = 0;
        p.voxels[item] = 0;
        if (BOX) bx.clip[item] = 0;
      }
      continue;
    }
    const int px = (int)(seed % (uint32_t)p.sx), py = (int)((seed / (uint32_t)p.sx) % (uint32_t)p.sy),
              pz = (int)(seed / ((uint32_t)p.sx * (uint32_t)p.sy));
    const double nax = nx * p.ax, nay = ny * p.ay, naz = nz * p.az;
    const int w = xs_dominant(nx, ny, nz, p.ax, p.ay, p.az);
    const int U = w == 0 ? p.sy : p.sx;      // columns are numbered over the two other axes, (y, z) / (x, z) / (x, y)

    // the visited bit of voxel (x, y, z): word and mask
    auto visit_bit = [&](int x, int y, int z, int64_t& word) -> uint32_t {
      const int cu = w == 0 ? y : x, cv = w == 2 ? y : z, cw = w == 0 ? x : (w == 1 ? y : z);
      const int64_t col = (int64_t)cu + (int64_t)U * cv;
      word = col >> 3;
      return 1u << (((int)(col & 7) << 2) + (cw & 3));
    };
    auto queue_get = [&](int64_t i) -> uint32_t { return i < XS_LDS_QUEUE ? lq[i] : spill[i - XS_LDS_QUEUE]; };
    auto queue_put = [&](int64_t i, uint32_t v) {
      if (i < XS_LDS_QUEUE) lq[i] = v;
      else if (i < cap) spill[i - XS_LDS_QUEUE] = v;
    };

    if (lane == 0) {
      int64_t word;
      const uint32_t bit = visit_bit(px, py, pz, word);
      atomicOr(&bitmap[word], bit);
      lq[0] = seed;
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    int64_t qn = 1, head = 0;
    long long fixed = 0;
    uint32_t count = 0, touch = 0;

    while (head < qn) {
      const int64_t m = qn - head < 64 ? qn - head : 64;
      uint32_t fresh = 0;          // bit k: neighbour k is new to the section (k = (dx+1) + 3 (dy+1) + 9 (dz+1))
      int x = 0, y = 0, z = 0;
      if (lane < m) {
        const uint32_t self = queue_get(head + lane);
        x = (int)(self % (uint32_t)p.sx);
        y = (int)((self / (uint32_t)p.sx) % (uint32_t)p.sy);
        z = (int)(self / ((uint32_t)p.sx * (uint32_t)p.sy));
        const double d = xs_offset(nax, nay, naz, x - px, y - py, z - pz);
        fixed += __double2ll_rn(xs_voxel_area(nx, ny, nz, p.ax, p.ay, p.az, d) * p.fixed_scale);
        count++;
        touch |= (x == 0 ? 1u : 0u) | (x == p.sx - 1 ? 2u : 0u) | (y == 0 ? 4u : 0u) | (y == p.sy - 1 ? 8u : 0u) |
                 (z == 0 ? 16u : 0u) | (z == p.sz - 1 ? 32u : 0u);
        // every neighbour's label in flight at once: a neighbour that is outside or not cut reads the voxel itself instead
        uint32_t same = 0, other = 0;      // other (FILLED): cut neighbours that carry another label
#pragma unroll
        for (int k = 0; k < 27; k++) {
          if (k == 13) continue;
          const int dx = k % 3 - 1, dy = (k / 3) % 3 - 1, dz = k / 9 - 1;
          const int qx = x + dx, qy = y + dy, qz = z + dz;
          const bool inside = qx >= 0 && qx < p.sx && qy >= 0 && qy < p.sy && qz >= 0 && qz < p.sz;
          const double dq = xs_offset(nax, nay, naz, qx - px, qy - py, qz - pz);
          const bool ok = inside && fabs(dq) < h;
          const int64_t at = ok ? (int64_t)qx + (int64_t)p.sx * ((int64_t)qy + (int64_t)p.sy * qz) : (int64_t)self;
          const uint32_t l = (uint32_t)lab[at];
          same |= (ok && l == want) ? 1u << k : 0u;
          if (FILLED) other |= (ok && l != want) ? 1u << k : 0u;
        }
        if (FILLED && n_holes) {
          // their regions, all loads in flight at once as the labels above (a neighbour that is not asked reads nothing), then
          // the searches
          uint32_t rid[27];
#pragma unroll
          for (int k = 0; k < 27; k++) {
            if (k == 13) continue;
            const int64_t at = (int64_t)(x + k % 3 - 1) + (int64_t)p.sx * ((int64_t)(y + (k / 3) % 3 - 1) + (int64_t)p.sy * (z + k / 9 - 1));
            rid[k] = (other >> k & 1u) ? hs.region[at] : 0u;
          }
#pragma unroll
          for (int k = 0; k < 27; k++) {
            if (k == 13) continue;
            if ((other >> k & 1u) && in_hole(rid[k])) same |= 1u << k;
          }
        }
        while (same) {
          const int k = __ffs((int)same) - 1;
          same &= same - 1;
          int64_t word;
          const uint32_t bit = visit_bit(x + k % 3 - 1, y + (k / 3) % 3 - 1, z + k / 9 - 1, word);
          if (!(atomicOr(&bitmap[word], bit) & bit)) fresh |= 1u << k;
        }
      }
      // append: an exclusive scan of the lanes' counts
      const int mine = __popc(fresh);
      int scan = mine;
#pragma unroll
      for (int s = 1; s < 64; s <<= 1) {
        const int o = __shfl_up(scan, s);
        if (lane >= s) scan += o;
      }
      const int total = __shfl(scan, 63);
      int64_t at = qn + (scan - mine);
      while (fresh) {
        const int k = __ffs((int)fresh) - 1;
        fresh &= fresh - 1;
        queue_put(at++, (uint32_t)((int64_t)(x + k % 3 - 1) + (int64_t)p.sx * ((int64_t)(y + (k / 3) % 3 - 1) + (int64_t)p.sy * (z + k / 9 - 1))));
      }
      qn += total;
      head += m;
      if (qn > cap) {          // cannot happen (the host sizes the spill for the largest section); never write past it
        if (lane == 0) p.header[1] = 1ull;
        qn = cap;
      }
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    }

    // clear the visited bits along the queue (all bits of a word belong to this item)
    for (int64_t i = lane; i < qn; i += 64) {
      const uint32_t v = queue_get(i);
      int64_t word;
      visit_bit((int)(v % (uint32_t)p.sx), (int)((v / (uint32_t)p.sx) % (uint32_t)p.sy), (int)(v / ((uint32_t)p.sx * (uint32_t)p.sy)), word);
      atomicAnd(&bitmap[word], 0u);
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
      fixed += __shfl_xor(fixed, s);
      count += __shfl_xor(count, s);
      touch |= __shfl_xor(touch, s);
    }
    if (lane == 0) {
      p.area[item] = (float)((double)fixed * p.fixed_inverse);
      p.contact[item] = (uint8_t)(BOX ? touch & bx.dataset_faces : touch);
      if (BOX) bx.clip[item] = (uint8_t)(touch & ~bx.dataset_faces);
      p.voxels[item] = count;
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");
  }
}

// what a launch needs per wave and in all
struct XsLayout {
  int64_t bitmap_words, spill_cap, wave_bytes, queue_cap;
};

static bool xs_layout(int64_t sx, int64_t sy, int64_t sz, XsLayout& L) {
  if (sx <= 0 || sy <= 0 || sz <= 0 || sx >= (1ll << 31) || sy >= (1ll << 31) || sz >= (1ll << 31)) return false;
  const double nv = (double)sx * (double)sy * (double)sz;
  if (nv >= 4294967295.0) return false;
  const int64_t nvox = sx * sy * sz;
  int64_t face = sx * sy;
  if (sx * sz > face) face = sx * sz;
  if (sy * sz > face) face = sy * sz;
  L.bitmap_words = (face + 7) / 8 + 1;
  L.queue_cap = 4 * face < nvox ? 4 * face : nvox;       // at most four cut voxels per column, at most the volume
  L.spill_cap = L.queue_cap > XS_LDS_QUEUE ? L.queue_cap - XS_LDS_QUEUE : 0;
  L.wave_bytes = 4 * (L.bitmap_words + L.spill_cap);
  return true;
}

// e with (the largest possible sum of a section of a volume of these extents) < 2^e: a voxel's polygon is no larger than the three
// faces of its box together, a section has at most min(4 x the largest face, the volume) voxels.  Extents up to 2^31 each: the face
// is exact in 64 bits, the products beyond that are float64.  False for extents or an anisotropy the launches refuse, and for a
// bound that float64 does not hold (e is frexp's then, as it always was).
static bool xs_fixed_exponent(int64_t sx, int64_t sy, int64_t sz, double ax, double ay, double az, int& e) {
  if (sx <= 0 || sy <= 0 || sz <= 0 || sx >= (1ll << 31) || sy >= (1ll << 31) || sz >= (1ll << 31)) return false;
  if (!(ax > 0 && ay > 0 && az > 0) || !isfinite(ax) || !isfinite(ay) || !isfinite(az)) return false;
  int64_t face = sx * sy;
  if (sx * sz > face) face = sx * sz;
  if (sy * sz > face) face = sy * sz;
  const double most = 4.0 * (double)face, nv = ((double)sx * (double)sy) * (double)sz;
  const double sum = ((ax * ay + ay * az) + ax * az) * (most < nv ? most : nv);
  e = 0;
  frexp(sum, &e);       // sum < 2^e
  return isfinite(sum) && sum > 0.0;
}

}  // namespace kh

using namespace kh;

extern "C" int kh_cross_sections_fixed_exponent(int64_t dx, int64_t dy, int64_t dz, double ax, double ay, double az) {
  int e = 0;
  return xs_fixed_exponent(dx, dy, dz, ax, ay, az, e) ? e : INT32_MIN;
}

extern "C" int64_t kh_cross_sections_scratch_bytes(int64_t sx, int64_t sy, int64_t sz, int64_t n_waves) {
  XsLayout L;
  if (!xs_layout(sx, sy, sz, L) || n_waves < 1) return -1;
  return XS_HEADER_BYTES + n_waves * L.wave_bytes;
}

// all entry points: hs == nullptr && bx == nullptr launches the plain instantiation, both given the filled box one; `name` heads the
// error messages;
// fixed_exponent is read with bx alone
static int xs_launch(const char* name, const void* labels, int label_bytes, int64_t sx, int64_t sy, int64_t sz, double ax, double ay,
                     double az, int64_t n_items, const uint32_t* seed_lin, const uint32_t* want_label, const double* normals,
                     const XsHoles* hs, const XsBox* bx, int fixed_exponent, float* area, uint8_t* contact, uint32_t* voxels,
                     void* scratch, int64_t scratch_bytes, void* stream) {
  if (int rc = require_device()) return rc;
  XsLayout L;
  if (!xs_layout(sx, sy, sz, L)) {
    set_error("%s: extents in [1, 2^31), fewer than 2^32 - 1 voxels", name);
    return KH_EINVAL;
  }
  if (!(ax > 0 && ay > 0 && az > 0) || !isfinite(ax) || !isfinite(ay) || !isfinite(az)) {
    set_error("%s: the anisotropy must be three finite positive numbers", name);
    return KH_EINVAL;
  }
  if (n_items < 0 || n_items >= (1ll << 32)) {
    set_error("%s: 0 <= n_items < 2^32", name);
    return KH_EINVAL;
  }
  if (n_items == 0) return KH_OK;
  if (hs && (!hs->region || !hs->begin || !hs->count || !hs->list)) {
    set_error("%s: region, hole_begin, hole_count and hole_regions must not be null", name);
    return KH_EINVAL;
  }
  if (label_bytes != 1 && label_bytes != 2 && label_bytes != 4) {       // before the memset below: a refused call writes nothing
    set_error("%s: label_bytes must be 1, 2 or 4", name);
    return KH_EINVAL;
  }
  int64_t waves = (scratch_bytes - XS_HEADER_BYTES) / L.wave_bytes;
  if (scratch_bytes < XS_HEADER_BYTES || waves < 1 || ((uintptr_t)scratch & 7)) {
    set_error("%s: the scratch holds no wave (kh_cross_sections_scratch_bytes) or is not 8-byte aligned", name);
    return KH_EINVAL;
  }
  if (waves > n_items) waves = n_items;
  if (waves > 16384) waves = 16384;
  hipStream_t st = (hipStream_t)stream;
  XsArgs p;
  p.sx = (int)sx; p.sy = (int)sy; p.sz = (int)sz;
  p.ax = ax; p.ay = ay; p.az = az;
  p.n_items = n_items;
  p.seed = seed_lin; p.want = want_label; p.normals = normals;
  p.area = area; p.contact = contact; p.voxels = voxels;
  p.header = (unsigned long long*)scratch;
  p.bitmap = (uint32_t*)((char*)scratch + XS_HEADER_BYTES);
  p.spill = p.bitmap + waves * L.bitmap_words;
  p.bitmap_words = L.bitmap_words;
  p.spill_cap = L.spill_cap;
  p.n_waves = (int)waves;
  // fixed point: a voxel's polygon is no larger than the three faces together, a section has at most queue_cap voxels; the sum
  // stays below 2^62 quanta.  The quantum is then below 2^-30 of one voxel's area even for 2^32 voxels -- far below half a
  // float32 ulp of any sum.
  int e = 0;
  xs_fixed_exponent(sx, sy, sz, ax, ay, az, e);
  if (bx) {
    // the caller's quantum: never finer than this array's own (the sums stay below 2^62), and 2^(62 - e) stays a normal double
    if (fixed_exponent < e || fixed_exponent > 1023) {
      set_error("%s: fixed_exponent %d, at least this box's own (%d: kh_cross_sections_fixed_exponent of the dataset)", name,
                fixed_exponent, e);
      return KH_EINVAL;
    }
    e = fixed_exponent;
  }
  p.fixed_scale = ldexp(1.0, 62 - e);
  p.fixed_inverse = ldexp(1.0, e - 62);
  KH_HIP_CHECK(hipMemsetAsync(scratch, 0, (size_t)(XS_HEADER_BYTES + waves * L.bitmap_words * 4), st));
  const unsigned grid = (unsigned)((waves + XS_WAVES_PER_BLOCK - 1) / XS_WAVES_PER_BLOCK);
  const dim3 block(64 * XS_WAVES_PER_BLOCK);
  const XsHoles none = {nullptr, nullptr, nullptr, nullptr};
  const XsBox whole = {63u, nullptr};
#define KH_XS_LAUNCH(LT)                                                                                                              \
  do {                                                                                                                                \
    if (hs && bx) hipLaunchKernelGGL((cross_sections_kernel<LT, true, true>), dim3(grid), block, 0, st, (const LT*)labels, p, *hs,    \
                                     *bx);                                                                                            \
    else if (hs) hipLaunchKernelGGL((cross_sections_kernel<LT, true, false>), dim3(grid), block, 0, st, (const LT*)labels, p, *hs,    \
                                    whole);                                                                                           \
    else if (bx) hipLaunchKernelGGL((cross_sections_kernel<LT, false, true>), dim3(grid), block, 0, st, (const LT*)labels, p, none,    \
                                    *bx);                                                                                             \
    else hipLaunchKernelGGL((cross_sections_kernel<LT, false, false>), dim3(grid), block, 0, st, (const LT*)labels, p, none, whole);   \
  } while (0)
  switch (label_bytes) {
    case 1: KH_XS_LAUNCH(uint8_t); break;
    case 2: KH_XS_LAUNCH(uint16_t); break;
    case 4: KH_XS_LAUNCH(uint32_t); break;
    default: break;       // (refused above)
  }
#undef KH_XS_LAUNCH
  KH_LAUNCH_CHECK();
  return KH_OK;
}

extern "C" int kh_cross_sections(const void* labels, int label_bytes, int64_t sx, int64_t sy, int64_t sz, double ax, double ay,
                                 double az, int64_t n_items, const uint32_t* seed_lin, const uint32_t* want_label,
                                 const double* normals, float* area, uint8_t* contact, uint32_t* voxels, void* scratch,
                                 int64_t scratch_bytes, void* stream) {
  return xs_launch("kh_cross_sections", labels, label_bytes, sx, sy, sz, ax, ay, az, n_items, seed_lin, want_label, normals, nullptr,
                   nullptr, 0, area, contact, voxels, scratch, scratch_bytes, stream);
}

extern "C" int kh_cross_sections_filled(const void* labels, int label_bytes, int64_t sx, int64_t sy, int64_t sz, double ax, double ay,
                                        double az, int64_t n_items, const uint32_t* seed_lin, const uint32_t* want_label,
                                        const double* normals, const uint32_t* region, const uint32_t* hole_begin,
                                        const uint32_t* hole_count, const uint32_t* hole_regions, float* area, uint8_t* contact,
                                        uint32_t* voxels, void* scratch, int64_t scratch_bytes, void* stream) {
  const XsHoles hs = {region, hole_begin, hole_count, hole_regions};
  return xs_launch("kh_cross_sections_filled", labels, label_bytes, sx, sy, sz, ax, ay, az, n_items, seed_lin, want_label, normals, &hs,
                   nullptr, 0, area, contact, voxels, scratch, scratch_bytes, stream);
}

// the two box entries: hs == nullptr is kh_cross_sections_box
static int xs_launch_box(const char* name, const void* labels, int label_bytes, int64_t sx, int64_t sy, int64_t sz, double ax, double ay,
                         double az, int64_t n_items, const uint32_t* seed_lin, const uint32_t* want_label, const double* normals,
                         const XsHoles* hs, int64_t ox, int64_t oy, int64_t oz, int64_t dx, int64_t dy, int64_t dz, int fixed_exponent,
                         float* area, uint8_t* contact, uint32_t* voxels, uint8_t* clip, void* scratch, int64_t scratch_bytes,
                         void* stream) {
  if (ox < 0 || oy < 0 || oz < 0 || sx <= 0 || sy <= 0 || sz <= 0 || dx <= 0 || dy <= 0 || dz <= 0 || ox > dx - sx || oy > dy - sy ||
      oz > dz - sz) {
    set_error("%s: the box [o, o + b) must lie inside the dataset [0, d)", name);
    return KH_EINVAL;
  }
  if (!clip && n_items > 0) {
    set_error("%s: clip must not be null", name);
    return KH_EINVAL;
  }
  XsBox bx;
  bx.dataset_faces = (ox == 0 ? 1u : 0u) | (ox + sx == dx ? 2u : 0u) | (oy == 0 ? 4u : 0u) | (oy + sy == dy ? 8u : 0u) |
                     (oz == 0 ? 16u : 0u) | (oz + sz == dz ? 32u : 0u);
  bx.clip = clip;
  return xs_launch(name, labels, label_bytes, sx, sy, sz, ax, ay, az, n_items, seed_lin, want_label, normals, hs, &bx,
                   fixed_exponent, area, contact, voxels, scratch, scratch_bytes, stream);
}

extern "C" int kh_cross_sections_box(const void* labels, int label_bytes, int64_t sx, int64_t sy, int64_t sz, double ax, double ay,
                                     double az, int64_t n_items, const uint32_t* seed_lin, const uint32_t* want_label,
                                     const double* normals, int64_t ox, int64_t oy, int64_t oz, int64_t dx, int64_t dy, int64_t dz,
                                     int fixed_exponent, float* area, uint8_t* contact, uint32_t* voxels, uint8_t* clip, void* scratch,
                                     int64_t scratch_bytes, void* stream) {
  return xs_launch_box("kh_cross_sections_box", labels, label_bytes, sx, sy, sz, ax, ay, az, n_items, seed_lin, want_label, normals,
                       nullptr, ox, oy, oz, dx, dy, dz, fixed_exponent, area, contact, voxels, clip, scratch, scratch_bytes, stream);
}

extern "C" int kh_cross_sections_filled_box(const void* labels, int label_bytes, int64_t sx, int64_t sy, int64_t sz, double ax,
                                            double ay, double az, int64_t n_items, const uint32_t* seed_lin, const uint32_t* want_label,
                                            const double* normals, const uint32_t* region, const uint32_t* hole_begin,
                                            const uint32_t* hole_count, const uint32_t* hole_regions, int64_t ox, int64_t oy,
                                            int64_t oz, int64_t dx, int64_t dy, int64_t dz, int fixed_exponent, float* area,
                                            uint8_t* contact, uint32_t* voxels, uint8_t* clip, void* scratch, int64_t scratch_bytes,
                                            void* stream) {
  const XsHoles hs = {region, hole_begin, hole_count, hole_regions};
  return xs_launch_box("kh_cross_sections_filled_box", labels, label_bytes, sx, sy, sz, ax, ay, az, n_items, seed_lin, want_label,
                       normals, &hs, ox, oy, oz, dx, dy, dz, fixed_exponent, area, contact, voxels, clip, scratch, scratch_bytes, stream);
}

// host: the membership test and the per-voxel area of one voxel at offset (dx, dy, dz) from the seed -- the same inline functions
// the kernel runs, for the tests that compare them with the CPU statement without a GPU.  Returns 1 when the voxel is cut.
extern "C" int kh_host_section_voxel(const double* normal, const double* anisotropy, int64_t dx, int64_t dy, int64_t dz,
                                     double* offset, double* half_width, double* area) {
  const double nx = normal[0], ny = normal[1], nz = normal[2], ax = anisotropy[0], ay = anisotropy[1], az = anisotropy[2];
  const double d = xs_offset(nx * ax, ny * ay, nz * az, (int)dx, (int)dy, (int)dz);
  const double h = xs_half_width(nx, ny, nz, ax, ay, az);
  *offset = d;
  *half_width = h;
  *area = xs_voxel_area(nx, ny, nz, ax, ay, az, d);
  return fabs(d) < h ? 1 : 0;
}
