// rows27.h -- the 27 words around a voxel of a whole-volume u32 / f32 array, loaded as nine rows of three consecutive words.
// Used by the searches (sssp.h) and by the sweep (sweep.h, sweep_rows).  Needs common.h only.
#pragma once
#include "common.h"

namespace kh {

// The 27 words around voxel u of a whole-volume u32 / f32 array as nine rows of three consecutive words:
// w[(dx + 1) + 3 * ((dy + 1) + 3 * (dz + 1))] = a[u + dx + sx * dy + sxy * dz].  A row outside the volume reads u's own row (its
// neighbours are in nobody's mask); a row that starts one word before the array or ends one behind it is read one word further in
// and shifted (the missing word belongs to a neighbour outside the volume).  nvox >= 3.
typedef uint32_t u32x3_t __attribute__((ext_vector_type(3)));
typedef u32x3_t u32x3_a4_t __attribute__((aligned(4)));
__device__ __forceinline__ void rows27_base(uint32_t nvox, int sx, int sxy, int sy, int sz, uint32_t u, int y, int z, uint32_t (&bc)[9],
                                            int (&sh)[9]) {
#pragma unroll
  for (int r = 0; r < 9; r++) {
    const int dy = r % 3 - 1, dz = r / 3 - 1;
    const bool in = (unsigned)(y + dy) < (unsigned)sy && (unsigned)(z + dz) < (unsigned)sz;
    const long long base = (long long)u + (in ? dy * sx + dz * sxy : 0) - 1;
    const long long hi = nvox >= 3u ? (long long)nvox - 3 : 0;       // (arrays of fewer than three words carry padding: include/kimi_hip.h)
    const long long c = base < 0 ? 0 : (base > hi ? hi : base);
    bc[r] = (uint32_t)c;
    sh[r] = (int)(base - c);
  }
}
__device__ __forceinline__ void rows27_shift(const u32x3_t (&t)[9], const int (&sh)[9], uint32_t (&w)[27]) {
#pragma unroll
  for (int r = 0; r < 9; r++) {
    w[3 * r + 0] = sh[r] > 0 ? t[r].y : t[r].x;                       // (sh < 0: the word in front of the array -- never used)
    w[3 * r + 1] = sh[r] > 0 ? t[r].z : (sh[r] < 0 ? t[r].x : t[r].y);
    w[3 * r + 2] = sh[r] < 0 ? t[r].y : t[r].z;                       // (sh > 0: the word behind the array -- never used)
  }
}
// words that memory-side atomics change: past the vector cache (sc1).  The nine loads and their wait are ONE asm statement, so the
// compiler never sees a register that is still in flight; the wait also covers the loads it has issued itself just before.
__device__ __forceinline__ void rows27_sc1(const KH_AS_GLOBAL uint32_t* a, uint32_t nvox, int sx, int sxy, int sy, int sz, uint32_t u,
                                           int y, int z, uint32_t (&w)[27]) {
  uint32_t bc[9];
  int sh[9];
  rows27_base(nvox, sx, sxy, sy, sz, u, y, z, bc, sh);
  u32x3_t t[9];
  asm volatile(
      "global_load_dwordx3 %0, %9, off sc1\n\t"
      "global_load_dwordx3 %1, %10, off sc1\n\t"
      "global_load_dwordx3 %2, %11, off sc1\n\t"
      "global_load_dwordx3 %3, %12, off sc1\n\t"
      "global_load_dwordx3 %4, %13, off sc1\n\t"
      "global_load_dwordx3 %5, %14, off sc1\n\t"
      "global_load_dwordx3 %6, %15, off sc1\n\t"
      "global_load_dwordx3 %7, %16, off sc1\n\t"
      "global_load_dwordx3 %8, %17, off sc1\n\t"
      "s_waitcnt vmcnt(0)"
      : "=&v"(t[0]), "=&v"(t[1]), "=&v"(t[2]), "=&v"(t[3]), "=&v"(t[4]), "=&v"(t[5]), "=&v"(t[6]), "=&v"(t[7]), "=&v"(t[8])
      : "v"(a + bc[0]), "v"(a + bc[1]), "v"(a + bc[2]), "v"(a + bc[3]), "v"(a + bc[4]), "v"(a + bc[5]), "v"(a + bc[6]), "v"(a + bc[7]),
        "v"(a + bc[8])
      : "memory");
  rows27_shift(t, sh, w);
}
// words only plain stores of this workgroup change (the weight field: rails are zeroed between the searches)
__device__ __forceinline__ void rows27_plain(const KH_AS_GLOBAL float* a, uint32_t nvox, int sx, int sxy, int sy, int sz, uint32_t u, int y,
                                             int z, float (&w)[27]) {
  uint32_t bc[9];
  int sh[9];
  rows27_base(nvox, sx, sxy, sy, sz, u, y, z, bc, sh);
  u32x3_t t[9];
#pragma unroll
  for (int r = 0; r < 9; r++) t[r] = *(const KH_AS_GLOBAL u32x3_a4_t*)((const KH_AS_GLOBAL uint32_t*)a + bc[r]);
  uint32_t wu[27];
  rows27_shift(t, sh, wu);
#pragma unroll
  for (int i = 0; i < 27; i++) w[i] = __uint_as_float(wu[i]);
}

}  // namespace kh
