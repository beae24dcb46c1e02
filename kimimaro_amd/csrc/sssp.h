// sssp.h -- the label-correcting search of one label by its workgroup (sssp<MODE>) with its LDS layout, and the distance-field
// search built on it (edf_label).  Needs search_state.h (Ctl, Queues, the L2 helpers) and rows27.h (the 27-word row loads).
#pragma once
#include "rows27.h"
#include "search_state.h"

namespace kh {

// LDS scratch of a search (north_star: "frontier relaxation with LDS bucket queues and wave-ballot compaction"): KH_SSSP_LDS_BYTES
// per thread of the workgroup, laid out as
//   key[H], val[H]   the COMBINE TABLE of a batch of frontier voxels: open addressing on the voxel index, val = the smallest
//                    fl(d[u] + w) any frontier voxel of the batch offers the voxel (LDS atomic min).  A batch relaxes into the
//                    table, a barrier, then every occupied slot is flushed by ONE thread: it is the only writer of dist[v], of
//                    v's membership byte and of v's list entries, so the searches issue NO global atomic (every global atomic
//                    on gfx950 is a fabric round trip that drops its line from the L2: DESIGN.md r6-1).
//   qa[NQ], qb[NQ]   the heads of the two near work lists (bucket "below T" being processed / being built); entries from NQ on
//                    overflow to the label's lists in HBM at the same index.  The far bucket stays in HBM (it is split by a
//                    streaming pass).
// List slots are handed out per wave: a ballot of the lanes that append, ONE LDS atomic add by the first of them, a prefix
// population count for the others.
#define KH_SSSP_LDS_BYTES 48u   /* per thread: H = 4 slots of 8 bytes, NQ = 2 + 2 entries of 4 bytes */
static constexpr uint32_t SSSP_EMPTY = 0xFFFFFFFFu;
__device__ __forceinline__ bool sssp_offer(KH_AS_LDS uint32_t* key, KH_AS_LDS uint32_t* val, uint32_t hmask, int hshift, uint32_t v,
                                           uint32_t nb) {
  uint32_t s = (v * 0x9E3779B1u) >> hshift;
#pragma unroll 1
  for (int t = 0; t < 12; t++) {
    uint32_t seen = SSSP_EMPTY;
    __hip_atomic_compare_exchange_strong(key + s, &seen, v, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (seen == SSSP_EMPTY || seen == v) {
      __hip_atomic_fetch_min(val + s, nb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      return true;
    }
    s = (s + 1u) & hmask;
  }
  return false;       // the neighbourhood of the slot is full: the frontier voxel is relaxed again after the flush
}

// MODE 0: EDF (edge length by direction).  MODE 1: railroad (cost = pdrf of the entered voxel, rails
// absorb, stops once everything at or below the nearest rail is final).  MODE 2: parental field
// (trace.py:155, fix_branching=False): field costs, no rails, runs to completion.
// On return distances below the final threshold are exact (ctl->best_rail set for MODE 1).
// lds / lds_bytes: the workgroup's search scratch, >= KH_SSSP_LDS_BYTES * blockDim.x bytes, 4-byte aligned.
template <int MODE>
__device__ __attribute__((noinline)) void sssp(const Geometry& g_, const uint32_t* __restrict__ nbrmask_, const float* __restrict__ wfield_,
                     float* dist_, uint8_t* qstate_, uint32_t source, Queues q, Ctl* ctl_, float delta_floor,
                     unsigned char* lds_, uint32_t lds_bytes, uint32_t preseeded_far = 0) {
  constexpr bool RAIL = MODE == 1;
  constexpr bool FIELD = MODE != 0;  // MODE 2: dijkstra3d.parental_field -- field weights, no rails, runs to completion
  const int tid = threadIdx.x;
  const int nthr = blockDim.x, nwav = nthr >> 6;
  const int lane = tid & 63, wave = tid >> 6;
  // The arguments of a function that is not a kernel arrive in VECTOR registers, uniform or not: eight 64-bit pointers and every
  // address derived from them would live in VGPR pairs.  Read back through lane 0 they are scalars again.
  const KH_AS_LDS Geometry* g = (const KH_AS_LDS Geometry*)(uintptr_t)uni32((uint32_t)(uintptr_t)(const KH_AS_LDS Geometry*)&g_);
  KH_AS_LDS Ctl* ctl = (KH_AS_LDS Ctl*)(uintptr_t)uni32((uint32_t)(uintptr_t)(KH_AS_LDS Ctl*)ctl_);
  const gu32_t* nbrmask = (const gu32_t*)uni64((uintptr_t)nbrmask_);
  const gf32_t* wfield = (const gf32_t*)uni64((uintptr_t)wfield_);
  gu32_t* dist = (gu32_t*)uni64((uintptr_t)dist_);                   // float bit patterns (non-negative: ordered like unsigned)
  gu8_t* qs8 = (gu8_t*)uni64((uintptr_t)qstate_);                    // membership bytes: bit 0 near list being built, bit 1 far list
  q.cap = uni32(q.cap);
  gu32_t* cur = (gu32_t*)uni64((uintptr_t)q.a);
  gu32_t* next = (gu32_t*)uni64((uintptr_t)q.b);
  gu32_t* far = (gu32_t*)uni64((uintptr_t)q.c);
  gu32_t* touched = (gu32_t*)uni64((uintptr_t)q.touched);
  source = uni32(source);
  lds_bytes = uni32(lds_bytes);
  delta_floor = __uint_as_float(uni32(__float_as_uint(delta_floor)));
  lds_ = (unsigned char*)(uintptr_t)uni32((uint32_t)(uintptr_t)(KH_AS_LDS unsigned char*)lds_);
  uint32_t H = 1u;
  while (H * 24u <= lds_bytes) H <<= 1;                              // the largest power of two with 12 H <= lds_bytes
  const uint32_t NQ = H >> 1, hmask = H - 1u;
  const int hshift = __clz((int)H) + 1;
  KH_AS_LDS uint32_t* key = (KH_AS_LDS uint32_t*)(uintptr_t)lds_;
  KH_AS_LDS uint32_t* val = key + H;
  KH_AS_LDS uint32_t* curL = val + H;
  KH_AS_LDS uint32_t* nextL = curL + NQ;
  float T = RAIL ? 1e-45f : delta_floor;
  for (uint32_t s = tid; s < H; s += nthr) { key[s] = SSSP_EMPTY; val[s] = 0xFFFFFFFFu; }
  if (tid == 0) {
    ctl->n_cur = 1; ctl->n_next = 0; ctl->n_far = preseeded_far; ctl->n_far2 = 0;  // far list q.c may hold seeds
    ctl->n_touched = 0;
    ctl->best_rail = NONE64;
    ctl->retry[0] = ctl->retry[1] = 0u;
    curL[0] = source;
    __hip_atomic_store(dist + source, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (RAIL) { touched[0] = source; ctl->n_touched = 1; }
  }
  __syncthreads();
  const int gsx = g->sx, gsxy = g->sxy, gsy = g->sy, gsz = g->sz;
  const uint32_t nvox = (uint32_t)gsxy * (uint32_t)gsz;
  uint32_t par = 0u;
  for (;;) {
    // ---- near phase: label-correct everything below T
    for (;;) {
      const uint32_t n = ctl->n_cur;
      if (n == 0) break;
      // ONE THREAD PER FRONTIER VOXEL, a batch of blockDim.x voxels at a time.  A thread reads its voxel's mask and the 27 distances
      // around it as nine rows of three consecutive words (past the vector cache) -- with a weight field its 27 weights the same
      // way -- in ONE round trip whose addresses depend on nothing but the voxel; every edge that lowers a distance is offered to
      // the combine table; after the barrier the table is flushed (see above).
      for (uint32_t base = 0; base < n; base += (uint32_t)nthr) {
        const uint32_t i = base + (uint32_t)tid;
        bool pending = i < n;
        const uint32_t u = pending ? (i < NQ ? curL[i] : cur[i]) : source;
        const uint32_t zz = u / (uint32_t)gsxy, rr = u - zz * (uint32_t)gsxy, yy = rr / (uint32_t)gsx;
        if (pending) gst8_l2(qs8 + u, gld8_l2(qs8 + u) & ~1u);       // out of the near list (the only thread that holds u)
        for (;;) {
          if (pending) {
            const uint32_t nm = nbrmask[u];
            float wr[27];
            if (FIELD) rows27_plain(wfield, nvox, gsx, gsxy, gsy, gsz, u, (int)yy, (int)zz, wr);
            uint32_t dr[27];
            rows27_sc1(dist, nvox, gsx, gsxy, gsy, gsz, u, (int)yy, (int)zz, dr);
            const float du = __uint_as_float(dr[13]);
            bool failed = false;
#pragma unroll
            for (int k = 0; k < 26; k++) {
              int dx, dy, dz;
              dir_delta(k, dx, dy, dz);
              const int idx = (dx + 1) + 3 * ((dy + 1) + 3 * (dz + 1));
              const float wn = FIELD ? wr[idx] : g->w[k];
              const uint32_t nb = __float_as_uint(du + wn);
              // distances only go down, so an edge that cannot lower dist[v] now never will
              if (((nm >> k) & 1u) && nb < dr[idx])
                failed |= !sssp_offer(key, val, hmask, hshift, u + (uint32_t)(dx + gsx * dy + gsxy * dz), nb);
            }
            pending = failed;
            if (failed) ctl->retry[par] = 1u;
          }
          __syncthreads();
          // ---- flush: one thread per occupied slot
          for (uint32_t s = (uint32_t)tid; s < H; s += (uint32_t)nthr) {
            const uint32_t v = key[s];
            const bool occ = v != SSSP_EMPTY;
            uint32_t nd = 0u, old = 0u, q8 = 0u;
            float wv = 1.0f;
            if (occ) {
              nd = val[s];
              key[s] = SSSP_EMPTY;
              val[s] = 0xFFFFFFFFu;
              if (RAIL) { old = gld_l2(dist + v); wv = wfield[v]; }
              q8 = gld8_l2(qs8 + v);
              __hip_atomic_store(dist + v, nd, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            const float ndf = __uint_as_float(nd);
            const bool rail = RAIL && occ && wv == 0.0f;            // a rail: absorbing
            if (rail) __hip_atomic_fetch_min(&ctl->best_rail, pack(ndf, v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            const bool t_touch = RAIL && occ && old == INF_BITS;
            const bool t_next = occ && !rail && ndf < T && !(q8 & 1u);
            const bool t_far = occ && !rail && !(ndf < T) && !(q8 & 2u);
            if (t_next | t_far) gst8_l2(qs8 + v, q8 | (t_next ? 1u : 2u));
            if (RAIL) {
              const uint32_t p = wave_slot(t_touch, &ctl->n_touched, lane);
              if (t_touch) {
                if (p < q.cap) touched[p] = v;
                else __hip_atomic_fetch_or(&ctl->status, (uint32_t)KH_ST_QUEUE_OVERFLOW, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
              }
            }
            {
              const uint32_t p = wave_slot(t_next, &ctl->n_next, lane);
              if (t_next) {
                if (p < NQ) nextL[p] = v;
                else if (p < q.cap) next[p] = v;
                else __hip_atomic_fetch_or(&ctl->status, (uint32_t)KH_ST_QUEUE_OVERFLOW, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
              }
            }
            {
              const uint32_t p = wave_slot(t_far, &ctl->n_far, lane);
              if (t_far) {
                if (p < q.cap) far[p] = v;
                else __hip_atomic_fetch_or(&ctl->status, (uint32_t)KH_ST_QUEUE_OVERFLOW, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
              }
            }
          }
          const bool again = ctl->retry[par] != 0u;                  // (stable since the barrier above)
          if (tid == 0) {
            ctl->retry[par ^ 1u] = 0u;                               // (nobody reads or sets the other word before the next barrier)
            if (again) ctl->n_retries++;
          }
          par ^= 1u;
          __syncthreads();
          if (!again) break;
        }
      }
      if (tid == 0) {
        ctl->n_cur = ctl->n_next < q.cap ? ctl->n_next : q.cap;
        ctl->n_next = 0;
        if (ctl->n_far > q.cap) ctl->n_far = q.cap;
        if (ctl->n_cur > NQ) ctl->n_spills++;                          // the next round reads entries from HBM
      }
      { gu32_t* t = cur; cur = next; next = t; }
      { KH_AS_LDS uint32_t* t = curL; curL = nextL; nextL = t; }
      __syncthreads();
    }
    // ---- every voxel with d < T is final now
    float tcap = KH_INF;
    if (RAIL) {
      const unsigned long long br = ctl->best_rail;
      if (br != NONE64) {
        const float D = __uint_as_float((uint32_t)(br >> 32));
        if (D < T) break;
        tcap = next_up(D);
      }
    }
    const uint32_t nfar = ctl->n_far;
    if (nfar == 0) break;
    // pass 1: min / mean of the far entries (current distances)
    float mn = KH_INF, sm = 0.0f;
    uint32_t cnt = 0;
    for (uint32_t i = tid; i < nfar; i += nthr) {
      const float d = __uint_as_float(gld_l2(dist + far[i]));
      mn = fminf(mn, d); sm += d; cnt++;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      mn = fminf(mn, __shfl_xor(mn, o));
      sm += __shfl_xor(sm, o);
      cnt += __shfl_xor(cnt, o);
    }
    if (lane == 0) { ctl->red_min[wave] = mn; ctl->red_sum[wave] = sm; ctl->red_cnt[wave] = cnt; }
    __syncthreads();
    mn = ctl->red_min[0]; sm = ctl->red_sum[0]; cnt = ctl->red_cnt[0];
    for (int i = 1; i < nwav; i++) { mn = fminf(mn, ctl->red_min[i]); sm += ctl->red_sum[i]; cnt += ctl->red_cnt[i]; }
    if (RAIL && !(mn < tcap)) break;  // nothing left at or below the nearest rail
    const float mean = sm / (float)cnt;
    float step = 0.5f * (mean - mn);
    if (!(step > delta_floor)) step = delta_floor;
    float Tn = mn + step;
    if (!(Tn > mn)) Tn = next_up(mn);
    if (Tn < T) Tn = T;
    if (Tn > tcap) Tn = tcap;
    T = Tn;
    // pass 2: split far -> cur (d < T) + compacted far (into the free `next` buffer); every entry has one thread, which is the
    // only writer of the voxel's membership byte
    for (uint32_t base = 0; base < nfar; base += (uint32_t)nthr) {
      const uint32_t i = base + (uint32_t)tid;
      const bool have = i < nfar;
      const uint32_t v = have ? far[i] : source;
      const float d = __uint_as_float(gld_l2(dist + v));
      const uint32_t q8 = gld8_l2(qs8 + v) & ~2u;
      const bool near = have && d < T;
      const bool t_cur = near && !(q8 & 1u);
      const bool t_far = have && !near;
      if (have) gst8_l2(qs8 + v, q8 | (t_cur ? 1u : 0u) | (t_far ? 2u : 0u));
      const uint32_t pc = wave_slot(t_cur, &ctl->n_cur, lane);
      if (t_cur) { if (pc < NQ) curL[pc] = v; else cur[pc] = v; }    // pc < nfar <= cap
      const uint32_t pf = wave_slot(t_far, &ctl->n_far2, lane);
      if (t_far) next[pf] = v;
    }
    __syncthreads();
    if (tid == 0) {
      ctl->n_far = ctl->n_far2; ctl->n_far2 = 0;
      ctl->n_splits++;
      if (ctl->n_cur > NQ) ctl->n_spills++;
    }
    gu32_t* t = far; far = next; next = t;
    __syncthreads();
  }
  __syncthreads();
}

// ------------------------------------------------------------------------------------------------
// One distance-field search of ONE label by its workgroup (dijkstra3d.euclidean_distance_field, kimimaro/trace.py:139-145, 302-307):
// the field over the label's voxels from `source`, +inf before; task.max_loc / max_val = the farthest voxel (ties -> smallest
// linear index); mode 1 (find_root): task.root = that voxel.  Out of line: the batch kernel and the path kernel share it.
__device__ __attribute__((noinline)) void edf_label(Ctl* ctl_, kh_label_t* task, int mode, const uint32_t* __restrict__ list, uint32_t nf,
                                                    const uint32_t* __restrict__ nbrmask, float* field, uint8_t* qstate, Queues q,
                                                    float delta_floor, uint32_t source, unsigned char* lds, uint32_t lds_bytes) {
  Ctl& ctl = *ctl_;
  const Geometry& g = ctl.g;
  const int tid = threadIdx.x;
  const int nthr = blockDim.x, nwav = nthr >> 6;
  const int lane = tid & 63, wave = tid >> 6;
  for (uint32_t i = tid; i < nf; i += nthr) st_f32_l2(&field[list[i]], KH_INF);
  __syncthreads();
  uint32_t seeded = 0;
  if (mode == 2 && task->fsr > 0.0f) {
    // free_space_radius (trace.py:134,142; dijkstra3d source absent, restated in oracle ko_edf): label
    // voxels closer than the radius in a straight line get that distance and seed the search (far list).
    const float fsr = task->fsr;
    const uint32_t sxu = (uint32_t)g.sx, sxy = (uint32_t)g.sxy;
    const uint32_t z0 = source / sxy, r0 = source - z0 * sxy, y0 = r0 / sxu, x0 = r0 - y0 * sxu;
    if (tid == 0) ctl.u0 = 0;
    __syncthreads();
    for (uint32_t i = tid; i < nf; i += nthr) {
      const uint32_t v = list[i];
      if (v == source) continue;
      const uint32_t z = v / sxy, r = v - z * sxy, y = r / sxu, x = r - y * sxu;
      const float a = g.wx * (float)((int)x - (int)x0), b = g.wy * (float)((int)y - (int)y0), c = g.wz * (float)((int)z - (int)z0);
      float s2 = a * a;
      const float t2 = b * b, u2 = c * c;
      s2 = s2 + t2;
      s2 = s2 + u2;
      const float sd = sqrtf(s2);
      if (sd < fsr) {
        st_f32_l2(&field[v], sd);
        flag_or(qstate, v, 2u);
        const uint32_t p = atomicAdd(&ctl.u0, 1u);
        q.c[p] = v;  // p < nf <= cap
      }
    }
    __syncthreads();
    seeded = ctl.u0;
  }
  sssp<0>(ctl.g, nbrmask, nullptr, field, qstate, source, q, &ctl, delta_floor, lds, lds_bytes, seeded);
  // farthest voxel: max finite distance, ties -> smallest linear index
  unsigned long long best = 0;
  for (uint32_t i = tid; i < nf; i += nthr) {
    const uint32_t v = list[i];
    const uint32_t b = __float_as_uint(ld_f32_l2(&field[v]));
    if (b == INF_BITS) continue;
    const unsigned long long key = ((unsigned long long)b << 32) | (0xFFFFFFFFu - v);
    if (key > best) best = key;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long ob = __shfl_xor(best, o);
    if (ob > best) best = ob;
  }
  if (lane == 0) ctl.red64[wave] = best;
  __syncthreads();
  if (tid == 0) {
    for (int i = 1; i < nwav; i++) if (ctl.red64[i] > best) best = ctl.red64[i];
    const uint32_t loc = 0xFFFFFFFFu - (uint32_t)best;
    task->max_loc = loc;
    task->max_val = __uint_as_float((uint32_t)(best >> 32));
    if (mode == 1) task->root = loc;
    ctl.red64[0] = best;          // (for the callers' other threads: the record itself was written by this thread only)
  }
  __syncthreads();
}

}  // namespace kh
