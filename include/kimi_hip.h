/*
 * kimi_hip.h -- C ABI of libkimi_hip.so, the MI355X (gfx950) implementation of the
 * kimimaro TEASAR hot path.
 *
 * Conventions
 *   - every entry point returns an int status (KH_OK == 0); kh_last_error() gives text.
 *     Nothing throws across the boundary (the reference's C++ `throw` at
 *     ext/skeletontricks/dijkstra_invalidation.hpp:54-58 would abort the process).
 *   - all volume pointers are DEVICE pointers (HBM resident), Fortran ordered:
 *     linear index = x + sx*(y + sy*z)  (ext/skeletontricks/skeletontricks.pyx:398).
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).  Calls are
 *     asynchronous unless stated; the caller synchronises.
 *   - caller allocates everything; the library never frees caller memory.
 *   - labels are "connected component ids" 1..N (0 = background) as produced by
 *     kimimaro/utility.py:58-83; label_bytes is 2 or 4.
 *
 * The whole-volume design: because connected components are disjoint, the per-label
 * fields of the reference (DAF, PDRF, parents/dist, the invalidation mask -- all
 * per-crop numpy arrays in kimimaro/trace.py) live in ONE set of whole-volume arrays
 * shared by all labels, and the per-label kernels run one workgroup per label.
 */
#ifndef KIMI_HIP_H
#define KIMI_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KH_OK 0
#define KH_EINVAL 1      /* bad argument */
#define KH_EHIP 2        /* a HIP runtime call failed */
#define KH_ENODEVICE 3   /* no gfx950 device visible */

/* per-label status bits written by the device kernels (kh_label_t.status) */
#define KH_ST_OK 0u
#define KH_ST_QUEUE_OVERFLOW 1u   /* search work list overflow (scratch too small) */
#define KH_ST_HEAP_OVERFLOW 2u    /* invalidation heap overflow */
#define KH_ST_PATH_OVERFLOW 4u    /* path output buffer overflow */
#define KH_ST_NO_RAIL 8u          /* railroad: no rail reachable from a target */
#define KH_ST_PLATEAU 16u         /* a float-absorption plateau search found no exit (scratch exhausted) */
#define KH_ST_BAD_TARGET 32u      /* a target / root outside the label */

int kh_version(void);
/* copies the last error message of the calling thread, returns its length */
int kh_last_error(char* buf, int len);
/* number of visible devices whose arch is gfx950; 0 => every compute entry point fails loudly */
int kh_device_count(void);

/* ---- a1: edt.edt(labels, anisotropy, black_border) ---------------------------------
 * replaces: edt.edt as called at kimimaro/intake.py:178-183 and kimimaro/trace.py:112-117.
 * labels: u8/u16/u32 [sx,sy,sz]; out: f32 same shape; workspace: f32 of the same shape (ping-pong buffer, sx*sy*sz floats).
 * Squared distances are accumulated exactly as documented in oracle/kimi_oracle.c (ko_edt). */
int kh_edt(const void* labels, int label_bytes, int64_t sx, int64_t sy, int64_t sz,
           float wx, float wy, float wz, int black_border,
           float* workspace, float* out, void* stream);

/* kh_edt for an array of `ndim` (1..3) dimensions, the trailing axes having extent 1: edt.edt on a 2-D array is a
 * 2-D transform -- with black_border the missing axes have no border (kimimaro/intake.py:568 calls it on the six
 * faces of the volume).  kh_edt == kh_edt_nd(ndim = 3).                                                       */
int kh_edt_nd(const void* labels, int label_bytes, int ndim, int64_t sx, int64_t sy, int64_t sz,
              float wx, float wy, float wz, int black_border,
              float* workspace, float* out, void* stream);

/* kh_edt with each pass bracketed by HIP events on `stream`; ms3 (HOST pointer) receives the
 * x / y / z pass durations in milliseconds.  Synchronises the stream (measurement only).       */
int kh_edt_timed(const void* labels, int label_bytes, int64_t sx, int64_t sy, int64_t sz,
                 float wx, float wy, float wz, int black_border,
                 float* workspace, float* out, void* stream, float* ms3);

/* ---- preamble statistics on the device (fastremap.unique counts intake.py:198,
 * np.max(DBF) trace.py:100, first_label skeletontricks.pyx:307-326, x extent of
 * scipy.ndimage.find_objects utility.py:85-102) ------------------------------------
 * For every label id in [0, nlabels]: voxel count, max DBF, smallest linear index,
 * min/max x, and (yz_extent, nullable, 4 entries per label) [ymin, ymax, zmin, zmax].  All outputs
 * are device arrays of nlabels+1 entries, zero/identity initialised by the call.           */
int kh_label_stats(const void* labels, int label_bytes, const float* dbf, int64_t nvox, int64_t sx, int64_t sy,
                   int64_t nlabels, uint32_t* counts, float* dbf_max, uint32_t* first_index,
                   uint32_t* xmin, uint32_t* xmax, uint32_t* yz_extent, void* stream);

/* scatter the voxel indices of the selected labels into per-label lists.
 * slot_of_label: device int32[nlabels+1], -1 = label not selected, else its slot;
 * offsets: device u32[nslots] start of each slot's list in `lists`;
 * cursors: device u32[nslots] scratch (zeroed by the call).  Order inside a list is
 * unspecified (every consumer is order independent).                                  */
int kh_scatter_lists(const void* labels, int label_bytes, int64_t nvox, const int32_t* slot_of_label,
                     int64_t nslots, const uint32_t* offsets, uint32_t* cursors, uint32_t* lists, void* stream);

/* 26-bit same-label connectivity mask per voxel (bit i = neighbour i of the order in
 * dijkstra_invalidation.hpp:60-124 is inside the volume and has the same non-zero
 * label).  The optional voxel_graph of the reference is ANDed in by the caller (NULL
 * in every config).                                                                   */
int kh_neighbor_mask(const void* labels, int label_bytes, int64_t sx, int64_t sy, int64_t sz,
                     uint32_t* nbrmask, void* stream);

/* ---- per-label task descriptor (device array, one per selected label) -------------- */
typedef struct kh_label_t {
  uint32_t segid;        /* connected component id */
  uint32_t list_offset;  /* start of its voxel list */
  uint32_t count;        /* Nf */
  uint32_t xmin, xmax;   /* x extent of its bounding box (heap-order quirk, see paths.hip) */
  uint32_t source;       /* in: search source (linear index) for kh_edf_batch */
  uint32_t max_loc;      /* out: location of the farthest voxel */
  float max_val;         /* out: its distance */
  float M;               /* f32(1/dbf_max**1.01), kimimaro/trace.py:336 (host numpy) */
  uint32_t root;         /* root voxel (linear index) */
  uint32_t q_offset;     /* start of its slice of the work-list scratch (entries) */
  uint32_t q_capacity;   /* entries per work list */
  uint32_t heap_offset;  /* start of its invalidation heap slice (nodes) */
  uint32_t heap_capacity;
  uint32_t path_offset;  /* start of its slice of the path vertex buffer */
  uint32_t path_capacity;
  uint32_t tgt_offset;   /* manual targets: [tgt_offset, +n_before) before, then n_after after */
  uint32_t n_before, n_after;
  uint32_t max_paths;    /* 0 = unlimited (trace.py:214-215) */
  uint32_t n_paths;      /* out */
  uint32_t n_vertices;   /* out: vertices written to the path buffer */
  uint32_t status;       /* out: KH_ST_* bits */
  uint32_t stat_settled; /* out: sum of voxels touched by the railroad searches */
  uint32_t stat_heap_pushes; /* out (low 32 bits) */
  uint32_t cyc_target;   /* out: shader kilo-cycles spent in the target finder */
  uint32_t cyc_rail;     /* out: ... in railroad search + back-track */
  uint32_t cyc_inval;    /* out: ... in the invalidation flood, of which: */
  uint32_t cyc_pop;      /* out:   heap pops */
  uint32_t cyc_push;     /* out:   heap pushes */
  uint32_t cyc_fire;     /* out:   neighbour evaluation of live pops */
  /* soma mode (kimimaro/trace.py:119-134,160-168,246-251); all zero for ordinary labels */
  uint32_t soma_mode;    /* 1: root is the soma centre, one-off invalidation around it, paths are trimmed */
  float fsr;             /* free_space_radius of the DAF search = DBF[root] (trace.py:134) */
  float soma_radius;     /* dbf_max * soma_invalidation_scale + soma_invalidation_const (float32, trace.py:127) */
  float soma_scale;      /* soma_invalidation_scale */
  float soma_const;      /* soma_invalidation_const */
  /* order-free invalidation sweep (csrc/sweep.h); nlev == 0 switches it off for the label */
  uint32_t nlev;         /* in: number of distinct keys below the label's largest ball radius (levels it can touch) */
  float sweep_rmax;      /* in: a call whose largest radius exceeds this uses the heap emulation */
  uint32_t ev_offset;    /* in: start of its event arena, in units of 256 bytes */
  uint32_t ev_chunks;    /* in: event chunks in its arena */
  uint32_t ev_shift;     /* in: log2(slots per chunk), 4..7 (8 bytes per slot, slot 0 links the level's chunks) */
  uint32_t stat_sweep_calls;  /* out: invalidation calls tried by the sweep */
  uint32_t stat_sweep_bails;  /* out: ... of which fell back to the heap emulation */
  uint32_t stat_sweep_levels; /* out: levels processed */
  uint32_t stat_sweep_events; /* out: events processed (low 32 bits) */
  uint32_t stat_sweep_why;    /* out: OR of the bail reasons (sweep.h SW_BAIL_*) */
  uint32_t lev_window;   /* in: 0, or a power of two (>= 64) larger than the number of levels any event of this label can lie
                            ahead of the level being processed (= distinct keys within one 26-neighbour step of any key below
                            the label's radius, from the key table): the label then keeps lev_window level words, used round
                            robin, instead of nlev.  A bound that turns out too small costs speed, not results (the event
                            abandons the call to the heap emulation). */
  uint32_t ev_spill;     /* in: entries of the sweep's candidate-spill table at the front of the arena (0 or a power of two; 12 bytes
                            each, rounded up to 256 bytes): the fifth to eighth possible owner of a voxel (csrc/sweep.h) */
  uint32_t stat_ghost_calls;  /* out: calls of the sweep that left voxels undecided and went on with them as ghosts */
  uint32_t stat_rollbacks;    /* out: times the label rolled back to such a call and redid it by the heap emulation */
  /* KH_TRACE_FUSED_EDF: compute_pdrf's parameters (kimimaro/trace.py:315-356, the repeated-squaring branch) */
  uint32_t pdrf_log2e;   /* in: log2 of pdrf_exponent */
  float pdrf_scale;      /* in: pdrf_scale */
  /* regime counters of the searches (csrc/sssp.h sssp; kh_edf_batch, kh_path_search and kh_trace_paths ADD to them): what
     tests/test_gpu_search_regimes.py asserts before it compares a result */
  uint32_t stat_search_retries; /* out: flush rounds repeated because an offer found the combine table full */
  uint32_t stat_search_spills;  /* out: near-list rounds that started with more entries than the LDS part holds */
  uint32_t stat_search_splits;  /* out: far-list splits executed (pass 1 + pass 2 = one) */
} kh_label_t;

/* ---- a4: dijkstra3d.euclidean_distance_field for a batch of labels ------------------
 * replaces the calls at kimimaro/trace.py:139-145 and :302-307.  For every task: the
 * distance field from task.source over its label (26-connected, anisotropic edge
 * lengths, f32 accumulation) is written into `field` at the label's voxels (other
 * voxels untouched); task.max_loc / max_val receive the farthest voxel (ties ->
 * smallest linear index).  queues: device u32[...] scratch addressed by q_offset (4 lists
 * of q_capacity >= count entries per task); qstate: u8 per voxel, all zero on entry and on exit
 * (two membership bits per voxel keep every work list bounded by the label size).
 * mode 0: source = task.source.
 * mode 1 (find_root, trace.py:291-308): only tasks with root == 0xFFFFFFFF run; afterwards
 *         task.root = max_loc.   mode 2 (DAF, trace.py:139-145): source = task.root.
 * Bits 8.. of `mode`: threads per label (a multiple of 64 up to 1024; 0 = 512).                  */
int kh_edf_batch(kh_label_t* tasks, int ntasks, int mode, const uint32_t* lists, const uint32_t* nbrmask,
                 int64_t sx, int64_t sy, int64_t sz, float wx, float wy, float wz,
                 float* field, uint8_t* qstate, uint32_t* queues, void* stream);

/* ---- voxel_graph of dijkstra3d.* / roll_invalidation_ball_inside_component (kimimaro/trace.py:139-145,155,167,240-242,257;
 * dijkstra_invalidation.hpp:126-191): nbrmask[v] &= the directions the caller's connectivity word graph[v] allows (cc3d's bit layout,
 * read at the CURRENT voxel like the reference does).  Every search and the invalidation take their neighbourhoods from nbrmask, so
 * after this call they honour the graph.  corner_gate (nullable, u8 per voxel): bit j = the yz diagonal that corner entry 18 + j
 * degenerates into at an x face of the array exists AND the corner's own bit is set (dijkstra_invalidation.hpp:116-123 + :182-190);
 * kh_invalidate_ball takes it so that the heap emulation pushes the same duplicates as the reference there.                    */
int kh_apply_voxel_graph(uint32_t* nbrmask, const uint32_t* graph, int64_t nvox, uint8_t* corner_gate, void* stream);

/* ---- a3+a5: zero2inf / inf2zero / compute_pdrf fused, whole volume ------------------
 * replaces kimimaro/trace.py:138,146,148 (skeletontricks.pyx:177-224, trace.py:315-356).
 * For every voxel of a selected label: daf *= 1/max_daf (max_daf = task.max_val, skipped
 * when 0), pdrf = ((1 - dbf*M)^(2^log2_exponent)) * scale + daf, each op rounded to f32.
 * Voxels of unselected labels / background get pdrf = +inf.                           */
/* Exponents that are not a power of two take the reference's np.power branch (kimimaro/trace.py:346-347), whose rounding
 * is that of the host's numpy (libm / SVML powf -- machine dependent, so no device powf can promise the same bits).
 * The call is then made twice around the host's own np.power on the pdrf buffer:
 *   log2_exponent = KH_PDRF_BASE    pdrf = 1 - dbf*M for the selected voxels (+inf elsewhere), daf untouched;
 *   (host: np.power(pdrf, exponent, out=pdrf) in float32)
 *   log2_exponent = KH_PDRF_FINISH  pdrf = pdrf*scale + daf/max_daf, daf normalised in place -- the tail of the normal call. */
#define KH_PDRF_BASE (-1)
#define KH_PDRF_FINISH (-2)
#define KH_PDRF_KEEP_OTHERS 0x100   /* ORed into a log2_exponent >= 0: the voxels of unselected labels are left as they are (instead of
                                       +inf) -- the selected labels are only a part of what another launch computes into the same volume */
int kh_pdrf(const void* labels, int label_bytes, int64_t nvox, const int32_t* slot_of_label,
            const kh_label_t* tasks, const float* dbf, float* daf, int log2_exponent, float scale,
            float* pdrf, void* stream);

/* ---- a6..a11: the per-label TEASAR path loop ---------------------------------------
 * replaces kimimaro/trace.py:196-267 (compute_paths) with its callees
 * CachedTargetFinder.find_target (skeletontricks.pyx:1008-1045), dijkstra3d.railroad
 * (trace.py:240-242), roll_invalidation_ball_inside_component (skeletontricks.pyx:373-418
 * -> dijkstra_invalidation.hpp:239-332) and the rail edits trace.py:220,261-263.
 * alive: u8 per voxel, 1 for the voxels of selected labels (mutated: invalidation);
 * pdrf: mutated (rails are zeroed); dist: f32 scratch volume, must be +inf on entry and
 * is +inf again on exit; list_daf: DAF gathered in list order (target finder keys).
 * Paths are written as linear indices, rail end first, into path_vertices with
 * path_lengths (one u32 per path, same slice offsets /capacity as the vertices).
 * qstate as for kh_edf_batch.  heap_nodes: scratch for the invalidation heaps, 16 bytes per node
 * (16-byte aligned), each label owning nodes [heap_offset, heap_offset + heap_capacity).
 * Invalidation runs as the order-free level sweep of csrc/sweep.h whenever that certifies the call (the result is
 * then independent of the heap's tie order, hence equal to the reference's), and as the exact emulation of
 * std::priority_queue otherwise.  The sweep needs: level_rank = u32 [ra, rb, rc] table (x fastest) of the rank of
 * the key of offset (a, b, c) among the distinct keys (kh_level_keys + sort/unique by the caller), cstate = one
 * zeroed u64 per voxel (zero again on exit), event_arena = 256-byte aligned scratch addressed by ev_offset /
 * ev_chunks / ev_shift / nlev / lev_window of each task; max_nlev = the number of level words every workgroup of the launch
 * gets in LDS (<= KH_SWEEP_LDS_LEVELS): a task keeps its words there when its lev_window (if non-zero) or else its nlev fits;
 * a task for which neither does runs all its invalidations as the heap emulation.  A task's arena = the candidate-spill table,
 * a free stack of ev_chunks u32 (each rounded up to 256 bytes), then the chunks.  level_rank == NULL switches the sweep off.
 * sched = one u32 per voxel, 0xFFFFFFFF on entry: the sweep's filter words (csrc/sweep.h) -- the pending deadline of a live voxel
 * (with it a voxel is handed ~1.3 events per call instead of ~13), 0 once the voxel is dead (the sweep reads its neighbours' state
 * from these words, nine rows of three per event: the word BEFORE sched[0] and the word behind the last one must be readable).
 * NULL switches the sweep off.
 * Integer levels (round 6): level_rank == NULL and ra > 0 selects them -- (ra, rb, rc) = (wx^2, wy^2, wz^2) / gcd for an integral
 * anisotropy whose squared distances stay exact in float over the balls' reach (kimimaro_amd.engine.int_key_mode checks it): the
 * level of a key is then the integer key^2 / gcd itself, no table, no float operation per neighbour; task.nlev / lev_window count
 * such integers.  level_rank == NULL and ra == 0: no sweep.
 * Ghosts: journal (nullable) = u32 scratch, 2 * q_capacity entries per task at 2 * q_offset; rail_save (nullable)
 * = f32 scratch laid out like path_vertices.  With both, a call of the sweep that leaves voxels undecided goes on with them as
 * "ghosts" instead of running the heap emulation at once; the label rolls back to that call and redoes it exactly only if a
 * ghost would influence the loop.  Results are identical either way (KH_TRACE_NO_GHOSTS switches it off for A/B runs,
 * KH_TRACE_GHOST_PARANOID rolls every such call back at once -- a test of the roll-back itself).  Each task's arena starts with
 * its candidate-spill table (ev_spill entries of 12 bytes, rounded up to 256 bytes), then the free stack, then the chunks.
 * flags: KH_TRACE_PROFILE also fills cyc_pop / cyc_push / cyc_fire (slower kernel variant); KH_TRACE_HEAP_PRIO see below.
 * fix_branching = 0 selects the parental-field variant (trace.py:155,244): one weighted Dijkstra
 * from the root, paths returned root -> target.                                                  */
#define KH_TRACE_PROFILE 1
#define KH_TRACE_HEAP_PRIO 2   /* the wave running the heap emulation raises its issue priority (several volumes in flight) */
#define KH_TRACE_THREADS_64 4  /* workgroups of 64 threads (one wave per label, up to 12 labels per CU) instead of 256 */
#define KH_TRACE_THREADS_128 8 /* workgroups of 128 threads */
#define KH_TRACE_NO_GHOSTS 16  /* undecided voxels abandon the call to the heap emulation at once (rounds 2-4) */
#define KH_TRACE_GHOST_PARANOID 32  /* roll back after every call that made a ghost (tests) */
#define KH_TRACE_VOXEL_GRAPH 128    /* nbrmask went through kh_apply_voxel_graph (voxel_graph= of kimimaro.trace.trace): the edges are
                                       one-way, the predecessor walks read the step u -> v from u's word; corner_gate = the array that
                                       call filled (NULL without a graph) */
#define KH_TRACE_BIG_LDS_HEAP 64    /* two chunks (8191 nodes, 128 KiB) of every label's invalidation heap live in LDS: one workgroup
                                       per CU, for a launch of the few largest labels whose heap emulation sets the wall clock */
#define KH_TRACE_SCRATCH_POOL 256   /* heap_nodes is ONE pool for the launch instead of a slice per label: node 0 = {u32 nodes handed out so
                                       far (the caller sets 1), u32 nodes in the pool, -, -}; a label takes its heap (heap_capacity nodes) when
                                       it first runs the heap emulation and its ghost journal ((2 * q_capacity + 3) / 4 nodes) when it first
                                       makes a ghost; `journal` is ignored, heap_offset too.  A label the pool cannot serve ends with
                                       KH_ST_HEAP_OVERFLOW (trace it again with a slice of its own) or goes on without ghosts. */
#define KH_TRACE_FUSED_EDF 512      /* the label's workgroup runs find_root, the DAF search and compute_pdrf itself before its path loop
                                       (what kh_edf_batch modes 1 and 2, kh_gather_f32 and kh_pdrf do for all labels at once): a task with
                                       root == 0xFFFFFFFF gets its root from the search from task.source; list_daf and pdrf are OUTPUTS for
                                       the tasks' voxels (pdrf elsewhere is not read), dist serves as the searches' field; task.M,
                                       pdrf_log2e, pdrf_scale, fsr as for kh_pdrf / kh_edf_batch.  Only the power-of-two exponents. */
#define KH_SWEEP_LDS_LEVELS 16384   /* level words kept in LDS up to this many levels per label */
int kh_trace_paths(kh_label_t* tasks, int ntasks, const uint32_t* lists, float* list_daf,
                   const uint32_t* nbrmask,
                   int64_t sx, int64_t sy, int64_t sz, float wx, float wy, float wz,
                   const float* dbf, float* pdrf, float* dist, uint8_t* alive, uint8_t* qstate,
                   const uint32_t* manual_targets, float scale, float constant,
                   uint32_t* queues, void* heap_nodes,
                   uint32_t* path_vertices, uint32_t* path_lengths,
                   const uint32_t* level_rank, int64_t ra, int64_t rb, int64_t rc, int64_t max_nlev,
                   uint64_t* cstate, uint32_t* sched, void* event_arena, uint32_t* journal, float* rail_save,
                   const uint8_t* corner_gate, int flags, int fix_branching, void* stream);

/* keys[a + ra*(b + rb*c)] = the flood's key of the voxel offset (a, b, c): sqrt(fl(fl((wx*a)^2 + (wy*b)^2) + (wz*c)^2)),
 * float operation order of dijkstra_invalidation.hpp:310-316.  Device array of ra*rb*rc floats.              */
int kh_level_keys(int64_t ra, int64_t rb, int64_t rc, float wx, float wy, float wz, float* keys, void* stream);

/* ---- a9 on its own: kimimaro.skeletontricks.roll_invalidation_ball_inside_component(labels, DBF, scale, const,
 * anisotropy, path) (skeletontricks.pyx:373-418 -> dijkstra_invalidation.hpp:239-332) for ONE object, the device routine
 * of the path loop behind its own entry point.  task: a kh_label_t of the object (count, xmin, xmax, list_offset,
 * q_offset / q_capacity, heap_offset / heap_capacity and the sweep fields as for kh_trace_paths); alive: u8 per voxel,
 * 1 for the object's voxels that are still valid (mutated in place like the reference's `labels`); path: u32 linear
 * indices of the path vertices; *invalidated (device int64) = number of voxels invalidated by the call.
 * The ball radius of vertex v is f32(f32(scale * dbf[v]) + constant).  Sweep arguments as for kh_trace_paths.
 * corner_gate: NULL, or the array kh_apply_voxel_graph filled (voxel_connectivity_graph=, skeletontricks.pyx:380,405-416).      */
int kh_invalidate_ball(kh_label_t* task, const uint32_t* lists, const uint32_t* nbrmask,
                       int64_t sx, int64_t sy, int64_t sz, float wx, float wy, float wz,
                       const float* dbf, uint8_t* alive, uint32_t* queues, void* heap_nodes,
                       const uint32_t* path, int64_t npath, float scale, float constant,
                       const uint32_t* level_rank, int64_t ra, int64_t rb, int64_t rc, int64_t max_nlev,
                       uint64_t* cstate, uint32_t* sched, void* event_arena, const uint8_t* corner_gate, int64_t* invalidated,
                       void* stream);

/* ---- the invalidation heap on its own (csrc/heap.h: the wave-cooperative emulation of std::priority_queue with
 * Compare = `a.dist >= b.dist`), driven by a script.  For tests; the product does not call it.  One workgroup of one wave builds
 * the heap exactly as kh_trace_paths does (topl 1: 127 slots in LDS and the key mirror of slots 127..2046; topl 2, the heap of
 * KH_TRACE_BIG_LDS_HEAP: 8191 slots in LDS, no mirror; cap = min(capacity, what a pop can descend through)) and walks `ops`.
 *   ops     device array of nops records of four uint32 words {op, a, b, c}:
 *             {0, key bits, payload, source}  push: a push at n >= cap is refused and counted in state[1]
 *             {1, -, -, -}                    pop: appends {key bits, payload, source, n before the pop} of the top to `pops`, then
 *                                             removes it.  On an empty heap: counted in state[2], skipped.
 *             {2, flags, -, -}                dump: appends to `dumps` the header {n, index of this record}, then the n nodes in slot
 *                                             order (four words each: key bits, payload, source, the unused word), then -- topl 1 --
 *                                             the mirror's key words of slots 127 .. min(n, 2047)-1.  flags bit 0: the header only.
 *           Any other op is counted in state[2] and skipped.  Keys are the bit patterns of non-negative floats below +inf.
 *   nodes   device array of nodes_allocated 16-byte nodes, 16-byte aligned: the heap's slots in memory (slots below 127 / 8191 live
 *           in LDS and are never written here).  nodes_allocated >= max(capacity, 128 / 8192): a clamped load reads slot 127 / 8191.
 *   pops, dumps   device arrays of pops_capacity / dumps_capacity uint32 WORDS.  A pop record or a dump that does not fit is not
 *           written (the pop itself still happens) and counted in state[3].
 *   state   four device words, written at the end: {n, refused pushes, script errors, records that did not fit}.        */
int kh_heap_script(int topl, const uint32_t* ops, int64_t nops, void* nodes, int64_t nodes_allocated, uint32_t capacity,
                   uint32_t* pops, int64_t pops_capacity, uint32_t* dumps, int64_t dumps_capacity, uint32_t* state, void* stream);

/* ---- the flood on that heap on its own (csrc/heap.h, invalidate_ball): ONE call of the heap emulation of
 * roll_invalidation_ball_inside_component by one workgroup of one wave, without the sweep, the ghosts and the scratch pool that
 * surround it in kh_trace_paths and kh_invalidate_ball.  For tests; the product does not call it.
 *   topl     1 or 2: the heap as for kh_heap_script (2 is the heap of KH_TRACE_BIG_LDS_HEAP); profile: 0, or 1 for the build that
 *            KH_TRACE_PROFILE selects (the pop / push / neighbour-test cycle split).
 *   sx, sy, sz, wx, wy, wz   the volume's extents and anisotropy.
 *   nbrmask  the words of kh_neighbor_mask, or those words after kh_apply_voxel_graph; corner_gate: NULL, or the array
 *            kh_apply_voxel_graph filled.  dbf: f32 per voxel.  alive: u8 per voxel, mutated in place like the reference's `labels`.
 *   path     npath u32 linear indices of the sources (each below sx*sy*sz; the ball radius of source v is
 *            f32(f32(scale * dbf[v]) + constant)); xmin, xmax: the x extent the degenerate corner entries are judged by (kh_label_t).
 *   nodes, nodes_allocated, capacity   as for kh_heap_script: a push at n >= min(capacity, what a pop can descend through) is refused
 *            and sets KH_ST_HEAP_OVERFLOW in the status word; nothing at or behind `capacity` is written.
 *   state    three device words, written at the end: {voxels invalidated, pushes (refused ones included), status bits (KH_ST_*)}.
 *   cyc3     three device uint64, written at the end: the cycles spent in pops, pushes and neighbour tests; all zero unless profile. */
int kh_heap_flood(int topl, int profile, int64_t sx, int64_t sy, int64_t sz, float wx, float wy, float wz,
                  const uint32_t* nbrmask, const uint8_t* corner_gate, const float* dbf, uint8_t* alive,
                  const uint32_t* path, int64_t npath, float scale, float constant, uint32_t xmin, uint32_t xmax,
                  void* nodes, int64_t nodes_allocated, uint32_t capacity, uint32_t* state, uint64_t* cyc3, void* stream);

/* ---- a7 / a8 on their own: one search on one object (the path loop has them inside kh_trace_paths).
 * field: the weight volume (PDRF; +inf outside the object); dist: f32 volume, +inf on entry; qstate / queues as for
 * kh_edf_batch; task: the object's kh_label_t (q_offset / q_capacity, count).
 *   mode 0  dijkstra3d.railroad(field, source) (kimimaro/trace.py:240-242): path from `source` to the nearest voxel of
 *           weight 0, written rail end first; dist is +inf again on exit.
 *   mode 1  the search of dijkstra3d.parental_field(field, source) (trace.py:155): leaves the distances in `dist`.
 *   mode 2  dijkstra3d.path_from_parents(parents, target) (trace.py:244) on that `dist`: path source -> target.
 * *path_length (device u32) = vertices written (0 on failure, see task.status).  Ties between equally short paths are
 * resolved by the canonical predecessor rule of DESIGN.md 3.3 (dijkstra3d's own tie order is not observable: its
 * source is absent from the reference tree).  voxel_graph != 0: nbrmask went through kh_apply_voxel_graph (voxel_graph= of the
 * dijkstra3d calls): one-way edges, the predecessor walk reads the step u -> v from u's word.                          */
int kh_path_search(kh_label_t* task, int mode, const uint32_t* lists, const uint32_t* nbrmask,
                   int64_t sx, int64_t sy, int64_t sz, float wx, float wy, float wz,
                   const float* field, float* dist, uint8_t* qstate, uint32_t* queues,
                   uint64_t source, uint64_t target, uint32_t* path, int64_t path_capacity, uint32_t* path_length,
                   int voxel_graph, void* stream);

/* ---- a7 as ARRAYS: dijkstra3d.parental_field(field, source) -> parents and dijkstra3d.path_from_parents(parents, target)
 * (kimimaro/trace.py:155, 244).  The reference's caller edits the parents array between the two calls
 * (`parents[tuple(root)] = 0`, trace.py:220), so it has to be a plain array the caller owns.
 * kh_parental_field: the search of kh_path_search mode 1 (distances left in `dist`; task / lists / nbrmask / qstate / queues as
 *   there) followed by the canonical predecessor rule on every voxel of the object (oracle ko_parental_field):
 *   parents[v] = linear index of pred(v) + 1, 0 = none (the source, unreachable voxels, everything outside the object).
 *   parents: u32 [sx*sy*sz], zeroed by the call.  A voxel whose achieving neighbours all lie at its own distance (float
 *   absorption plateau) cannot be expressed as a pointer: task.status gets KH_ST_PLATEAU (like the oracle's KO_EPLATEAU).
 * kh_path_from_parents: the pointer chase target -> ... -> a voxel whose entry is 0, written source first; *path_length = 0
 *   when path_capacity is too small (or the caller's edits made a cycle).                                               */
int kh_parental_field(kh_label_t* task, const uint32_t* lists, const uint32_t* nbrmask, int64_t sx, int64_t sy, int64_t sz,
                      const float* field, float* dist, uint8_t* qstate, uint32_t* queues, uint64_t source,
                      uint32_t* parents, int voxel_graph, void* stream);
int kh_path_from_parents(const uint32_t* parents, int64_t nvox, uint64_t target, uint32_t* path, int64_t path_capacity,
                         uint32_t* path_length, void* stream);

/* ---- a3 / a5 / a6 as stand-alone operations (the path loop has them fused: kh_pdrf, kh_trace_paths) ----------------
 * kh_zero2inf / kh_inf2zero: skeletontricks.zero2inf / inf2zero (skeletontricks.pyx:177-224), in place.
 * kh_pdrf_field: compute_pdrf (kimimaro/trace.py:315-356) on every element: out = ((1 - dbf*M)^(2^log2_exponent)) * scale
 *   (+ daf / max_daf, with daf normalised in place, when max_daf != 0); every operation rounded to f32.  KH_PDRF_BASE /
 *   KH_PDRF_FINISH as for kh_pdrf (the two halves around the host's np.power for other exponents).
 * kh_target_max: CachedTargetFinder.find_target (skeletontricks.pyx:1008-1045) over a voxel list with its DAF values:
 *   *out (device u64) = 1<<63 | DAF bits << 32 | voxel of the valid (alive != 0) voxel with the largest DAF, ties ->
 *   largest index; 0 when no voxel is valid.                                                                       */
int kh_zero2inf(float* f, int64_t n, void* stream);
int kh_inf2zero(float* f, int64_t n, void* stream);
int kh_pdrf_field(const float* dbf, float* daf, int64_t n, float M, int log2_exponent, float scale, float max_daf,
                  float* out, void* stream);
int kh_target_max(const uint32_t* list, const float* list_daf, const uint8_t* alive, int64_t n, uint64_t* out, void* stream);
/* kh_find_target: the legacy skeletontricks.find_target(labels, PDRF) (skeletontricks.pyx:331-367): the first voxel in the
 *   reference's scan (x outermost, z innermost) whose field value is the maximum over the mask (strict >, from -inf).
 *   labels u8 / field f32 [sx,sy,sz] Fortran ordered; *out (device u64) = 0 when the mask is empty (the reference returns
 *   (-1,-1,-1)), else orderable value bits << 32 | (0xFFFFFFFF - (x*sy + y)*sz - z).
 * kh_first_label: skeletontricks.first_label (skeletontricks.pyx:307-326): *out (device u64) = smallest linear index of a
 *   non-zero voxel, ~0 when there is none (the reference returns None).                                              */
int kh_find_target(const uint8_t* labels, const float* field, int64_t sx, int64_t sy, int64_t sz, uint64_t* out, void* stream);
int kh_first_label(const uint8_t* labels, int64_t n, uint64_t* out, void* stream);

/* small helpers used by the host mirror */
int kh_fill_f32(float* p, int64_t n, float v, void* stream);
int kh_fill_u8(uint8_t* p, int64_t n, int v, void* stream);
int kh_gather_f32(const float* src, const uint32_t* idx, int64_t n, float* out, void* stream);
/* alive[v] = 1 where slot_of_label[label[v]] >= 0 else 0 */
int kh_init_alive(const void* labels, int label_bytes, int64_t nvox, const int32_t* slot_of_label,
                  uint8_t* alive, void* stream);

/* ---- a10: roll_invalidation_cube (skeletontricks.pyx:766-836 -> skeletontricks.hpp:42-155)
 * not on the reference's own skeletonize() call graph, exported and tested there
 * (automated_test.py:632-825).  mask: u8 device [sx,sy,sz], mutated; path: device u64
 * linear indices; *invalidated (device int64) receives the count.                      */
int kh_invalidate_cube(uint8_t* mask, const float* dbf, int64_t sx, int64_t sy, int64_t sz,
                       float wx, float wy, float wz, const uint64_t* path, int64_t npath,
                       float scale, float constant, int64_t* invalidated, void* stream);

/* ---- preamble row f1: 26-connected multi-label connected components on the DEVICE.
 * replaces cc3d.connected_components + fastremap.renumber/refit as called at kimimaro/utility.py:58-83.
 * labels: u8/u16/u32/u64 [sx,sy,sz]; out: u32 component ids 1..N by first appearance in the F-order raster
 * (the numbering of kh_host_ccl26); parent: u32 scratch [nvox]; chunk_counts: u32 scratch [ceil(nvox/1024)];
 * representative: u32 [nvox+1 worst case; N+1 used], representative[id] = smallest linear index of the
 * component (skeletontricks.get_mapping, skeletontricks.pyx:490-525, reads the original label there);
 * *ncomponents (device u32) = N.  out16 (nullable, u16 [nvox]): filled with the same ids when N < 65536
 * (fastremap.refit, kimimaro/utility.py:79), untouched otherwise.                                     */
int kh_ccl26(const void* labels, int label_bytes, int64_t sx, int64_t sy, int64_t sz, uint32_t* parent,
             uint32_t* chunk_counts, uint32_t* out, uint32_t* representative, uint32_t* ncomponents,
             uint16_t* out16, void* stream);

/* ---- skeletonize(voxel_graph=) (kimimaro/intake.py:66,162,174-183; utility.py:73-75).  PARITY UNPINNED: cc3d and edt are
 * third-party packages whose sources are absent from the reference tree.
 * kh_ccl26_graph replaces cc3d.color_connectivity_graph(voxel_graph, connectivity=26) followed by `cc_labels *= all_labels > 0`:
 * two foreground voxels are joined iff they are 26-neighbours and the graph word (cc3d's bit layout, u32 per voxel) of the later
 * one in the raster allows the step to the earlier one.  Arguments and numbering as kh_ccl26.  Also unpinned: it never links two
 * foreground voxels through background voxels, which color_connectivity_graph(graph) * (labels > 0) can (the mask comes after the
 * components there).  A component may hold several labels: `representative` is its first voxel, the host names it by the label at
 * its last run start in the raster (skeletontricks.get_mapping).
 * kh_edt_graph_cells / kh_edt_graph_sample are the two ends of edt.edt(labels, voxel_graph=): cells (u8 [2sx, 2sy, 2sz], F order)
 * receives the doubled image -- voxel (x, y, z) at cell (2x, 2y, 2z); the cell towards +x / +y / +z is foreground iff the voxel is
 * and bit 0 / 2 / 4 of its graph word is set (without black_border: also behind the last voxel of an axis); the other cells of the
 * voxel's 2 x 2 x 2 block follow the voxel -- on which the caller runs kh_edt(label_bytes = 1) with HALF the voxel pitch;
 * kh_edt_graph_sample reads that transform back at the voxel cells.  8 * nvox < 2^32.                                          */
int kh_ccl26_graph(const void* labels, int label_bytes, const uint32_t* graph, int64_t sx, int64_t sy, int64_t sz,
                   uint32_t* parent, uint32_t* chunk_counts, uint32_t* out, uint32_t* representative, uint32_t* ncomponents,
                   uint16_t* out16, void* stream);
int kh_edt_graph_cells(const void* labels, int label_bytes, const uint32_t* graph, int64_t sx, int64_t sy, int64_t sz,
                       int black_border, uint8_t* cells, void* stream);
int kh_edt_graph_sample(const float* fine, int64_t sx, int64_t sy, int64_t sz, float* out, void* stream);

/* ---- the graph itself: cc3d.voxel_connectivity_graph(labels, connectivity), which the reference's docstring names as the source of
 * skeletonize's voxel_graph (kimimaro/intake.py:113-117), extended by a list of label pairs (csrc/graph.hip).
 * PARITY UNPINNED: cc3d's source is absent from the reference tree; the word is DEFINED here.
 * graph[v] (u32 per voxel, F order) in cc3d's bit layout -- the inverse of kh_apply_voxel_graph's reading: bit 0 +x, 1 -x, 2 +y,
 * 3 -y, 4 +z, 5 -z, 6..9 the xy edges, 10..13 the edges towards +z, 14..17 towards -z, 18..21 the +z corners, 22..25 the -z ones.
 * The bit of a step is set iff (1) the step is one of the `connectivity` neighbours: 6 = bits 0..5, 18 = bits 0..17, 26 = all;
 * (2) the neighbour lies inside the array; (3) the two label values a, b are equal -- background included, 0 == 0 -- or the
 * unordered pair {a, b} is a row of `pairs`.  Bits 26..31 are clear.
 * labels: 1, 2, 4 or 8 bytes each, compared at full width as bit patterns.
 * pairs: npairs rows of two u64 (lo, hi), lo < hi, neither 0, sorted lexicographically, unique; NULL or npairs == 0: none.  The
 * relation is NOT transitive: {a, b} and {b, c} do not connect a to c.  Up to KH_GRAPH_LDS_PAIRS rows are searched in LDS, more in
 * global memory.  sx*sy*sz < 2^32, every extent and npairs < 2^31.  KH_EINVAL for another connectivity or label_bytes, a null
 * pointer, a non-positive extent.                                                                                                 */
#define KH_GRAPH_LDS_PAIRS 2048
int kh_voxel_graph(const void* labels, int label_bytes, int64_t sx, int64_t sy, int64_t sz, int connectivity,
                   const uint64_t* pairs, int64_t npairs, uint32_t* graph, void* stream);

/* ---- f3: binary hole filling, replaces fill_voids.fill(img, in_place=True, return_fill_count=True) as
 * called at kimimaro/trace.py:109 (third-party, source absent): a background voxel (mask == 0) stays
 * background iff a 6-connected background path joins it to a face of the array.  mask/out: u8 [nvox]
 * (out may not alias mask); parent: u32 [nvox] scratch; open: u8 [nvox] scratch; *filled (device i64) =
 * number of voxels that changed.                                                                    */
int kh_fill_voids(const uint8_t* mask, int64_t sx, int64_t sy, int64_t sz, uint32_t* parent, uint8_t* open,
                  uint8_t* out, int64_t* filled, void* stream);
/* the same for an array of `ndim` (1..3) dimensions, the axes beyond it having extent 1: they are not axes and have no faces -- the
 * border of a 2-D image is its outline (fill_voids.fill on the six faces of a crop, kimimaro/intake.py:655-666, fix_avocados).
 * kh_fill_voids == kh_fill_voids_nd(ndim = 3).                                                                      */
int kh_fill_voids_nd(const uint8_t* mask, int ndim, int64_t sx, int64_t sy, int64_t sz, uint32_t* parent, uint8_t* open,
                     uint8_t* out, int64_t* filled, void* stream);

/* ---- kimimaro.intake.fill_all_holes (kimimaro/intake.py:747-795): the holes of EVERY label in one pass over the volume
 * (csrc/ccl.hip).  hole(L) = the union of the 6-connected components of {v : labels[v] != L} that own no voxel on a
 * face of the array -- what fill_voids.fill paints on L's bounding box.  A REGION is a 6-connected component of equal value, 0
 * included; hole(L) is a union of regions, so the volume is read for the regions, their table and their adjacency only.
 * labels: u8/u16/u32/u64 [sx,sy,sz] (label_bytes 1, 2, 4 or 8), fewer than 2^32 - 1 voxels.
 * kh_regions6: region (u32 [nvox]) = ids 1..R by first appearance in the raster, *nregions (device u32) = R, representative
 *   (u32 [nvox + 1]): [r] = smallest linear index of region r; parent (u32 [nvox]), chunk_counts (u32 [ceil(nvox / 1024)]): scratch.
 * kh_region_table: value (u64 [R + 1]) = the label a region carries, count (u32 [R + 1]) = its voxels, face (u8 [R + 1]) = 1 iff
 *   it owns a voxel on a face of the array; entry 0 is 0.  ndim as in kh_fill_voids_nd: an axis beyond it (extent 1) has no faces;
 *   an axis of extent 1 WITHIN ndim puts every voxel on a face.
 * kh_region_pairs: table (u64 [capacity], capacity a power of two >= 64; set by the call) = an open-addressing hash set of the
 *   unordered pairs of regions that share a voxel face, key = smaller id << 32 | larger id, 0 = empty slot, in no particular order;
 *   state (device u32 [2], set by the call): [0] = keys in the table, [1] != 0: the table was too small and holds a PART of the
 *   set -- call again with a larger one (memory is bounded by the capacity, not by the number of faces).
 * kh_region_apply: labels[v] = owner[region[v]] where that is non-zero (owner: u64 [R + 1]), in place.
 * kh_region_table_box: kh_region_table for a label array that is a box of a dataset.  dataset_faces names the faces
 *   of the array that are faces of the DATASET (bit 0 x == 0, bit 1 x == sx-1, bits 2, 3 the y faces, 4, 5 the z faces; what
 *   kh_cross_sections_box derives from o, b and d): face = 1 iff the region owns a voxel on one of those.  value and count are
 *   kh_region_table's; dataset_faces == 63 gives its face flags too, 0 gives none.  More than six bits are a bad argument.
 * kh_region_seam_pairs: low, high (u32 [m], 1 <= m < 2^32) are two planes of region ids that face each other across
 *   a cut, low[p] the neighbour of high[p]; the distinct keys low[p] << 32 | high[p] are put into `table` with kh_region_pairs'
 *   layout, capacity rule, `state` and overflow report (call again with a larger table).  The caller numbers the regions so that
 *   low[p] < high[p]; no labels are read: whether a pair joins two pieces of one region (equal value) or two adjacent regions is
 *   the caller's to tell.
 * kh_region_apply_box: kh_region_apply for a core of a dataset.  region (u32 [nvox]) holds the DATASET's
 *   provisional ids; the core owns base + 1 .. base + nregions (nregions >= 1, base + nregions <= 2^32 - 1) and owner (u64
 *   [nregions + 1], entry 0 unused) is the table of those.  Per voxel r = region[v] - base in u32 arithmetic: for r in 1..nregions
 *   labels[v] = owner[r] where that is non-zero; for any other r the voxel is left alone and owner is NOT read.  state (device u64
 *   [2], set by the call): [0] = voxels painted, [1] = voxels whose id lay outside the core's range (a stale region store).        */
int kh_regions6(const void* labels, int label_bytes, int64_t sx, int64_t sy, int64_t sz, uint32_t* parent, uint32_t* chunk_counts,
                uint32_t* region, uint32_t* representative, uint32_t* nregions, void* stream);
int kh_region_table(const void* labels, int label_bytes, const uint32_t* region, const uint32_t* representative, int64_t nregions,
                    int ndim, int64_t sx, int64_t sy, int64_t sz, uint64_t* value, uint32_t* count, uint8_t* face, void* stream);
int kh_region_pairs(const uint32_t* region, int64_t sx, int64_t sy, int64_t sz, uint64_t* table, int64_t capacity, uint32_t* state,
                    void* stream);
int kh_region_apply(const uint32_t* region, const uint64_t* owner, void* labels, int label_bytes, int64_t nvox, void* stream);
int kh_region_table_box(const void* labels, int label_bytes, const uint32_t* region, const uint32_t* representative, int64_t nregions,
                        int ndim, int64_t sx, int64_t sy, int64_t sz, uint32_t dataset_faces, uint64_t* value, uint32_t* count,
                        uint8_t* face, void* stream);
int kh_region_seam_pairs(const uint32_t* low, const uint32_t* high, int64_t m, uint64_t* table, int64_t capacity, uint32_t* state,
                         void* stream);
int kh_region_apply_box(const uint32_t* region, uint32_t base, int64_t nregions, const uint64_t* owner, void* labels, int label_bytes,
                        int64_t nvox, uint64_t* state, void* stream);
/* host (no GPU needed): who fills what, on the region graph.  value / count / face: the table of kh_region_table ([nregions + 1]);
 * pairs: u64 [npairs], the non-empty keys of kh_region_pairs in any order, each unordered pair once.  The labels (non-zero values,
 * compared as unsigned words) are gone through in ascending order with a dead set, as the reference's loop does:
 *   a label that is not dead and has hole(L) != {} adds |hole(L)| to *filled, kills every label with a region in hole(L) and
 *   becomes the owner of hole(L)'s regions (a later owner replaces an earlier one; *filled counts such a voxel twice).
 * hole(L) = the regions that no path of the graph joins to a face-owning region once L's regions are removed.
 * owner (u64 [nregions + 1]) = the label a region ends up with, 0 = it keeps its own; label_value / label_state ([nregions],
 * the first `return value` entries are set) = the distinct labels ascending and KH_HOLES_* bits for each.
 * Returns the number of labels, -1 on allocation failure, -2 on bad arguments (null pointer, a pair outside 1..nregions).      */
#define KH_HOLES_PROCESSED 1   /* the label was alive at its turn: its holes were looked for          */
#define KH_HOLES_FILLED 2      /* ... and it had some                                               */
#define KH_HOLES_KILLED 4      /* a region of the label lies in a hole that was filled (at any time) */
int64_t kh_host_resolve_holes(int64_t nregions, const uint64_t* value, const uint32_t* count, const uint8_t* face, int64_t npairs,
                              const uint64_t* pairs, uint64_t* owner, uint64_t* label_value, uint8_t* label_state, int64_t* filled);
/* host (no GPU needed): hole(L) itself for each of n_labels wanted label words (labels: u64, any order, duplicates allowed, 0 is a
 * value like any other), on the graph as given: no dead set, no order among the labels, so a region may be listed for several
 * labels (a core inside shell B inside shell A lies in hole(A) and in hole(B)).  nregions / value / face / npairs / pairs as above.
 * offsets (u64 [n_labels + 1]) is always set; regions (u32 [capacity]) receives for label i, at offsets[i] .. offsets[i + 1], the ids
 * of hole(labels[i])'s regions, ascending; a label that does not occur or has no holes gets an empty range.
 * Returns the total offsets[n_labels]; when it exceeds `capacity` NOTHING was written to regions: call again with a larger one
 * (capacity 0 with regions == NULL asks for the size).  -1 on allocation failure, -2 on bad arguments (as above).
 * These lists, expanded per item, are what kh_cross_sections_filled reads.                                                       */
int64_t kh_host_enclosed_regions(int64_t nregions, const uint64_t* value, const uint8_t* face, int64_t npairs, const uint64_t* pairs,
                                 int64_t n_labels, const uint64_t* labels, uint64_t* offsets, uint32_t* regions, int64_t capacity);

/* ---- kimimaro.oversegment (kimimaro/utility.py:562-644) / dijkstra3d.euclidean_distance_field(..., return_feature_map=True) from
 * MANY sources: the geodesic Voronoi diagram of seed voxels inside every label, over the whole volume at once (csrc/feature.hip,
 * DESIGN.md 3.10).  PARITY UNPINNED (dijkstra3d and fastremap are absent from the reference tree); the result is defined order free:
 *   d(v) = the unique fixpoint of  d(v) = min(0 if v is a seed, min over same-label 26-neighbours u of fl(d(u) + w(u, v)))  in f32,
 *          w as in kh_edf_batch (make_geometry); +inf where no seed reaches;
 *   f(v) = at a seed the smallest number seeded there, elsewhere min f(u) over the neighbours u with fl(d(u) + w(u, v)) == d(v).
 * nbrmask: the words of kh_neighbor_mask.  All volumes < 2^32 voxels, numbers 1 .. 2^32 - 2.
 * kh_geodesic_seed: dist = +inf and feature = 0xFFFFFFFF ("none") for all nvox voxels, then for every seed s whose voxel
 *   seed_voxel[s] carries the label seed_label[s] (!= 0): dist = 0, feature = min(feature, seed_number[s]).
 * kh_geodesic_relax / kh_feature_relax: `sweeps` pull sweeps in place, each a launch of its own on `stream`; a sweep visits a brick
 *   of KH_BRICK_X x KH_BRICK_Y x KH_BRICK_Z voxels only if it or one of its 26 brick neighbours changed in the sweep before.
 *   brick_dirty: 3 planes of one byte per brick (x fastest), used round robin -- sweep number s reads plane s % 3, writes plane
 *   (s + 1) % 3 and clears plane (s + 2) % 3; before the first sweep of a phase the caller sets plane first_sweep % 3 to 1 and the
 *   other two to 0, and passes first_sweep = the number of sweeps of the phase already run.  changed: device u32 [2 * sweeps], set by
 *   the call: [2 j] = bricks that changed in the call's sweep j, [2 j + 1] = bricks it visited.  The phase is at its fixpoint when
 *   a sweep changed nothing -- the only valid end of the loop; the caller reads `changed` once per call.
 *   kh_feature_relax must run on the FINAL dist (it does not write it).
 * kh_first_appearance: first_of_number[n] (u32 [nnumbers + 1], set by the call) = smallest linear index whose feature is n,
 *   0xFFFFFFFF when n owns no voxel; features 0 and > nnumbers are ignored.
 * kh_remap_u32: feature[v] = map[feature[v]] (map: u32 [nnumbers + 1]); features 0 and > nnumbers (the "none" word) become 0.   */
#define KH_BRICK_X 64
#define KH_BRICK_Y 4
#define KH_BRICK_Z 4
int kh_geodesic_seed(const uint32_t* seed_voxel, const uint32_t* seed_number, int64_t nseeds, const void* labels, int label_bytes,
                     const uint32_t* seed_label, int64_t nvox, float* dist, uint32_t* feature, void* stream);
int kh_geodesic_relax(const uint32_t* nbrmask, int64_t sx, int64_t sy, int64_t sz, float wx, float wy, float wz, float* dist,
                      uint8_t* brick_dirty, uint32_t* changed, int sweeps, int64_t first_sweep, void* stream);
int kh_feature_relax(const uint32_t* nbrmask, int64_t sx, int64_t sy, int64_t sz, float wx, float wy, float wz, const float* dist,
                     uint32_t* feature, uint8_t* brick_dirty, uint32_t* changed, int sweeps, int64_t first_sweep, void* stream);
int kh_first_appearance(const uint32_t* feature, int64_t nvox, int64_t nnumbers, uint32_t* first_of_number, void* stream);
int kh_remap_u32(uint32_t* feature, const uint32_t* map, int64_t nnumbers, int64_t nvox, void* stream);

/* ---- the same labels for a dataset that is relaxed box by box (kimimaro_amd.post.oversegment_chunked).  A box is
 * bx x by x bz voxels (x fastest, < 2^32 in all); its CORE is [core_lo, core_hi) in box-local voxels, half open; core_lo, core_hi
 * and origin are HOST arrays of three int64.
 * kh_geodesic_seed_at: kh_geodesic_seed without the init pass -- dist and feature hold what the stores gave; for every seed whose
 *   voxel carries its label: dist = 0, feature = min(feature, seed_number[s]).  dist or feature may be NULL: that array is left out.
 * kh_box_shell_diff: one pass over the core that compares the 32-bit words old[v] and now[v] (distances or features).  out: device
 *   u32 [3], set by the call: [0] bit k = a core voxel changed that lies in the core's outermost layer towards direction k, k in
 *   kh_neighbor_mask's order (dz, dy, dx from -1 to 1, x fastest, the centre left out) -- a corner voxel sets its corner, its three
 *   edges and its three faces, and on an axis where the core is one voxel thick a voxel lies in both layers; [1] the core voxels
 *   that changed; [2] the largest word of now[] over the core below 0x7F800000 (the largest finite non-negative f32 as bits), 0
 *   when there is none.  Voxels of the box outside the core are not read.
 * kh_first_appearance_box: first_of_number[n] (u64 [nnumbers + 1]) = min(itself, the smallest DATASET raster index
 *   (origin + v)_x + SX * ((origin + v)_y + SY * (origin + v)_z) of a core voxel v whose feature is n); features 0 and > nnumbers
 *   are ignored.  The table is NOT cleared: it accumulates over the boxes of a dataset, the caller sets it to all ones once.       */
int kh_geodesic_seed_at(const uint32_t* seed_voxel, const uint32_t* seed_number, int64_t nseeds, const void* labels, int label_bytes,
                        const uint32_t* seed_label, int64_t nvox, float* dist, uint32_t* feature, void* stream);
int kh_box_shell_diff(const uint32_t* old, const uint32_t* now, int64_t bx, int64_t by, int64_t bz, const int64_t* core_lo,
                      const int64_t* core_hi, uint32_t* out, void* stream);
int kh_first_appearance_box(const uint32_t* feature, int64_t bx, int64_t by, int64_t bz, const int64_t* core_lo,
                            const int64_t* core_hi, const int64_t* origin, int64_t SX, int64_t SY, int64_t nnumbers,
                            uint64_t* first_of_number, void* stream);

/* ---- kimimaro.synapses_to_targets (kimimaro/intake.py:706-745): the voxel of a label nearest to a centroid, for all labels and
 * centroids in two passes over the volume (csrc/points.hip).
 * labels: u8/u16/u32/u64 [sx,sy,sz] (label_bytes 1, 2, 4 or 8).  table: u64 [nlabels], the distinct labels asked for as the unsigned
 * words the volume holds, ascending; query_start: u32 [nlabels + 1], the queries of table[k] are [query_start[k], query_start[k+1]);
 * centroids: f64 [nqueries, 3] in voxel coordinates.  Both outputs are u64 [nqueries], set by the call:
 *   best_distance[q] = bits of  d = sqrt(((x-cx)^2 + (y-cy)^2) + (z-cz)^2)  in float64, every operation rounded (what scipy's cdist
 *                      computes), minimised over the voxels of the query's label;
 *   best_voxel[q]    = x*sy*sz + y*sz + z (the C-order index: np.nonzero enumerates in C order whatever the memory layout) of the
 *                      first such voxel in that order -- np.argmin's choice among equal distances.
 * Both are ~0 ("none") for a query whose label does not occur.  Centroids must be finite.                                       */
int kh_nearest_label_voxels(const void* labels, int label_bytes, int64_t sx, int64_t sy, int64_t sz,
                            const uint64_t* table, const uint32_t* query_start, int64_t nlabels, const double* centroids,
                            int64_t nqueries, uint64_t* best_distance, uint64_t* best_voxel, void* stream);

/* ---- the same for a dataset that is never resident as a whole: ONE visit of ONE box, on running per-query results that live on
 * the device across visits (csrc/points.hip).  labels: the box, [ex,ey,ez] Fortran ordered, its low corner at
 * (lox, loy, loz) of a dataset whose y and z extents are dsy, dsz.  table / query_start / centroids as above, for the nqueries queries
 * of THIS visit, centroids in dataset coordinates; query_index: u32 [nqueries], the row g of each listed query in the running
 * arrays best_distance / best_voxel (distinct rows), which the caller sets to ~0 once and which are never filled here.  On return,
 * for every listed query, (best_distance[g], best_voxel[g]) is the lexicographic minimum of the pair that came in and, over the
 * box's voxels of the query's label, (bits of d, C-order index in the DATASET ((lox+x)*dsy + (loy+y))*dsz + (loz+z), 64 bit), d as
 * above from dx = (double)(lox + x) - cx and likewise y, z.  A box that lowers best_distance[g] thereby discards the best_voxel[g]
 * earlier boxes found; with an equal distance the earlier index stays and competes.  Rows not listed are not touched.
 * scratch: u64 [nqueries].  Everything is stream-ordered, no host synchronisation, nothing is allocated.                          */
int kh_nearest_label_voxels_box(const void* labels, int label_bytes, int64_t ex, int64_t ey, int64_t ez,
                                int64_t lox, int64_t loy, int64_t loz, int64_t dsy, int64_t dsz,
                                const uint64_t* table, const uint32_t* query_start, int64_t nlabels, const double* centroids,
                                const uint32_t* query_index, int64_t nqueries, uint64_t* best_distance, uint64_t* best_voxel,
                                uint64_t* scratch, void* stream);

/* ---- skeletontricks.extract_edges_from_binary_image (skeletontricks.pyx:1047-1086 -> skeletontricks.hpp:399-495) on the words of
 * kh_neighbor_mask of the image (foreground = one label): every unordered pair of foreground voxels that are neighbours in one of
 * `directions` (bit i = direction i of that mask: 0x3F connectivity 6, 0x3FFFF 18, 0x3FFFFFF 26) is an edge, every voxel on an edge a
 * vertex.  The reference's numbering is the iteration order of an unordered_set; here it is canonical: vertices by
 * ascending index x + sx*(y + sy*z), edges (a, b) with a < b sorted by a, then b.
 * kh_binary_edge_count: is_vertex / n_owned (u8 [nvox]) = whether the voxel is a vertex / how many edges lead from it to LATER
 *   voxels; totals (device u64 [2], set by the call) = number of vertices, number of edges.
 * kh_binary_edge_emit: vertex_scan / edge_scan (i64 [nvox]) = the caller's INCLUSIVE prefix sums of is_vertex / n_owned;
 *   vertices u32 [totals[0], 3] = (x, y, z) rows, edges u32 [totals[1], 2].  Fewer than 2^32 vertices.                           */
int kh_binary_edge_count(const uint32_t* nbrmask, int64_t nvox, uint32_t directions, uint8_t* is_vertex, uint8_t* n_owned,
                         uint64_t* totals, void* stream);
int kh_binary_edge_emit(const uint32_t* nbrmask, int64_t sx, int64_t sy, int64_t sz, uint32_t directions,
                        const int64_t* vertex_scan, const int64_t* edge_scan, uint32_t* vertices, uint32_t* edges, void* stream);

/* ---- kimimaro.cross_sectional_area's inner call (xs3d.cross_sectional_area at kimimaro/utility.py:315-320; the package is absent
 * from the reference tree: PARITY UNPINNED, the section is DEFINED in DESIGN.md 3.12) for a batch of items in one launch
 * (csrc/section.hip).  Item i: the seed voxel seed_lin[i] = x + sx*(y + sy*z) (any value >= sx*sy*sz: outside the volume), the
 * label want_label[i] its section stays in, the normal normals[3i .. 3i+2] (float64, any length).  With p the seed, a the anisotropy:
 *   voxel c is CUT iff |d| < h,  d = ((nx*ax)*(cx-px) + (ny*ay)*(cy-py)) + (nz*az)*(cz-pz),  h = 0.5*((|nx|*ax + |ny|*ay) + |nz|*az),
 *   float64, every operation rounded; the section is the 26-connected component of p among the cut voxels that carry the label.
 * area[i]    = sum over the section of area(plane /\ voxel box) in physical units: float64 per voxel, summed in a 64-bit fixed point
 *              (independent of the order of arrival, the same bits on every run), rounded to float32 at the end;
 * contact[i] = bit 0 some section voxel has x == 0, bit 1 x == sx-1, bit 2 y == 0, bit 3 y == sy-1, bit 4 z == 0, bit 5 z == sz-1;
 * voxels[i]  = the number of voxels of the section.
 * All three are 0 for an empty section: a seed outside the volume or off its label, a normal with a non-finite component or all zero.
 * labels: u8/u16/u32 [sx,sy,sz] (label_bytes 1, 2, 4), fewer than 2^32 - 1 voxels.  scratch: device memory of at least
 * kh_cross_sections_scratch_bytes(sx, sy, sz, 1) bytes, 8-byte aligned; the launch uses as many waves (at most n_items) as it holds.
 * It needs no initialisation; afterwards its second u64 word is non-zero if a queue overflowed (a defect, not a size limit:
 * the bytes per wave cover the largest section the volume admits).
 * kh_cross_sections_scratch_bytes: the bytes for n_waves concurrent waves, -1 for extents the call refuses.                     */
int kh_cross_sections(const void* labels, int label_bytes, int64_t sx, int64_t sy, int64_t sz, double ax, double ay, double az,
                      int64_t n_items, const uint32_t* seed_lin, const uint32_t* want_label, const double* normals, float* area,
                      uint8_t* contact, uint32_t* voxels, void* scratch, int64_t scratch_bytes, void* stream);
int64_t kh_cross_sections_scratch_bytes(int64_t sx, int64_t sy, int64_t sz, int64_t n_waves);
/* kimimaro.cross_sectional_area(fill_holes=True): the same sections of filled(L) = {labels == L} u hole(L) (hole(L) as defined at
 * kh_regions6, ndim 3) -- "carries the label" becomes "lies in filled(label)", for the seed too: a seed in a hole voxel is valid.
 * region: u32 [nvox], kh_regions6's output for the same label array; item i's holes are the region ids
 * hole_regions[hole_begin[i] .. hole_begin[i] + hole_count[i]), ASCENDING (kh_host_enclosed_regions' list of the item's label; the
 * caller expands label -> item).  An item with hole_count 0 reads no region and gives kh_cross_sections' outputs bit for bit.
 * Everything else, the scratch and kh_cross_sections_scratch_bytes included, as kh_cross_sections; a null region / hole_begin /
 * hole_count / hole_regions with n_items > 0 is a bad argument.                                                                 */
int kh_cross_sections_filled(const void* labels, int label_bytes, int64_t sx, int64_t sy, int64_t sz, double ax, double ay, double az,
                             int64_t n_items, const uint32_t* seed_lin, const uint32_t* want_label, const double* normals,
                             const uint32_t* region, const uint32_t* hole_begin, const uint32_t* hole_count,
                             const uint32_t* hole_regions, float* area, uint8_t* contact, uint32_t* voxels, void* scratch,
                             int64_t scratch_bytes, void* stream);
/* kimimaro_amd.cross_sectional_area_chunked: kh_cross_sections for a label array that is the box [o, o + b) of a
 * dataset of extents d, b = (sx, sy, sz); o and d are 64-bit and the dataset may hold 2^32 voxels or more, only the box obeys the
 * limits of kh_cross_sections.  seed_lin are linear indices IN THE BOX.  The box must lie inside the dataset.
 * contact[i] refers to the DATASET: bit 0 some section voxel has dataset coordinate x + ox == 0, bit 1 x + ox == dx-1, and so on.
 * clip[i]    the same bit layout for the faces of the BOX that are no faces of the dataset: bit 0 x == 0 && ox > 0, bit 1
 *            x == sx-1 && ox + sx < dx, ...  clip == 0: every neighbour of every section voxel lay inside the box, the section is the
 *            voxel set a launch on the whole dataset finds.  Otherwise it is a subset of that and area / voxels are lower bounds.
 * The fixed point of the sum is 2^(62 - fixed_exponent), the caller's: kh_cross_sections_fixed_exponent of the DATASET makes the
 * integer sum of a section with clip == 0 the one kh_cross_sections computes on the whole dataset, and area bit-equal.  It must not
 * be smaller than the box's own exponent (bad argument), which keeps every sum below 2^62.
 * scratch: kh_cross_sections_scratch_bytes of the BOX's extents.  Everything else as kh_cross_sections; clip is 0 for an empty
 * section.
 * kh_cross_sections_filled_box: both at once, kh_cross_sections_box's arguments and kh_cross_sections_filled's
 * region / hole_begin / hole_count / hole_regions.  region (u32 [sx * sy * sz]) holds, for the voxels of the box, region ids of the
 * DATASET's region graph in any numbering the lists share (kimimaro_amd.post.region_graph_chunked's provisional ids); an item's list
 * names, ascending, the regions of hole(label) taken on the dataset that have voxels in the box.  An item with hole_count 0 gives
 * kh_cross_sections_box's outputs bit for bit, an item with clip == 0 what kh_cross_sections_filled gives on the whole dataset.
 * kh_cross_sections_fixed_exponent (host, no device needed): the e kh_cross_sections uses for a volume of extents (dx, dy, dz), each
 * below 2^31, with the anisotropy (ax, ay, az): the binary exponent of ((ax*ay + ay*az) + ax*az) * min(4 * largest face, dx*dy*dz),
 * the face exact in 64 bits, the other products float64.  INT32_MIN for extents or an anisotropy the launches refuse, or a
 * bound that is not a positive finite float64.                                                                                   */
int kh_cross_sections_box(const void* labels, int label_bytes, int64_t sx, int64_t sy, int64_t sz, double ax, double ay, double az,
                          int64_t n_items, const uint32_t* seed_lin, const uint32_t* want_label, const double* normals, int64_t ox,
                          int64_t oy, int64_t oz, int64_t dx, int64_t dy, int64_t dz, int fixed_exponent, float* area,
                          uint8_t* contact, uint32_t* voxels, uint8_t* clip, void* scratch, int64_t scratch_bytes, void* stream);
int kh_cross_sections_filled_box(const void* labels, int label_bytes, int64_t sx, int64_t sy, int64_t sz, double ax, double ay,
                                 double az, int64_t n_items, const uint32_t* seed_lin, const uint32_t* want_label,
                                 const double* normals, const uint32_t* region, const uint32_t* hole_begin, const uint32_t* hole_count,
                                 const uint32_t* hole_regions, int64_t ox, int64_t oy, int64_t oz, int64_t dx, int64_t dy, int64_t dz,
                                 int fixed_exponent, float* area, uint8_t* contact, uint32_t* voxels, uint8_t* clip, void* scratch,
                                 int64_t scratch_bytes, void* stream);
int kh_cross_sections_fixed_exponent(int64_t dx, int64_t dy, int64_t dz, double ax, double ay, double az);
/* host: the membership test and the area of ONE voxel at offset (dx, dy, dz) from the seed, by the functions the kernel runs
 * (normal, anisotropy: f64 [3]).  Returns 1 if the voxel is cut; *offset = d, *half_width = h, *area = area(plane /\ box).      */
int kh_host_section_voxel(const double* normal, const double* anisotropy, int64_t dx, int64_t dy, int64_t dz, double* offset,
                          double* half_width, double* area);

/* ---- kh_ccl26 on HOST memory (used for the 2-D faces of fix_borders and as a cross-check),
 * restating cc3d.connected_components as called at kimimaro/utility.py:74-77.
 * Returns the number of components (ids 1..N by first appearance in F-order raster).   */
int64_t kh_host_ccl26(const void* labels, int label_bytes, int64_t sx, int64_t sy, int64_t sz,
                      uint32_t* out);

/* ---- row f2 (host side): skeletontricks.find_border_targets (skeletontricks.pyx:591-647 with
 * compute_centroids :528-588 and compute_tiebreaker_maxima :650-760) on HOST memory.
 * dt (f32) and cc (u32) are [sx,sy] Fortran ordered planes; for each component id with a maximum
 * out_xy[2*id..2*id+1] receives (x, y) and `order` the ids in dict-insertion order.
 * cc holds ids 0..nlab.  The caller sizes out_xy for 2 * (nlab + 1) floats -- the rows of id 0 and of ids
 * without a maximum are not written -- and `order` for nlab + 1 entries, of which at most nlab are written
 * (none when nlab is 0).
 * Returns the number of ids, -1 on allocation failure.                                  */
int64_t kh_host_find_border_targets(const float* dt, const uint32_t* cc, int64_t sx, int64_t sy,
                                    float wx, float wy, int64_t nlab, float* out_xy, int32_t* order);

/* ---- row a12 (host side): Skeleton.from_path per path + Skeleton.simple_merge + consolidate (kimimaro/trace.py:182-184) for
 * every component ("slot") of a result group in one call, outside the interpreter.  voff / loff [nslots+1]: first path vertex /
 * first path of every slot in locs (linear voxel indices x + sx (y + sy z), the paths of a slot back to back) / lens (vertices
 * per path); radii: the DBF at every path vertex.  Output, slot by slot: out_verts [N,3] = the slot's unique vertices that an
 * edge refers to, as voxel coordinates in f32, sorted lexicographically by (x, y, z) like np.unique(axis=0); out_radii [N] = the
 * radius of each vertex's first occurrence; out_edges [M,2] = rows (lo, hi), lo != hi, unique, sorted, indices local to the slot;
 * vstart / estart [nslots+1] = where every slot's vertices / edges start.  The caller sizes out_verts / out_radii for sum(lens)
 * vertices and out_edges for sum(lens) edges.  Returns N, -1 on allocation failure.                                             */
int64_t kh_host_consolidate_paths(int64_t nslots, const int64_t* voff, const int64_t* loff, const uint32_t* locs,
                                  const uint32_t* lens, const float* radii, int64_t sx, int64_t sy, int64_t sz,
                                  float* out_verts, float* out_radii, uint32_t* out_edges, int64_t* vstart, int64_t* estart);

/* ---- row a12 (host side): the merge of a label's components into one skeleton, kimimaro/intake.py:587-593
 * (Skeleton.simple_merge(...).consolidate() per original label) for ALL labels of a volume in one call, outside the
 * interpreter.  The components of a label are disjoint voxel sets whose vertices are sorted lexicographically by
 * (x, y, z) already (kimimaro_amd.intake.consolidate_paths_batch), so consolidate() is a re-sort on integer keys.
 * Parts are given label by label, in component order: part_of_label[l] .. part_of_label[l+1] are label l's parts;
 * vstart / estart [nparts+1]: first vertex / edge of every part in verts [N,3] (voxel coordinates as f32) / radii [N] /
 * edges [M,2] (indices local to the part).  Output, label by label at the same offsets: out_verts = sorted vertices
 * times (ax, ay, az) in f32 (intake.py:513), out_radii, out_edges [M,2] = rows (lo, hi) sorted lexicographically, indices
 * local to the LABEL.  Returns 0, -1 on allocation failure.                                                         */
int64_t kh_host_merge_components(int64_t nlabels, const int64_t* part_of_label, const int64_t* vstart, const int64_t* estart,
                                 const float* verts, const float* radii, const uint32_t* edges, int64_t sy, int64_t sz,
                                 float ax, float ay, float az, float* out_verts, float* out_radii, uint32_t* out_edges);

/* ---- row f4 on the device: the nearest vertex pairs between the parts of skeleton groups ------------------
 * replaces: the cKDTree queries of kimimaro/post.py:89-218 (join_close_components), which are repeated after every merge; here
 * one table of raw nearest pairs between all ORIGINAL parts determines the whole merge sequence (kh_host_join_plan below).
 * Parts: the components of the skeletons of a group, consolidated, the empty ones dropped; vertex k of a part is its row k.
 * Device inputs: xyz f32 [V,3], the vertices of all parts back to back; part_start u32 [P+1]; part_box f32 [P,6] = (min x, y, z,
 * max x, y, z) of every part; group_start u32 [G+1], indexing parts; bound2 f64 [G]; rec_start i64 [G+1] with
 * rec_start[g+1] - rec_start[g] = n_g * n_g for the n_g parts of group g, rec_start[G] = nrecords (at most 2^26: 1 GiB of tables).
 * Outputs, every cell written: rec_d2 [nrecords] (the bits of an f64) and rec_idx [nrecords,2] = (kt, kq); the cell of tree part
 * t and query part q of group g, both local to the group, is rec_start[g] + t * n_g + q.
 * Record R[t][q], t != q: the lexicographic minimum of (d2, kq, kt) over the vertices kq of q and kt of t, where
 * d2 = ((dx*dx + dy*dy) + dz*dz), dx = (double)xq - (double)xt, every operation rounded in f64, no FMA.  It is "none" exactly when
 * that minimal d2 >= bound2[g] (+inf allowed: nothing is none), stored as d2 = the bits of +inf and both indices 0xFFFFFFFF; so is
 * the diagonal.  No record crosses groups.  Pairs whose boxes are at least the bound apart are not visited.  Asynchronous on
 * `stream`; the library allocates nothing.                                                                                     */
int kh_part_gaps(const float* xyz, const uint32_t* part_start, const float* part_box, const uint32_t* group_start,
                 const double* bound2, const int64_t* rec_start, int64_t ngroups, int64_t nrecords, uint64_t* rec_d2,
                 uint32_t* rec_idx, void* stream);

/* ---- row f4 on the device, the broad phase in front of kh_part_gaps: the sets of parts of a group that are
 * connected through near pairs.  Parts t != q of one group g are NEAR iff low(t, q) < bound2[g], where low = (gx*gx + gy*gy) + gz*gz
 * and g. is the distance of the two parts' intervals along an axis (0 where they overlap), taken on the part_box floats widened to
 * f64, every operation rounded in f64, no FMA: the very quantity on which kh_part_gaps declares a pair "none" without a look at
 * its vertices (one device function serves both), so a pair that has a record is near.  cluster[p] = the smallest part index, in
 * the numbering of part_box, among the parts connected to p through near pairs; a part alone is its own cluster, parts of
 * different groups are never connected, with bound2 = +inf a group is one cluster.  A function of the boxes alone.
 * Device inputs: part_box f32 [P,6], group_start u32 [G+1], bound2 f64 [G] as for kh_part_gaps; order u32 [P]: at the positions
 * [group_start[g], group_start[g+1]) the parts of group g sorted by part_box[.][axis] ascending, ties by part index; axis 0, 1 or 2.
 * The result does not depend on the axis.  An entry of order outside its group is skipped (its part then joins nothing by it).
 * Output: cluster u32 [P], every word written; it doubles as the parent array of the union-find, so the library allocates
 * nothing and no list of pairs is stored.  Three launches (identity, unions, flatten), asynchronous on `stream`.
 * Cost: a part is tested against the later parts of `order` up to the first whose low end lies the bound beyond its high end:
 * at worst n_g^2 / 2 box tests for a group whose boxes all span the axis.  0 <= G, P < 2^31.                                     */
int kh_part_clusters(const float* part_box, const uint32_t* group_start, const double* bound2, const uint32_t* order,
                     int64_t ngroups, int64_t nparts, int axis, uint32_t* cluster, void* stream);

/* ---- row f4 (host side, no GPU): the merge plan of join_close_components (kimimaro/post.py:89-218) for ONE group, reading only
 * the table of its nparts parts: rec_d2 [nparts*nparts], rec_idx [nparts*nparts,2] as above; part_size [nparts]; radii = the
 * parts' vertex radii back to back; radius = the value the search ends up with (with restrict_by_radius: twice the largest
 * vertex radius, computed by the caller, who derived bound2 = (radius + 0.000001)^2 from it).
 * A cluster is an ordered list of (original part, vertex offset); at first every part is one.  The gap of cluster A as tree and
 * cluster B as query is the lexicographic minimum of (d2, kq + offset_B, kt + offset_A) over the records R[a][b] of their members
 * that are not none; d = sqrt(d2); with restrict_by_radius a d above the float32 sum of the two vertices' radii counts as
 * infinite; the key is (float)d.  Repeatedly: the smallest (key, i, j), i < j in the current numbering -- the fused cluster
 * first, the rest in their previous order, the earlier cluster being the tree -- is merged (A's members, then B's) unless the key
 * is not finite or (double)key > radius, which ends the plan.  Each merge writes one edge (tree vertex, query vertex) in the
 * numbering of the concatenated ORIGINAL parts; edges has room for (nparts - 1) * 2 entries.
 * Returns the number of edges; -1 for a bad argument (null pointer, nparts < 0, more than 2^32 - 1 vertices, an index outside
 * its part in a record that is not none), -2 on allocation failure.                                                            */
int64_t kh_host_join_plan(int64_t nparts, const uint32_t* part_size, const uint64_t* rec_d2, const uint32_t* rec_idx,
                          const float* radii, double radius, int restrict_by_radius, uint32_t* edges);

/* ---- row f4 on the device: the skeletons of a call packed back to back, "the forest"  ------------------------
 * replaces: the Python loops over the vertices of one skeleton at a time in Skeleton.components, remove_dust, remove_loops and
 * remove_ticks (kimimaro/post.py:222-362).  Vertices and edges of all skeletons are numbered call-wide; no edge joins two
 * skeletons.  0 <= nverts, nedges < 2^31.  All three are asynchronous on `stream`, and the library allocates nothing.
 *
 * kh_forest_components: edges u32 [nedges,2] -> comp u32 [nverts], every word written: the smallest vertex connected to v (a
 * vertex without an edge is its own).  comp doubles as the parent array of the union-find: three launches (identity, unions,
 * flatten).  A function of the edge SET: the order of the rows does not matter.  A row that names a vertex >= nverts is skipped. */
int kh_forest_components(const uint32_t* edges, int64_t nverts, int64_t nedges, uint32_t* comp, void* stream);

/* kh_forest_measure: xyz f32 [nverts,3], edges, comp as above -> per component, AT ITS ROOT v = comp[v] (every other word 0):
 * nv[v] its vertices, ne[v] its edges, cable[v] (f64) the sum of its edges' float32 lengths widened to f64, each length
 * sqrtf(((dx*dx) + (dy*dy)) + (dz*dz)) of the float32 differences, correctly rounded, no FMA (Skeleton.cable_length's terms; the
 * ORDER of the f64 sum is not fixed); and degree[v] for every vertex.  All four arrays have nverts words and all are written.
 * Atomics: one 32-bit add per edge end (degree) and one add per run of equal roots among the 64 edges (vertices) of a wave.      */
int kh_forest_measure(const float* xyz, const uint32_t* edges, const uint32_t* comp, int64_t nverts, int64_t nedges, double* cable,
                      uint32_t* nv, uint32_t* ne, uint32_t* degree, void* stream);

/* kh_forest_ticks: the tick removal of kimimaro/post.py:262-362 for every listed component at once, operation by operation
 * (DESIGN.md 3.22 states it).  Adjacency as CSR: row_start u32 [nverts+1], nbr u32 [nslots] (nslots = 2 * edges), the neighbours of
 * a vertex ascending.  A component is listed by its CRITICAL vertices (degree 1 or >= 3), ascending: crit u32 [ncrit], those of
 * component c at [crit_start[c], crit_start[c+1]), crit_start u32 [ncomps+1].  Only trees with at least one vertex of degree >= 3
 * may be listed (the caller checks ne == nv - 1); a component with fewer than two critical vertices is left alone.
 * Output: alive u8 [nslots], every word written: 0 for both slots of every edge on a removed path, 1 elsewhere.
 * Superedge lengths are accumulated in float32 from the end nearer the component's smallest terminal, outward, then widened; fused
 * lengths are f64 sums; the next tick is the removable superedge of smallest (length, larger end, smaller end); `threshold` is f64.
 * Scratch, sized by the caller: slot_scratch u32 [4*nslots], arity i32 [nverts], rec_scratch u32 [5*ncrit], rec_len f64 [ncrit],
 * rec_flag u8 [ncrit].  One wave per component, no atomics.                                                                     */
int kh_forest_ticks(const float* xyz, const uint32_t* row_start, const uint32_t* nbr, const uint32_t* crit, const uint32_t* crit_start,
                    int64_t nverts, int64_t nslots, int64_t ncrit, int64_t ncomps, double threshold, uint32_t* slot_scratch,
                    int32_t* arity, uint32_t* rec_scratch, double* rec_len, uint8_t* rec_flag, uint8_t* alive, void* stream);

/* ---- the path walk on the forest form (csrc/walk.hip) ------------------------------------------------------------
 * replaces: Skeleton.paths() and the per-path numpy of utility._xs_occurrences, for every tree of a call at once.  Both calls are
 * asynchronous on `stream`, allocate nothing, use no atomics and are built with -ffp-contract=off.
 *
 * kh_walk_orient: adjacency as for kh_forest_ticks (row_start u32 [nverts+1], nbr u32 [nslots], the distinct neighbours of a vertex
 * ascending, no self loops); comp u32 [nverts] as kh_forest_components writes it.  A listed component is a TREE of two vertices or
 * more (the caller checks ne == nv - 1), given by its critical vertices, ascending: those of degree 1 or >= 3 AND its smallest
 * vertex (comp[v] == v) whatever its degree: crit u32 [ncrit], component c at [crit_start[c], crit_start[c+1]), crit_start u32
 * [ncomps+1].  leaf_start u32 [ncomps+1]: the prefix sum of (vertices of degree 1) - 1 per listed component; npaths = its last word.
 * Output, every word written:
 *   parent, depth u32 [nverts]   the tree oriented from its root: the vertex farthest in hops from the component's smallest vertex,
 *                                the smallest index among equally far ones.  The root, and every vertex of no listed component,
 *                                has parent 0xFFFFFFFF and depth 0.
 *   path_leaf, path_len u32 [npaths]   at leaf_start[c] + k the k-th leaf of component c in the order a depth-first walk from the
 *                                root reaches them when it takes neighbours in ascending index (the vertices of degree 1 but the
 *                                root, in preorder), and depth + 1, the vertices of the path root .. leaf.
 * Scratch, sized by the caller: slot_scratch u32 [3*nslots] (far, twin, hops per slot of a critical vertex), rec_scratch u32
 * [8*ncrit] (per record of the oriented contracted tree: vertex, slot to the parent, depth, first child, children, first record of
 * round b, leaves below, leaves before).  A thread per critical vertex walks its chains; ONE WAVE per component orients the
 * contracted tree, twice (from the smallest vertex for the hops, from the root), counts the leaves bottom-up and places them
 * top-down; a thread per record writes parent / depth along its chain.  0 <= nverts, nslots < 2^31.                              */
int kh_walk_orient(const uint32_t* row_start, const uint32_t* nbr, const uint32_t* comp, const uint32_t* crit,
                   const uint32_t* crit_start, const uint32_t* leaf_start, int64_t nverts, int64_t nslots, int64_t ncrit,
                   int64_t ncomps, int64_t npaths, uint32_t* slot_scratch, uint32_t* rec_scratch, uint32_t* parent, uint32_t* depth,
                   uint32_t* path_leaf, uint32_t* path_len, void* stream);

/* kh_walk_emit: parent, path_leaf as above; pstart i64 [npaths+1], the prefix sum of path_len (pstart[0] = 0, pstart[npaths] =
 * nocc < 2^31); vox i32 [nverts,3], every vertex's voxel.
 * Output: occ_vertex u32 [nocc], every word written: at [pstart[p], pstart[p+1]) the vertices of path p from the root to the leaf;
 * normal f64 [nocc,3] (window >= 1; with window 0 it is not touched and may be null): the unit normals of
 * kimimaro.utility's section loop along every path.  d_j = vox[next] - vox[this], the last vertex repeats the last difference.
 *   window 1: float32 d / sqrtf(((dx*dx) + (dy*dy)) + (dz*dz)), root and quotient correctly rounded, then widened; a thread per
 *             occurrence.
 *   window n > 1: f64 throughout, |d| < 2^24; two moving averages over the input extended by n entries on both sides by reflection
 *             (np.pad "symmetric": j mod 2L, mirrored above L): forwards (sums of integers, exact), then over the reversed result,
 *             where R is the SEQUENTIAL running sum in padded order and out = (R[i + n] - R[i]) / n -- numpy's cumsum, addition by
 *             addition -- then v / sqrt(((x*x) + (y*y)) + (z*z)).  A thread per path; first f64 [nocc,3] is its scratch.
 * A zero vector gives NaN in all three components.                                                                              */
int kh_walk_emit(const uint32_t* parent, const uint32_t* path_leaf, const int64_t* pstart, const int32_t* vox, int64_t nverts,
                 int64_t npaths, int64_t nocc, int window, uint32_t* occ_vertex, double* normal, double* first, void* stream);

#ifdef __cplusplus
}
#endif
#endif
