"""Host orchestration of the HIP kernels (one process = one GPU).

PyTorch is used ONLY as plumbing: device allocations (caching allocator), H2D/D2H copies and the
current HIP stream.  Every computation is a hand-written kernel in libkimi_hip.so reached through the
C ABI of include/kimi_hip.h.

The engine works on whole-volume, Fortran-ordered 1-D device arrays.  Because connected components
are disjoint, all labels share one DAF / PDRF / dist / alive volume and every label is processed by
its own workgroup (kimimaro/intake.py:434-517 runs them one after the other on cropped copies).
"""
from __future__ import annotations

import ctypes as C
import os
import sys
import time
from types import SimpleNamespace

import numpy as np

from . import _abi
from .holes import resolve_holes
from .volume import as_3d, ranges

NONE32 = 0xFFFFFFFF


def _torch():
    import torch
    if not torch.cuda.is_available():
        raise _abi.HipUnavailableError("kimimaro_amd: torch sees no GPU; the product path has no CPU fallback.")
    return torch


# the launch plan is pure numpy and lives in kimimaro_amd.plan; its names stay importable from here
from .plan import (SCHED_LEVELS, SCRATCH_BYTES_PER_LABEL, SCRATCH_BYTES_PER_VOXEL, SCRATCH_POOL_FRACTION, SWEEP_FIELDS,  # noqa: F401
                   LabelSet, LabelStats, arena_units, int_key_mode, int_levels, label_order, level_windows, plan_arena, plan_launches,
                   plan_spill, plan_sweep, plan_tasks, sweep_radii)


class Engine:
    def __init__(self, device=None):
        self.lib = _abi.require_gpu()
        self.torch = _torch()
        if device is None:
            device = self.torch.cuda.current_device()
        self.device = self.torch.device("cuda", device) if isinstance(device, int) else self.torch.device(device)
        # one process drives one GPU: the library launches on the CURRENT device, so make this engine's device current
        self.torch.cuda.set_device(self.device)
        self.last_tasks = None   # task records (statistics, status) of this engine's most recent run_labels call
        self.last_path_kernel_ms = []   # (labels, milliseconds) of its path-loop launches when `timings` was asked for (HIP events)
        self.last_path_span_ms = 0.0    # first start to last end of those launches (they overlap on two streams)
        self.profile = False  # True: kh_trace_paths also fills the pop / push / fire cycle split (slower)
        self._side = None     # second stream: the biggest labels run there while the others are collected
        self.split_slots = int(os.environ.get("KH_SPLIT_SLOTS", "256"))   # labels that go to the second stream (one big-LDS workgroup per CU) when results are consumed incrementally
        self.split_min_voxels = 16384       # ... if they have at least this many voxels
        self.sweep = os.environ.get("KH_SWEEP", "1") != "0"   # False: every invalidation runs as the heap emulation (tests, comparisons)
        # integer levels (csrc/sweep.h) whenever the anisotropy allows them; False: always the table of ranks (tests, A/B runs)
        self.int_keys = os.environ.get("KH_SWEEP_INT_KEYS", "1") != "0"
        # heap and ghost journal of a launch's labels from one pool, on demand (False: a slice per label, rounds 1-5)
        self.scratch_pool = os.environ.get("KH_SCRATCH_POOL", "1") != "0"
        self.scratch_pool_fraction = SCRATCH_POOL_FRACTION      # tests: a pool too small for the labels that ask (they are traced again)
        # find_root, the DAF search and compute_pdrf inside the path kernel, by each label's own workgroup (KH_TRACE_FUSED_EDF);
        # False: as launches of their own over all labels in front of it (rounds 1-5; kept for return_fields and other exponents)
        self.fuse_edf = os.environ.get("KH_FUSE_EDF", "1") != "0"
        # volumes in flight: this many of the largest labels of a call are fused and launched FIRST, on a second stream (0: off)
        self.early_labels = int(os.environ.get("KH_EARLY_LABELS", "0"))
        # volumes in flight: called (once per volume) between the searches and the path loop, with this lane's stream drained --
        # kimimaro_amd.lanes._CohortGate holds the lane there until the searches of every volume of its cohort are through
        self.path_gate = None
        self.heap_prio = os.environ.get("KH_HEAP_PRIO", "0") == "1"         # s_setprio 3 for the heap-emulation wave (A/B knob)
        self.sweep_window = os.environ.get("KH_SWEEP_WINDOW", "1") != "0"   # level words for a window of levels only (A/B knob)
        # ghosts: a call of the sweep that leaves voxels undecided goes on with them as ghosts instead of running
        # the heap emulation at once; "paranoid" rolls every such call back at once (a test of the roll-back; results identical)
        self.ghosts = os.environ.get("KH_GHOSTS", "1") != "0"
        self.ghost_paranoid = os.environ.get("KH_GHOSTS", "1") == "paranoid"
        # the launch of the largest labels (second stream, single-volume mode) keeps two chunks of the invalidation heap in LDS
        # (128 KiB per workgroup, one workgroup per CU): every pop of a heap emulation saves one of its two L2 round trips
        self.big_lds_heap = os.environ.get("KH_BIG_LDS_HEAP", "1") != "0"
        # how many of the largest labels get such a workgroup: None = all of the second-stream launch in single-volume mode
        # (256 threads per label), none with 64 / 128 threads; a number = that many, whatever the thread count (the lanes)
        self.big_lds_labels = int(os.environ["KH_BIG_LDS_LABELS"]) if os.environ.get("KH_BIG_LDS_LABELS") else None
        self.big_threads = int(os.environ.get("KH_BIG_THREADS", "0"))     # threads per label of that launch (0: trace_threads)
        # threads per label in the path loop (64, 128 or 256).  256 serves one volume best (its searches are 4 x as wide);
        # with volumes in flight 64 does: a label whose call runs on the heap emulation -- one wave for seconds -- then holds a
        # twelfth of a CU instead of a third, and the sweep's levels hold tens of events, not hundreds (kimimaro_amd.lanes
        # sets it for its engines; measured at c3, 8 lanes: 784 vs 1134 ms per step)
        self.trace_threads = int(os.environ.get("KH_TRACE_THREADS", "256"))
        # threads per label of the two distance-field searches before the path loop (kh_edf_batch; 512 serves one volume best)
        self.edf_threads = int(os.environ.get("KH_EDF_THREADS", "512"))
        # soma labels of one volume traced side by side (kimimaro_amd.intake._trace_soma_labels): host threads with an Engine
        # and a stream each; 1 = one after the other.  The lanes set 1 for their engines (the other volumes fill the GPU).
        self.soma_lanes = int(os.environ.get("KH_SOMA_LANES", "4"))
        # HIP events around every launch of the path loop, on the launch's own stream, also without the phase marks
        # (bench.py: the production launches of one volume -> last_path_kernel_ms)
        self.time_kernels = False
        self._soma_pool = None
        self.sweep_table_limit = 1 << 24    # largest level table (entries)
        # Level words of a label stay in LDS up to this many levels (4 B each), beyond in HBM.  This sizes the LDS of the
        # path kernel's workgroups: 8192 -> 39 KiB, which leaves the registers (3 workgroups per CU) as the occupancy limit
        # instead of LDS (2 per CU at 16384) -- +20 % labels/s with several volumes in flight, nothing for a single one.
        self.sweep_lds_levels = min(int(os.environ.get("KH_SWEEP_LDS_LEVELS", 8192)), _abi.SWEEP_LDS_LEVELS)
        self._level_tables = {}
        self.scratch_divisor = 1            # tests: shrink the heap / path scratch to exercise the overflow retry
        self.holes_table_capacity = None    # tests: first size of fill_all_holes' pair table (a power of two), to exercise its retry
        self.arena_divisor = 1              # tests: shrink the sweep's event arena (a call that runs out falls back to the heap)
        # Cap of the level window (words of LDS per label's workgroup; an event beyond it abandons the call to the heap emulation).
        # The launch gives EVERY workgroup the LDS of its neediest label: at c3 one label of 3 402 wants 4 096 words (20 KB), which
        # holds a CU to 7 one-wave workgroups where the registers allow 12; with 2 048 (11.5 KB) all 12 fit.  The lanes set 2 048
        # for their 64-thread engines (kimimaro_amd.lanes); 0 = no cap (one volume alone: three 256-thread workgroups per CU).
        # The cap applies only when at most 0.5 % of the launch's labels want more (window_cap_always: whatever the share; tests).
        self.window_cap = int(os.environ.get("KH_WINDOW_CAP", "0"))
        self.window_cap_always = "KH_WINDOW_CAP" in os.environ
        # Per-label scratch (heap, work lists, event arena, path buffers: SCRATCH_BYTES_PER_VOXEL per voxel of a label) of ONE path-loop
        # launch.  Labels beyond it go to further launches of the same call, largest labels first (callers that consume
        # results incrementally only); the whole-volume fields (~40 B per voxel of the volume) are not counted.
        self.scratch_budget = int(float(os.environ.get("KH_SCRATCH_BUDGET_GB", "150")) * 1e9)

    # -- plumbing -----------------------------------------------------------
    def stream(self):
        return C.c_void_p(self.torch.cuda.current_stream(self.device).cuda_stream)

    def empty(self, n, dtype):
        return self.torch.empty(int(n), dtype=dtype, device=self.device)

    def to_device(self, arr):
        """numpy (any shape, F order expected) -> 1-D device tensor in memory order."""
        flat = np.ascontiguousarray(arr.reshape(-1, order="F"))
        if flat.dtype == np.uint16:
            flat = flat.view(np.int16)
        elif flat.dtype == np.uint32:
            flat = flat.view(np.int32)
        elif flat.dtype == np.uint64:
            flat = flat.view(np.int64)
        return self.torch.from_numpy(flat).to(self.device)

    def graph_to_device(self, voxel_graph, shape):
        """a voxel connectivity graph given on the host (cc3d's bit layout; fewer than three axes get trailing ones) -> u32 device
        volume in Fortran order.  It must have the shape of the labels.  A flat u32 / i32 tensor on this engine's device with the
        volume's number of words (what voxel_graph returns) is taken as it is."""
        t = self.torch
        if isinstance(voxel_graph, t.Tensor):
            words = int(shape[0]) * int(shape[1]) * int(shape[2])
            if (voxel_graph.device != self.device or voxel_graph.ndim != 1 or voxel_graph.numel() != words
                    or voxel_graph.dtype not in (t.int32, getattr(t, "uint32", t.int32)) or not voxel_graph.is_contiguous()):
                raise ValueError("voxel_graph must have the shape of the labels")
            return voxel_graph.view(t.int32)
        vg = as_3d(voxel_graph)
        if tuple(vg.shape) != tuple(shape):
            raise ValueError("voxel_graph must have the shape of the labels")
        return self.to_device(np.asfortranarray(vg.astype(np.uint32)))

    @staticmethod
    def ptr(t):
        return C.c_void_p(t.data_ptr())

    @staticmethod
    def optr(t):
        """pointer of an optional tensor (None -> NULL)"""
        return C.c_void_p(t.data_ptr() if t is not None else 0)

    SCHED_PAD = 4      # words in front of (and behind) the volume's filter words: the sweep reads rows of three around a voxel

    def sched_volume(self, nvox):
        """the filter words of the invalidation sweep (csrc/sweep.h): one u32 per voxel, all ones ("alive, no deadline pending"),
        with SCHED_PAD readable words on either side; hand `sched_ptr(t)` to the library."""
        return self.torch.full((int(nvox) + 2 * self.SCHED_PAD,), -1, dtype=self.torch.int32, device=self.device)

    def sched_ptr(self, t):
        return C.c_void_p(t.data_ptr() + 4 * self.SCHED_PAD if t is not None else 0)

    def sweep_levels(self, shape, anisotropy, rmax_t, cnt):
        """The sweep's level arguments for labels with largest ball radii `rmax_t` (f32 array) and voxel counts `cnt`:
        dict(rank_ptr, rdims, nlev, win, ok) -- integer mode (rank_ptr NULL, rdims = (gx, gy, gz)) when the anisotropy allows it
        (int_key_mode), else the table of ranks (level_table); None when no label can use the sweep."""
        rmax_t = np.asarray(rmax_t, dtype=np.float32)
        finite = rmax_t[np.isfinite(rmax_t)]
        if not finite.size or float(finite.max()) <= 0:
            return None
        top = float(finite.max())
        mode = int_key_mode(anisotropy, top) if self.int_keys else None
        if mode is not None:
            gq, gx, gy, gz = mode
            nlev, win = int_levels(anisotropy, gq, rmax_t.astype(np.float64), self.sweep_lds_levels)
            ok = np.isfinite(rmax_t) & (rmax_t > 0) & (nlev <= _abi.SWEEP_MAX_LEVELS)
            if not self.sweep_window:
                win = np.zeros_like(win)
            return {"d_rank": None, "rdims": (gx, gy, gz), "nlev": np.where(ok, nlev, 0), "win": np.where(ok, win, 0), "ok": ok}
        d_rank, rdims, keys, covered = self.level_table(shape, anisotropy, top)
        nlev = np.searchsorted(keys, rmax_t, side="left").astype(np.int64)   # keys below the radius: levels 0..nlev-1
        ok = np.isfinite(rmax_t) & (rmax_t <= covered) & (nlev <= _abi.SWEEP_MAX_LEVELS) & (nlev > 0)
        nlev = np.where(ok, nlev, 0)
        win = level_windows(keys, anisotropy, nlev, self.sweep_lds_levels).astype(np.int64) if self.sweep_window \
            else np.zeros(nlev.shape, dtype=np.int64)
        return {"d_rank": d_rank, "rdims": rdims, "nlev": nlev, "win": win, "ok": ok}

    def sync(self):
        self.torch.cuda.synchronize(self.device)

    def soma_lane_pool(self, width):
        """the lanes of the soma labels (made once per Engine): engines of the single-volume kind on streams of their own"""
        from .lanes import Lanes, _StreamScope
        if self._soma_pool is None or self._soma_pool.width < width:
            if self._soma_pool is not None:
                self._soma_pool.close()

            def make():
                e = Engine(self.device)
                e.soma_lanes = 1
                # the lane engines trace with the parent's settings (a test that switches the sweep or the ghosts off means the somas too)
                for knob in ("sweep", "ghosts", "ghost_paranoid", "int_keys", "scratch_divisor", "arena_divisor", "window_cap", "window_cap_always", "profile",
                             "trace_threads", "edf_threads", "sweep_window", "sweep_lds_levels", "big_lds_heap", "scratch_pool",
                             "scratch_pool_fraction", "heap_prio"):
                    setattr(e, knob, getattr(self, knob))
                return e
            self._soma_pool = Lanes(width, device=self.device, engine_factory=make,
                                    stream_factory=lambda e: _StreamScope(self.torch, e))
        return self._soma_pool

    def sync_stream(self):
        """wait for the calling thread's current stream only (the phase marks: another lane's kernels are not this volume's)"""
        self.torch.cuda.current_stream(self.device).synchronize()

    # -- f1: connected components on the device ---------------------------------
    def ccl(self, labels, d_graph=None):
        """26-connected multi-label CCL (kimimaro/utility.py:58-83).  labels: host ndarray (F order, integer).
        Returns (d_cc u32 device tensor, N, representative[N+1] host array of smallest linear indices)."""
        t = self.torch
        lab = labels
        if lab.dtype == bool:
            lab = lab.view(np.uint8)
        if lab.dtype.kind not in "ui":
            lab = lab.astype(np.uint64)
        lab = np.asfortranarray(lab)
        return self.ccl_device(self.to_device(lab), lab.dtype.itemsize, lab.shape, d_graph)

    def ccl_device(self, d_lab, itemsize, shape, d_graph=None):
        """kh_ccl26 on a label volume that is already resident in HBM; d_graph (u32 per voxel, cc3d's layout): kh_ccl26_graph,
        the components of the voxel connectivity graph (kimimaro/utility.py:73-75)."""
        t = self.torch
        n = int(shape[0]) * int(shape[1]) * int(shape[2])
        d_parent = self.empty(n, t.int32)
        d_counts = self.empty((n + 1023) // 1024, t.int32)
        d_cc = self.empty(n, t.int32)
        d_rep = self.empty(n + 1, t.int32)
        d_total = self.empty(1, t.int32)
        d_cc16 = self.empty(n, t.int16)
        if d_graph is not None:
            _abi.check(self.lib.kh_ccl26_graph(self.ptr(d_lab), itemsize, self.ptr(d_graph), shape[0], shape[1], shape[2],
                                               self.ptr(d_parent), self.ptr(d_counts), self.ptr(d_cc), self.ptr(d_rep), self.ptr(d_total),
                                               self.ptr(d_cc16), self.stream()))
        else:
            _abi.check(self.lib.kh_ccl26(self.ptr(d_lab), itemsize, shape[0], shape[1], shape[2], self.ptr(d_parent),
                                         self.ptr(d_counts), self.ptr(d_cc), self.ptr(d_rep), self.ptr(d_total), self.ptr(d_cc16),
                                         self.stream()))
        ncomp = int(d_total.cpu().numpy().view(np.uint32)[0])
        if ncomp < 65536:
            d_cc.kh_u16 = d_cc16      # the u16 copy of the ids serves every later sweep (narrow()); it lives as long as this object
        rep = d_rep[: ncomp + 1].cpu().numpy().view(np.uint32)
        return d_cc, ncomp, rep

    def voxel_graph(self, d_lab, itemsize, shape, connectivity=26, d_pairs=None):
        """kh_voxel_graph (csrc/graph.hip) on a label volume resident in HBM: the voxel connectivity graph, a flat u32
        device volume (int32 words) in Fortran order -- the form ccl_device, edt_graph and the searches take as d_graph.
        itemsize: 1, 2, 4 or 8 bytes per label.  d_pairs: None, or a flat int64 device tensor of the pair table's rows (lo, hi) as
        the kernel wants them: lo < hi, neither 0, sorted, unique (ops.merge_pairs makes them)."""
        sx, sy, sz = (int(v) for v in shape)
        d_graph = self.empty(sx * sy * sz, self.torch.int32)
        npairs = 0 if d_pairs is None else int(d_pairs.numel()) // 2
        _abi.check(self.lib.kh_voxel_graph(self.ptr(d_lab), int(itemsize), sx, sy, sz, int(connectivity),
                                           self.optr(d_pairs if npairs else None), npairs, self.ptr(d_graph), self.stream()))
        return d_graph

    def narrow(self, d_cc):
        """(device label volume, bytes per label) to sweep over: the u16 copy kh_ccl26 made of `d_cc` when it carries one, else
        (d_cc, 4).  The copy is an attribute of the tensor OBJECT ccl_device returned: a clone, a view or a converted tensor has
        none.  The rule: whoever writes into the storage of such a tensor calls edited() on it first."""
        d16 = getattr(d_cc, "kh_u16", None)
        return (d_cc, 4) if d16 is None else (d16, 2)

    @staticmethod
    def edited(d):
        """`d` is about to be written in place: the u16 copy it may carry (narrow()) no longer matches and is dropped."""
        if hasattr(d, "kh_u16"):
            del d.kh_u16

    def fill_voids(self, d_mask, shape, ndim=3):
        """kh_fill_voids (fill_voids.fill, kimimaro/trace.py:109) on a u8 mask resident in HBM; ndim < 3: a 2-D / 1-D image given as
        shape (nx, ny, 1) / (nx, 1, 1), whose border is its outline.  Returns (filled u8 mask on the device, number of voxels that changed)."""
        t = self.torch
        shape = tuple(int(v) for v in shape) + (1,) * (3 - len(shape))
        n = int(shape[0]) * int(shape[1]) * int(shape[2])
        d_parent = self.empty(n, t.int32)
        d_open = self.empty(n, t.uint8)
        d_out = self.empty(n, t.uint8)
        d_cnt = self.empty(1, t.int64)
        _abi.check(self.lib.kh_fill_voids_nd(self.ptr(d_mask), int(ndim), shape[0], shape[1], shape[2], self.ptr(d_parent),
                                             self.ptr(d_open), self.ptr(d_out), self.ptr(d_cnt), self.stream()))
        return d_out, int(d_cnt.cpu().numpy()[0])

    def region_graph(self, d_lab, label_bytes, shape, ndim=3, mark=lambda name: None, faces=None):
        """The regions of a label volume resident in HBM (6-connected components of equal value, 0 included) and their adjacency:
        kh_regions6 -> kh_region_table -> kh_region_pairs.  Returns (d_region: u32 ids 1..R per voxel on the device; value u64,
        count u32, face u8: host arrays [R + 1]; pairs: host u64, every unordered pair of regions that share a voxel face once, as
        smaller id << 32 | larger id, in no particular order; info: regions, pairs, table_capacity, table_tries, compact_ms).
        mark(name) is called in front of and behind the launches of each pass (Engine.fill_all_holes puts HIP events there).
        faces (a box of a dataset, post.region_graph_chunked): the six-bit mask of the faces of the array that are faces of the
        dataset; `face` then means "owns a voxel on one of those" (kh_region_table_box).  None: every face, kh_region_table."""
        t = self.torch
        sx, sy, sz = shape
        n = sx * sy * sz
        mark("regions")
        d_parent = self.empty(n, t.int32)
        d_chunks = self.empty((n + 1023) // 1024, t.int32)
        d_region = self.empty(n, t.int32)
        d_rep = self.empty(n + 1, t.int32)
        d_total = self.empty(1, t.int32)
        _abi.check(self.lib.kh_regions6(self.ptr(d_lab), int(label_bytes), sx, sy, sz, self.ptr(d_parent), self.ptr(d_chunks),
                                        self.ptr(d_region), self.ptr(d_rep), self.ptr(d_total), self.stream()))
        mark("regions")
        nreg = int(d_total.cpu().numpy().view(np.uint32)[0])
        del d_parent, d_chunks
        mark("table")
        d_value = self.empty(nreg + 1, t.int64)
        d_count = self.empty(nreg + 1, t.int32)
        d_face = self.empty(nreg + 1, t.uint8)
        if faces is None:
            _abi.check(self.lib.kh_region_table(self.ptr(d_lab), int(label_bytes), self.ptr(d_region), self.ptr(d_rep), nreg, int(ndim),
                                                sx, sy, sz, self.ptr(d_value), self.ptr(d_count), self.ptr(d_face), self.stream()))
        else:
            _abi.check(self.lib.kh_region_table_box(self.ptr(d_lab), int(label_bytes), self.ptr(d_region), self.ptr(d_rep), nreg,
                                                    int(ndim), sx, sy, sz, int(faces), self.ptr(d_value), self.ptr(d_count),
                                                    self.ptr(d_face), self.stream()))
        mark("table")
        del d_rep
        # the hash set of region pairs: 32 slots per region to begin with (a region of dense neuropil touches about a dozen others),
        # never more than the 3 n faces can ask for; a table that overflows is reported by the kernel and tried again, 4 x larger
        pow2 = lambda v: 1 << max(int(v) - 1, 1).bit_length()
        limit = max(pow2(8 * n), 1 << 12)
        cap = self.holes_table_capacity or min(max(pow2(32 * nreg), 1 << 12), limit)
        tries = 0
        while True:
            tries += 1
            d_table = self.empty(cap, t.int64)
            d_state = self.empty(2, t.int32)
            mark("pairs")
            _abi.check(self.lib.kh_region_pairs(self.ptr(d_region), sx, sy, sz, self.ptr(d_table), cap, self.ptr(d_state), self.stream()))
            mark("pairs")
            state = d_state.cpu().numpy().view(np.uint32)
            if state[1] == 0:
                break
            if cap >= limit:
                raise _abi.KimiHipError("kh_region_pairs: the pair table overflows at %d slots for %d voxels" % (cap, n))
            del d_table
            cap *= 4
        t0 = time.perf_counter()
        pairs = d_table[d_table != 0].cpu().numpy().view(np.uint64)
        del d_table
        value = d_value.cpu().numpy().view(np.uint64)
        count = d_count.cpu().numpy().view(np.uint32)
        face = d_face.cpu().numpy()
        if pairs.size != int(state[0]):
            raise _abi.KimiHipError("kh_region_pairs: %d keys counted, %d found in the table" % (int(state[0]), pairs.size))
        info = dict(regions=nreg, pairs=int(pairs.size), table_capacity=cap, table_tries=tries, compact_ms=(time.perf_counter() - t0) * 1e3)
        return d_region, value, count, face, pairs, info

    def region_seam_pairs(self, d_low, d_high, capacity=None):
        """kh_region_seam_pairs: the distinct keys low[p] << 32 | high[p] of two facing planes of region ids (u32 on the device, one
        length m) -> (the keys as a host u64 array in no particular order, the table capacity that held them, the tries).  The
        table starts at `capacity`, by default the power of two above 4 m slots (at most m keys: a quarter full at the worst), and
        is tried again 4 x larger when the kernel reports a probe sequence past its limit."""
        t = self.torch
        m = int(d_low.numel())
        assert int(d_high.numel()) == m and m >= 1
        cap = int(capacity) if capacity else max(1 << max(4 * m - 1, 1).bit_length(), 64)
        tries = 0
        while True:
            tries += 1
            d_table = self.empty(cap, t.int64)
            d_state = self.empty(2, t.int32)
            _abi.check(self.lib.kh_region_seam_pairs(self.ptr(d_low), self.ptr(d_high), m, self.ptr(d_table), cap, self.ptr(d_state),
                                                     self.stream()))
            state = d_state.cpu().numpy().view(np.uint32)
            if state[1] == 0:
                break
            if cap >= 64 * m + 4096:
                raise _abi.KimiHipError("kh_region_seam_pairs: the pair table overflows at %d slots for %d pairs" % (cap, m))
            del d_table
            cap *= 4
        keys = d_table[d_table != 0].cpu().numpy().view(np.uint64)
        if keys.size != int(state[0]):
            raise _abi.KimiHipError("kh_region_seam_pairs: %d keys counted, %d found in the table" % (int(state[0]), keys.size))
        return keys, cap, tries

    def region_apply_box(self, d_region, base, d_owner, d_lab, label_bytes):
        """kh_region_apply_box: paints a core of a dataset, resident in HBM, in place.  d_region: the core's slice of
        the region store (u32 provisional ids, one per voxel of d_lab); d_owner: u64 [nregions + 1] on the device, the owners of the
        ids base + 1 .. base + nregions (entry 0 unused).  -> (voxels painted, voxels whose id lay outside that range: they are left
        alone and no table entry is read for them)."""
        self.edited(d_lab)
        n = int(d_region.numel())
        assert int(d_lab.numel()) == n
        d_state = self.empty(2, self.torch.int64)
        _abi.check(self.lib.kh_region_apply_box(self.ptr(d_region), int(base), int(d_owner.numel()) - 1, self.ptr(d_owner), self.ptr(d_lab),
                                                int(label_bytes), n, self.ptr(d_state), self.stream()))
        state = d_state.cpu().numpy().view(np.uint64)
        return int(state[0]), int(state[1])

    def fill_all_holes(self, d_lab, label_bytes, shape, ndim=3, stats=None):
        """kimimaro.intake.fill_all_holes (kimimaro/intake.py:747-795) on a label volume resident in HBM (1-D, Fortran order, 1 / 2 / 4 /
        8 bytes per label; modified in place): the holes of every label in ONE pass over the volume instead of a fill per bounding
        box.  The regions, their table and their adjacency are made on the device (region_graph); the table and
        the pairs (the only device-to-host traffic) go to kh_host_resolve_holes, which says who fills what; kh_region_apply paints.
        ndim: dimensionality of the caller's array (kh_fill_voids_nd's meaning).  Returns the number of voxels filled.
        stats (a dict, optional): region_graph's info, labels, label_value / label_state (the host's verdict per label,
        _abi.HOLES_* bits), filled, resolve_ms, and -- at the price of a synchronisation at the end -- the HIP-event time of every
        pass (regions_ms, table_ms, pairs_ms, apply_ms)."""
        self.edited(d_lab)
        t = self.torch
        shape = tuple(int(v) for v in shape) + (1,) * (3 - len(shape))
        n = shape[0] * shape[1] * shape[2]
        marks = []

        def mark(name):
            if stats is not None:
                ev = t.cuda.Event(enable_timing=True)
                ev.record(t.cuda.current_stream(self.device))
                marks.append((name, ev))

        d_region, value, count, face, pairs, info = self.region_graph(d_lab, label_bytes, shape, ndim, mark)
        t0 = time.perf_counter()
        owner, label_value, label_state, filled = resolve_holes(value, count, face, pairs)
        t1 = time.perf_counter()
        mark("apply")
        if filled:
            d_owner = t.from_numpy(owner.view(np.int64)).to(self.device)
            _abi.check(self.lib.kh_region_apply(self.ptr(d_region), self.ptr(d_owner), self.ptr(d_lab), int(label_bytes), n, self.stream()))
        mark("apply")
        if stats is not None:
            stats.update(info, labels=int(label_value.size), label_value=label_value, label_state=label_state, filled=int(filled),
                         resolve_ms=(t1 - t0) * 1e3)
            self.sync_stream()
            for (name, a), (_, b) in zip(marks[0::2], marks[1::2]):
                stats[name + "_ms"] = stats.get(name + "_ms", 0.0) + a.elapsed_time(b)
        return int(filled)

    def to_host_volume(self, d, shape, dtype=np.uint32):
        return d.cpu().numpy().view(dtype).reshape(shape, order="F")

    def face(self, d, shape, axis, index):
        """one face of a device volume as a host array (Fortran order semantics: d is [sx, sy, sz], x fastest)."""
        v = d.view(shape[2], shape[1], shape[0])  # torch C order (z, y, x) == F order (x, y, z)
        if axis == 2:
            f = v[index, :, :]      # (y, x)
        elif axis == 1:
            f = v[:, index, :]      # (z, x)
        else:
            f = v[:, :, index]      # (z, y)
        return np.asfortranarray(f.contiguous().cpu().numpy().view(np.uint32).T)  # -> (x,y) / (x,z) / (y,z)

    # -- a1 -------------------------------------------------------------------
    def edt(self, d_labels, label_bytes, shape, anisotropy, black_border, out=None, workspace=None, ndim=3):
        """ndim: dimensionality of the caller's array (trailing axes of extent 1 beyond it are not axes)."""
        sx, sy, sz = shape
        n = sx * sy * sz
        t = self.torch
        if out is None:
            out = self.empty(n, t.float32)
        if workspace is None:
            workspace = self.empty(n, t.float32)  # ping-pong buffer of the passes (include/kimi_hip.h)
        _abi.check(self.lib.kh_edt_nd(self.ptr(d_labels), label_bytes, int(ndim), sx, sy, sz, float(anisotropy[0]),
                                      float(anisotropy[1]), float(anisotropy[2]), int(bool(black_border)),
                                      self.ptr(workspace), self.ptr(out), self.stream()))
        return out

    def edt_graph(self, d_labels, label_bytes, d_graph, shape, anisotropy, black_border):
        """edt.edt(labels, voxel_graph=) (kimimaro/intake.py:174-183; PARITY UNPINNED, include/kimi_hip.h): the doubled image of the
        graph's walls, a binary transform with half the pitch, sampled at the voxels."""
        sx, sy, sz = (int(v) for v in shape)
        n = sx * sy * sz
        t = self.torch
        cells = self.empty(8 * n, t.uint8)
        _abi.check(self.lib.kh_edt_graph_cells(self.ptr(d_labels), label_bytes, self.ptr(d_graph), sx, sy, sz, int(bool(black_border)),
                                               self.ptr(cells), self.stream()))
        half = [np.float32(a) / np.float32(2) for a in anisotropy]
        fine = self.edt(cells, 1, (2 * sx, 2 * sy, 2 * sz), half, black_border)
        out = self.empty(n, t.float32)
        _abi.check(self.lib.kh_edt_graph_sample(self.ptr(fine), sx, sy, sz, self.ptr(out), self.stream()))
        return out

    def label_stats(self, d_labels, label_bytes, d_dbf, shape, nlabels):
        t = self.torch
        n1 = nlabels + 1
        counts = self.empty(n1, t.int32)
        dmax = self.empty(n1, t.float32)
        first = self.empty(n1, t.int32)
        xmin = self.empty(n1, t.int32)
        xmax = self.empty(n1, t.int32)
        yz = self.empty(4 * n1, t.int32)
        nvox = shape[0] * shape[1] * shape[2]
        _abi.check(self.lib.kh_label_stats(self.ptr(d_labels), label_bytes, self.ptr(d_dbf), nvox, shape[0], shape[1],
                                           nlabels, self.ptr(counts), self.ptr(dmax), self.ptr(first), self.ptr(xmin),
                                           self.ptr(xmax), self.ptr(yz), self.stream()))
        u32 = lambda x: x.cpu().numpy().view(np.uint32)
        return LabelStats(u32(counts), dmax.cpu().numpy(), u32(first), u32(xmin), u32(xmax), u32(yz).reshape(n1, 4))

    @staticmethod
    def box(d, shape, lo, hi):
        """the box [lo, hi) (x, y, z) of a device volume as a device view indexed [z, y, x]: torch C order (z, y, x) == Fortran
        order (x, y, z).  Writing through it writes the volume."""
        return d.view(shape[2], shape[1], shape[0])[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]]

    def crop(self, d, shape, lo, hi, dtype=np.uint32):
        """host copy of the box [lo, hi) of a device volume, as an (x, y, z) Fortran-ordered array."""
        return np.asfortranarray(self.box(d, shape, lo, hi).contiguous().cpu().numpy().view(dtype).transpose(2, 1, 0))

    # -- level table of the order-free invalidation sweep (csrc/sweep.h) -------------
    def level_table(self, shape, anisotropy, rmax):
        """(d_rank int32 [ra*rb*rc], (ra, rb, rc), keys host f32 sorted, radius covered) for balls up to `rmax`.
        rank[a + ra*(b + rb*c)] = index of the flood's key of offset (a, b, c) among the distinct keys; the keys
        are computed by the device with the flood's own float operations (kh_level_keys), sorting and ranking is
        plumbing (torch.unique).  The table is clipped to `sweep_table_limit` entries."""
        t = self.torch
        w = [float(np.float32(a)) for a in anisotropy]
        dims = [int(min(int(rmax / w[i]) + 2, int(shape[i]))) for i in range(3)]
        while dims[0] * dims[1] * dims[2] > self.sweep_table_limit:
            rmax *= 0.8
            dims = [int(min(int(rmax / w[i]) + 2, int(shape[i]))) for i in range(3)]
        # every offset with a key below `covered` is inside the table (one row of slack for the rounding of the key)
        covered = min([w[i] * (dims[i] - 1) for i in range(3) if dims[i] < shape[i]] + [float("inf")])
        key = (tuple(w), tuple(dims))
        hit = self._level_tables.get(key)
        if hit is None:
            n = dims[0] * dims[1] * dims[2]
            d_keys = self.empty(n, t.float32)
            _abi.check(self.lib.kh_level_keys(dims[0], dims[1], dims[2], w[0], w[1], w[2], self.ptr(d_keys), self.stream()))
            uniq, inverse = t.unique(d_keys, sorted=True, return_inverse=True)
            hit = (inverse.to(t.int32).contiguous(), tuple(dims), uniq.cpu().numpy())
            if len(self._level_tables) > 8:
                self._level_tables.clear()
            self._level_tables[key] = hit
        return hit[0], hit[1], hit[2], covered

    # -- one binary object on its own (the function-level mirrors of ops.py) ---------------
    def single_object(self, mask, anisotropy, rmax=0.0, dbf=None, voxel_graph=None, window_cap=0, window_cap_always=False,
                      arena_divisor=1):
        """Device context of ONE binary object given as a host mask (x, y, z; Fortran order): component volume (0 / 1),
        voxel list, neighbour masks, per-label scratch and -- for ball radii up to `rmax` -- the level table and the
        event arena of the invalidation sweep.  Returns a dict of device tensors + the kh_label_t record.
        window_cap, window_cap_always, arena_divisor: the planner's knobs (plan.plan_sweep) for a smaller level window or event
        arena than the object is entitled to; a call that runs out of either is redone by the heap emulation (tests)."""
        t = self.torch
        lib = self.lib
        P = self.ptr
        m = as_3d(mask)
        shape = tuple(int(v) for v in m.shape)
        nvox = shape[0] * shape[1] * shape[2]
        cc = np.asfortranarray((m != 0).astype(np.uint32))
        d_cc = self.to_device(cc)
        d_dbf = self.to_device(np.asfortranarray(dbf, dtype=np.float32).reshape(shape, order="F")) if dbf is not None \
            else t.zeros(nvox, dtype=t.float32, device=self.device)
        stats = self.label_stats(d_cc, 4, d_dbf, shape, 1)
        cnt = int(stats.counts[1])
        task = np.zeros(1, dtype=_abi.LABEL_T)
        task["segid"] = 1
        task["count"] = cnt
        # the reference runs on the array it is given: the x faces of THAT array matter to the heap order
        # (dijkstra_invalidation.hpp:116-123), not the object's own extent
        task["xmin"], task["xmax"] = 0, shape[0] - 1
        task["source"] = stats.first_index[1]
        task["root"] = NONE32
        task["q_capacity"] = cnt + 64
        hcap = 27 * cnt + 4096          # every push of the flood fits: a voxel is pushed by at most 26 neighbours (and the sweep's lists)
        task["heap_capacity"] = hcap
        task["path_capacity"] = 4 * cnt + 1024
        ctx = {"shape": shape, "nvox": nvox, "count": cnt, "d_cc": d_cc, "d_dbf": d_dbf, "dbf_max": float(stats.dbf_max[1])}
        d_slot = t.from_numpy(np.array([-1, 0], dtype=np.int32)).to(self.device)
        d_off = t.zeros(1, dtype=t.int32, device=self.device)
        d_cur = self.empty(1, t.int32)
        d_lists = self.empty(max(cnt, 1), t.int32)
        d_nbr = self.empty(nvox, t.int32)
        st = self.stream()
        _abi.check(lib.kh_scatter_lists(P(d_cc), 4, nvox, P(d_slot), 1, P(d_off), P(d_cur), P(d_lists), st))
        _abi.check(lib.kh_neighbor_mask(P(d_cc), 4, shape[0], shape[1], shape[2], P(d_nbr), st))
        d_gate = None
        if voxel_graph is not None:
            # voxel_graph= / voxel_connectivity_graph= of the reference's calls: directions the caller's words do not allow
            # leave the neighbour masks every search and the invalidation work from (kh_apply_voxel_graph)
            d_graph = self.graph_to_device(voxel_graph, shape)
            d_gate = t.zeros(nvox + 4, dtype=t.uint8, device=self.device)
            _abi.check(lib.kh_apply_voxel_graph(P(d_nbr), P(d_graph), nvox, P(d_gate), st))
        ctx["d_gate"] = d_gate
        ctx.update(d_slot=d_slot, d_lists=d_lists, d_nbr=d_nbr, d_queues=self.empty(4 * (cnt + 64), t.int32),
                   d_heap=self.empty(2 * hcap, t.int64), d_qstate=t.zeros(nvox + 4, dtype=t.uint8, device=self.device))
        rmax = float(np.float32(rmax))
        lv = self.sweep_levels(shape, anisotropy, [rmax], [cnt]) if self.sweep and cnt > 0 and np.isfinite(rmax) and rmax > 0 else None
        # (by default no window cap and no arena divisor; keep_unfit: this record books arena and spill table whatever the levels fit)
        sw = plan_sweep([cnt], np.array([rmax], dtype=np.float32), lv, window_cap=window_cap, window_cap_always=window_cap_always,
                        arena_divisor=arena_divisor, lds_levels=self.sweep_lds_levels, keep_unfit=True)
        for key in SWEEP_FIELDS:
            task[key] = getattr(sw, key)
        sweep_on, max_nlev, ev_units = sw.sweep_on, sw.max_nlev, sw.ev_total
        d_rank, rdims = (lv["d_rank"], lv["rdims"]) if sweep_on else (None, (0, 0, 0))
        d_arena = self.empty(max(ev_units, 1) * 32 + 32, t.int64)
        ctx.update(d_rank=d_rank, rdims=rdims, max_nlev=max_nlev, d_arena=d_arena,
                   arena_ptr=C.c_void_p((d_arena.data_ptr() + 255) & ~255),
                   sweep_on=sweep_on,
                   d_cstate=t.zeros(nvox if sweep_on else 1, dtype=t.int64, device=self.device),
                   d_sched=self.sched_volume(nvox) if sweep_on else None,
                   d_task=t.from_numpy(task.view(np.uint8).reshape(-1).copy()).to(self.device), task=task)
        return ctx

    def invalidate_ball(self, ctx, d_alive, path_locs, scale, const, anisotropy):
        """kh_invalidate_ball on the object of `ctx` (Engine.single_object): d_alive (u8, device) is mutated.
        Returns (voxels invalidated, task record after the call)."""
        t = self.torch
        P = self.ptr
        shape = ctx["shape"]
        d_path = t.from_numpy(np.asarray(path_locs, dtype=np.uint32).view(np.int32).copy()).to(self.device)
        d_cnt = t.zeros(1, dtype=t.int64, device=self.device)
        rank_ptr = P(ctx["d_rank"]) if ctx["d_rank"] is not None else C.c_void_p(0)
        rd = ctx["rdims"] if ctx["sweep_on"] else (0, 0, 0)       # (the kernel derives the filter words from the caller's mask)
        _abi.check(self.lib.kh_invalidate_ball(P(ctx["d_task"]), P(ctx["d_lists"]), P(ctx["d_nbr"]), shape[0], shape[1], shape[2],
                                               float(anisotropy[0]), float(anisotropy[1]), float(anisotropy[2]), P(ctx["d_dbf"]),
                                               P(d_alive), P(ctx["d_queues"]), P(ctx["d_heap"]), P(d_path), int(d_path.numel()),
                                               np.float32(scale), np.float32(const), rank_ptr, rd[0], rd[1], rd[2], ctx["max_nlev"],
                                               P(ctx["d_cstate"]), self.sched_ptr(ctx["d_sched"]), ctx["arena_ptr"],
                                               self.optr(ctx.get("d_gate")), P(d_cnt), self.stream()))
        task = ctx["d_task"].cpu().numpy().view(_abi.LABEL_T).copy()
        if int(task["status"][0]):
            raise _abi.KimiHipError("kh_invalidate_ball: %s" % _abi.describe_status(int(task["status"][0])))
        return int(d_cnt.item()), task

    # -- the per-label pipeline -------------------------------------------------
    def trace_flags(self, ghosts, pool, voxel_graph, big=False, fused=False):
        """the flag word of one kh_trace_paths launch (KH_TRACE_* of include/kimi_hip.h); big: the second-stream launch of the
        largest labels, which may keep heap chunks in LDS and have a thread count of its own"""
        A = _abi
        big_ok = self.trace_threads == 256 if self.big_lds_labels is None else True
        on = ((A.TRACE_PROFILE, self.profile), (A.TRACE_HEAP_PRIO, self.heap_prio), (A.TRACE_NO_GHOSTS, not ghosts),
              (A.TRACE_GHOST_PARANOID, ghosts and self.ghost_paranoid), (A.TRACE_BIG_LDS_HEAP, big and self.big_lds_heap and big_ok),
              (A.TRACE_SCRATCH_POOL, pool), (A.TRACE_FUSED_EDF, fused), (A.TRACE_VOXEL_GRAPH, voxel_graph))
        threads = self.big_threads if big and self.big_threads else self.trace_threads
        return sum(flag for flag, yes in on if yes) | {64: A.TRACE_THREADS_64, 128: A.TRACE_THREADS_128}.get(threads, 0)

    def edf_mode(self, mode):
        """the mode word of kh_edf_batch: 1 = find_root, 2 = DAF, with the threads per label above the low byte"""
        return mode | (self.edf_threads << 8)

    def run_labels(self, d_cc, label_bytes, d_dbf, shape, anisotropy, nlabels, labels, params, fix_branching=True, max_paths=None,
                   return_fields=False, timings=None, consume=None, scratch_scale=1, voxel_graph=None):
        """Run find_root -> DAF -> PDRF -> path loop for the connected components `labels` (kimimaro_amd.plan.LabelSet: host
        columns indexed by position, the roots as linear indices or NONE32, the target lists).  Returns a dict with per-label
        path arrays -- or, when `consume` is given, hands such dicts (one per group of labels, as the groups finish) to
        `consume` and returns None.  A label whose scratch overflowed is traced again in a launch of its own: its task record
        (in "tasks" and last_tasks) is then the retry's, so its offsets and capacities refer to that launch's buffers, not to the
        first plan's -- find a label's paths through voff / loff, never through the record's offsets.
        """
        if len(labels) == 0:
            return {"order": np.zeros(0, np.int64), "tasks": np.zeros(0, _abi.LABEL_T), "paths": []}
        volume = (d_cc, label_bytes, d_dbf, shape, anisotropy, nlabels)
        opts = SimpleNamespace(fix_branching=fix_branching, max_paths=max_paths, return_fields=return_fields, timings=timings,
                               scratch_scale=scratch_scale, voxel_graph=voxel_graph, streaming=consume is not None)
        # with a sink: more per-label scratch than the budget means several launches, each over a group of labels that fits;
        # without one (single labels, tests): one group, whose dicts -- first attempt, retries -- are kept and merged by label
        groups = plan_launches(labels.count, self.scratch_budget) if consume is not None and len(labels) > 1 else [None]
        parts, done, retried = [], [], 0
        for g in groups:
            run = self._trace_group(volume, labels if len(groups) == 1 else labels.take(g), params, consume or parts.append, opts)
            done.append(self.last_tasks)
            retried += self.last_retries
        self.last_tasks = np.concatenate(done) if len(done) > 1 else done[0]
        self.last_retries = retried           # (each group resets it: accumulate over the groups)
        if consume is not None:
            return None
        res = _merge_groups(parts, self.last_tasks)
        if return_fields:
            res["daf"] = run.d_field[:run.nvox].cpu().numpy()
            res["pdrf"] = run.b["pdrf"][:run.nvox].cpu().numpy()
            res["alive"] = run.b["alive"].cpu().numpy()
        return res

    def _trace_group(self, volume, labels, params, sink, o):
        """One group of labels that fits the scratch budget: plan -> allocate -> one of the two schedules -> retry of the labels
        whose scratch overflowed.  Every result dict goes to `sink`; leaves the labels' final task records in last_tasks."""
        d_cc, label_bytes, d_dbf, shape, anisotropy, nlabels = volume
        nl = len(labels)
        order = label_order(labels.count)
        rmax_t = sweep_radii(labels.dbf_max[order], params)
        lv = self.sweep_levels(shape, anisotropy, rmax_t, labels.count[order]) if self.sweep else None
        p = plan_tasks(labels, params, lv, order=order, rmax_t=rmax_t, nlabels=nlabels, max_paths=o.max_paths,
                       scratch_scale=o.scratch_scale, scratch_divisor=self.scratch_divisor, scratch_pool=self.scratch_pool,
                       scratch_pool_fraction=self.scratch_pool_fraction, window_cap=self.window_cap,
                       window_cap_always=self.window_cap_always, arena_divisor=self.arena_divisor, lds_levels=self.sweep_lds_levels)
        if p.sweep_on:
            self.last_arena_bytes = p.ev_total * 256
        # Who runs the searches (find_root, DAF) and the PDRF, decided once:
        #   "fused"  each label's own workgroup, inside the path kernel (KH_TRACE_FUSED_EDF);
        #   "before" batch launches over all labels in front of the path loop (return_fields, other exponents, fuse_edf off);
        #   "early"  volumes in flight (`early_labels`, set by kimimaro_amd.lanes): the LARGEST labels are fused and go first, on a
        #            second stream -- their chains, the heap emulation of a volume's large labels, seconds long, then start at once
        #            instead of behind the searches of all labels; the rest keeps the batch kernels (70 VGPRs: twice the waves per
        #            CU of the path kernel) on the lane's own stream, behind that launch.
        can_fuse = _abi.is_pow2_exponent(params["pdrf_exponent"]) and not o.return_fields
        early = int(min(self.early_labels, nl - 1)) if (can_fuse and o.streaming and self.early_labels > 0 and nl > 1) else 0
        who = "early" if early > 0 else "fused" if can_fuse and self.fuse_edf else "before"
        # tasks are sorted by size, so the biggest labels (the head of the run) are dispatched first; when the results
        # are consumed incrementally they go to a second stream and the others are collected while they still run
        slots = self.split_slots if self.big_lds_labels is None else self.big_lds_labels    # (big_lds_labels: also in a lane, whose split_slots is 0)
        n_large = early if early > 0 else int(min(slots, np.count_nonzero(p.cnt >= self.split_min_voxels)))

        run = _LabelRun(self, volume, labels, params, p, lv, o)
        run.allocate_inputs()
        if who == "before":
            run.searches(0, nl)          # (before the path loop's own volumes are allocated: the DAF volume's block serves them afterwards)
        run.allocate_path_scratch()
        self.last_retries = 0
        if o.streaming and 0 < n_large < nl:
            records = run.split_schedule(n_large, who, sink)
        else:
            records = run.single_schedule(who, sink)
        if run.retry:
            # the labels whose scratch overflowed, again with 8 x as much; their dicts go to the sink like every other and
            # their records -- the good attempt's status bits and statistics -- take the place of the failed attempt's
            nretry = len(run.retry)
            again = SimpleNamespace(**{**vars(o), "scratch_scale": o.scratch_scale * 8, "timings": None, "return_fields": False})
            self._trace_group(volume, labels.take(run.retry), params, sink, again)
            self.last_retries = nretry + self.last_retries      # (the nested call counted its own)
            pos = {int(sid): i for i, sid in enumerate(records["segid"])}
            for rec in self.last_tasks:
                records[pos[int(rec["segid"])]] = rec
        self.last_tasks = records
        return run


def _merge_groups(parts, records):
    """One result dict from the dicts a call without a sink produced: the first attempt over all labels, then the retries, whose
    labels' paths replace the failed attempt's (matched by component id); `records`: the labels' final task records."""
    res = parts[0]
    if len(parts) > 1:
        cut = lambda d, key, off, s: d[key][d[off][s]:d[off][s + 1]]
        pos = {int(sid): s for s, sid in enumerate(res["tasks"]["segid"])}
        per = {key: [cut(res, key, off, s) for s in range(len(pos))] for key, off in (("verts", "voff"), ("radii", "voff"), ("lens", "loff"))}
        for sub in parts[1:]:
            for s2, sid in enumerate(sub["tasks"]["segid"]):
                for key, off in (("verts", "voff"), ("radii", "voff"), ("lens", "loff")):
                    per[key][pos[int(sid)]] = cut(sub, key, off, s2)
        for key in per:
            res[key] = np.concatenate(per[key])
        res["voff"] = np.concatenate([[0], np.cumsum([len(v) for v in per["verts"]])])
        res["loff"] = np.concatenate([[0], np.cumsum([len(v) for v in per["lens"]])])
    res["tasks"] = records
    return res


class _LabelRun:
    """One launch plan of Engine.run_labels on the device: the plan (kimimaro_amd.plan.plan_tasks), the device buffers and the
    call's options; the steps of the pipeline are its methods."""

    def __init__(self, eng, volume, labels, params, plan, lv, o):
        self.eng, self.lib, self.t = eng, eng.lib, eng.torch
        self.d_cc, self.label_bytes, self.d_dbf, self.shape, anisotropy, _ = volume
        self.nvox = self.shape[0] * self.shape[1] * self.shape[2]
        self.w = (float(anisotropy[0]), float(anisotropy[1]), float(anisotropy[2]))
        self.labels, self.params, self.p, self.o = labels, params, plan, o
        self.nl = len(labels)
        self.st = eng.stream()
        self.timed = o.timings is not None or eng.time_kernels
        self.d_rank, self.rdims = (lv["d_rank"], lv["rdims"]) if plan.sweep_on else (None, (0, 0, 0))
        self.b = {}                # device buffers by name, in the order they were allocated
        self.d_field = None        # the DAF volume of the batch searches (kept for return_fields only)
        self.kernel_events = []    # (first, count, start, end, stream): HIP events around each path-loop launch (timings only)
        self.retry = []            # positions (caller order) of the labels whose scratch overflowed

    def mark(self, name):
        if self.o.timings is not None:
            self.eng.sync_stream()
            self.o.timings.append((name, time.perf_counter()))

    def allocate_inputs(self):
        """task records, voxel lists, neighbour masks and the work lists; then the two fields the searches fill"""
        t, eng, lib, p, b, P = self.t, self.eng, self.lib, self.p, self.b, Engine.ptr
        sx, sy, sz = self.shape
        host = lambda a: t.from_numpy(a).to(eng.device)
        b["tasks"] = host(p.tasks.view(np.uint8).reshape(-1))
        b["slot"] = host(p.slot_of_label)
        b["off"] = host(p.list_off.astype(np.uint32).view(np.int32))
        b["cur"] = eng.empty(self.nl, t.int32)
        b["lists"] = eng.empty(max(p.total, 1), t.int32)
        b["tgt"] = host(p.tgt_arr.view(np.int32))
        b["nbr"] = eng.empty(self.nvox, t.int32)
        b["queues"] = eng.empty(4 * int(p.qcap.sum()), t.int32)
        b["qstate"] = t.zeros(self.nvox + 4, dtype=t.uint8, device=eng.device)
        self.mark("setup")
        _abi.check(lib.kh_scatter_lists(P(self.d_cc), self.label_bytes, self.nvox, P(b["slot"]), self.nl, P(b["off"]), P(b["cur"]),
                                        P(b["lists"]), self.st))
        _abi.check(lib.kh_neighbor_mask(P(self.d_cc), self.label_bytes, sx, sy, sz, P(b["nbr"]), self.st))
        b["gate"] = None
        if self.o.voxel_graph is not None:
            # voxel_graph= of kimimaro.trace.trace (a u32 device volume, cc3d's bit layout): the directions a voxel's word does not
            # allow leave the masks every search and the invalidation work from; gate = the corner entries at the x faces
            b["gate"] = t.zeros(self.nvox + 4, dtype=t.uint8, device=eng.device)
            _abi.check(lib.kh_apply_voxel_graph(P(b["nbr"]), P(self.o.voxel_graph), self.nvox, P(b["gate"]), self.st))
        self.mark("lists+nbrmask")
        b["ldaf"] = eng.empty(max(p.total, 1), t.float32)
        b["pdrf"] = eng.empty(self.nvox + 4, t.float32)

    def allocate_path_scratch(self):
        """the path loop's own volumes and per-label scratch (after the batch searches: their DAF volume's block is free again)"""
        t, eng, lib, p, b, P = self.t, self.eng, self.lib, self.p, self.b, Engine.ptr
        nvox = self.nvox
        b["dist"] = eng.empty(nvox + 4, t.float32)     # (+ padding: the searches read rows of three words)
        _abi.check(lib.kh_fill_f32(P(b["dist"]), nvox + 4, float("inf"), self.st))
        b["alive"] = eng.empty(nvox, t.uint8)
        _abi.check(lib.kh_init_alive(P(self.d_cc), self.label_bytes, nvox, P(b["slot"]), P(b["alive"]), self.st))
        if p.use_pool:
            b["heap"] = eng.empty(2 * p.pool_nodes, t.int64)   # 16-byte nodes; node 0 = {handed out, capacity}
            b["heap"][:2] = t.from_numpy(np.array([1, p.pool_nodes, 0, 0], dtype=np.uint32).view(np.int64)).to(eng.device)
        else:
            b["heap"] = eng.empty(2 * int(p.hcap.sum()), t.int64)  # 16-byte nodes
        b["cstate"] = t.zeros(nvox if p.sweep_on else 1, dtype=t.int64, device=eng.device)
        b["sched"] = eng.sched_volume(nvox) if p.sweep_on else None
        b["arena"] = eng.empty(max(p.ev_total, 1) * 32 + 32, t.int64)   # units of 256 bytes, 256-byte aligned start
        self.arena_ptr = C.c_void_p((b["arena"].data_ptr() + 255) & ~255)
        b["pverts"] = eng.empty(int(p.pcap.sum()), t.int32)
        b["plens"] = eng.empty(int(p.pcap.sum()), t.int32)
        # ghosts: the journal of the voxels that changed since the call that made the first ghost (2 entries per voxel of a
        # label at most: made a ghost, killed) and the weights the path vertices had before they became rails
        self.use_ghosts = eng.ghosts and p.sweep_on
        b["journal"] = eng.empty(2 * int(p.qcap.sum()), t.int32) if self.use_ghosts and not p.use_pool else None
        b["psave"] = eng.empty(int(p.pcap.sum()), t.float32) if self.use_ghosts and self.o.fix_branching else None
        if os.environ.get("KH_DEBUG_ALLOC") == "1":      # developer knob: where every array of this call lives (to place a fault address)
            for name, tt in list(b.items()) + [("dbf", self.d_dbf), ("cc", self.d_cc)]:
                if tt is not None:
                    print("KHALLOC %-8s %#x .. %#x (%d B)" % (name, tt.data_ptr(), tt.data_ptr() + tt.numel() * tt.element_size(),
                                                             tt.numel() * tt.element_size()), file=sys.stderr, flush=True)

    def searches(self, first, count):
        """find_root + DAF + PDRF of the task slots [first, first + count) as batch launches on the current stream"""
        if count <= 0:
            return
        if self.d_field is None:
            self.d_field = self.eng.empty(self.nvox + 4, self.t.float32)
        self._batch_searches(first, count, self.d_field)
        if not self.o.return_fields:
            self.d_field = None     # the DAF lives on in list order (ldaf); its volume goes back to the pool

    def _batch_searches(self, first, count, d_field):
        t, eng, lib, p, b, P, st = self.t, self.eng, self.lib, self.p, self.b, Engine.ptr, self.st
        (sx, sy, sz), (wx, wy, wz), nvox, expo = self.shape, self.w, self.nvox, self.params["pdrf_exponent"]
        tasks_ptr = C.c_void_p(b["tasks"].data_ptr() + first * _abi.LABEL_T.itemsize)
        lo = int(p.list_off[first])
        n_list = int(p.cnt[first:first + count].sum())
        lists_ptr = C.c_void_p(b["lists"].data_ptr() + 4 * lo)
        ldaf_ptr = C.c_void_p(b["ldaf"].data_ptr() + 4 * lo)
        d_slot_use, keep = b["slot"], 0
        if first > 0 or first + count < self.nl:
            # only these labels: the others' voxels are left alone (they are another launch's business)
            sl = p.slot_of_label.copy()
            sl[p.tasks["segid"][:first]] = -1
            sl[p.tasks["segid"][first + count:]] = -1
            d_slot_use, keep = t.from_numpy(sl).to(eng.device), _abi.PDRF_KEEP_OTHERS
        # find_root (trace.py:291-308) then DAF (trace.py:139-145)
        for mode, name in ((1, "edf_root"), (2, "edf_daf")):
            _abi.check(lib.kh_edf_batch(tasks_ptr, count, eng.edf_mode(mode), P(b["lists"]), P(b["nbr"]), sx, sy, sz, wx, wy, wz,
                                        P(d_field), P(b["qstate"]), P(b["queues"]), st))
            self.mark(name)
        _abi.check(lib.kh_gather_f32(P(d_field), lists_ptr, n_list, ldaf_ptr, st))
        # PDRF (trace.py:148)
        pdrf_call = lambda stage: _abi.check(lib.kh_pdrf(P(self.d_cc), self.label_bytes, nvox, P(d_slot_use), P(b["tasks"]), P(self.d_dbf),
                                                         P(d_field), stage | keep if stage >= 0 else stage,
                                                         np.float32(self.params["pdrf_scale"]), P(b["pdrf"]), st))
        if _abi.is_pow2_exponent(expo):
            pdrf_call(int(expo).bit_length() - 1)          # repeated squaring, trace.py:343-345
        else:
            # trace.py:346-347: np.power.  Its rounding is the host numpy's (libm / SVML powf), which no device powf can
            # promise, so exactly that function is applied -- by numpy itself -- between the two device halves.
            # Only the selected labels' voxels make the trip (their list is on the device already): gathered into a compact
            # array, raised on the host, scattered back -- 8 B per foreground voxel instead of 8 B per voxel of the volume.
            pdrf_call(_abi.PDRF_BASE)
            d_base = eng.empty(max(p.total, 1), t.float32)
            _abi.check(lib.kh_gather_f32(P(b["pdrf"]), P(b["lists"]), p.total, P(d_base), st))
            base = d_base[:p.total].cpu().numpy()
            with np.errstate(all="ignore"):
                np.power(base, expo, out=base)
            idx = b["lists"][:p.total].to(t.int64) & 0xFFFFFFFF       # u32 linear indices kept in an int32 tensor
            b["pdrf"].index_copy_(0, idx, t.from_numpy(base).to(eng.device))
            pdrf_call(_abi.PDRF_FINISH)
        self.mark("pdrf")

    def launch(self, first, count, stream, tstream=None, big=False, fused=False):
        """the path loop of the task slots [first, first + count) on `stream` (tstream: its torch object, for the HIP events)"""
        t, eng, b, P, O = self.t, self.eng, self.b, Engine.ptr, Engine.optr
        (sx, sy, sz), (wx, wy, wz), rdims = self.shape, self.w, self.rdims
        tasks_ptr = C.c_void_p(b["tasks"].data_ptr() + first * _abi.LABEL_T.itemsize)
        flags = eng.trace_flags(self.use_ghosts, self.p.use_pool, b["gate"] is not None, big=big, fused=fused)
        if self.timed:
            tstream = tstream if tstream is not None else t.cuda.current_stream(eng.device)
            ev0, ev1 = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
            ev0.record(tstream)
            self.kernel_events.append((first, count, ev0, ev1, tstream))
        _abi.check(self.lib.kh_trace_paths(tasks_ptr, count, P(b["lists"]), P(b["ldaf"]), P(b["nbr"]), sx, sy, sz, wx, wy, wz,
                                           P(self.d_dbf), P(b["pdrf"]), P(b["dist"]), P(b["alive"]), P(b["qstate"]), P(b["tgt"]),
                                           np.float32(self.params["scale"]), np.float32(self.params["const"]), P(b["queues"]),
                                           P(b["heap"]), P(b["pverts"]), P(b["plens"]), O(self.d_rank), rdims[0], rdims[1], rdims[2],
                                           self.p.max_nlev, P(b["cstate"]), eng.sched_ptr(b["sched"]), self.arena_ptr, O(b["journal"]),
                                           O(b["psave"]), O(b["gate"]), flags, int(bool(self.o.fix_branching)), stream))
        if self.timed:
            ev1.record(tstream)

    def kernel_times(self):
        """milliseconds of each path-loop launch of this call, from HIP events on the launch's own stream"""
        ke = self.kernel_events
        self.eng.last_path_kernel_ms = [(c, e0.elapsed_time(e1)) for _, c, e0, e1, _ in ke]
        # the span of the path phase: first start to last end over the (overlapped) launches of this call
        first = min(ke, key=lambda k: -min(k[2].elapsed_time(o[2]) for o in ke))[2] if ke else None
        self.eng.last_path_span_ms = max((first.elapsed_time(e1) for _, _, _, e1, _ in ke), default=0.0) if first else 0.0

    def collect(self, lo, hi):
        """results of task slots [lo, hi) (device -> host on the current stream)."""
        t, eng, b, P = self.t, self.eng, self.b, Engine.ptr
        isz = _abi.LABEL_T.itemsize
        part = b["tasks"][lo * isz:hi * isz].cpu().numpy().view(_abi.LABEL_T).copy()
        overflow = (part["status"] & 7) != 0          # work list / heap / path buffer too small: traced again (Engine._trace_group)
        bad = np.flatnonzero((part["status"] & ~np.uint32(7)) != 0)
        if bad.size or (overflow.any() and self.o.scratch_scale >= 64):
            s = int(bad[0]) if bad.size else int(np.flatnonzero(overflow)[0])
            raise _abi.KimiHipError("label %d (cc id): %s" % (int(part["segid"][s]),
                                                               _abi.describe_status(int(part["status"][s]))))
        for s in np.flatnonzero(overflow):
            self.retry.append(int(self.p.order[lo + s]))
            part["n_vertices"][s] = 0
            part["n_paths"][s] = 0
        # gather the used part of the path buffers: build a flat index on the host (small), gather on device
        nverts = part["n_vertices"].astype(np.int64)
        npaths = part["n_paths"].astype(np.int64)
        p_off = self.p.p_off[lo:hi].astype(np.int64)
        d_vidx = t.from_numpy(ranges(p_off, nverts)).to(eng.device)
        d_lidx = t.from_numpy(ranges(p_off, npaths)).to(eng.device)
        verts_dev = b["pverts"][d_vidx]
        verts = verts_dev.cpu().numpy().view(np.uint32)
        lens = b["plens"][d_lidx].cpu().numpy().view(np.uint32)
        d_radii = eng.empty(max(verts.size, 1), t.float32)
        if verts.size:
            _abi.check(self.lib.kh_gather_f32(P(self.d_dbf), P(verts_dev.contiguous()), verts.size, P(d_radii), eng.stream()))
        radii = d_radii.cpu().numpy()[: verts.size]
        return {"order": self.p.order[lo:hi], "tasks": part, "verts": verts, "radii": radii, "lens": lens,
                "voff": np.concatenate([[0], np.cumsum(nverts)]), "loff": np.concatenate([[0], np.cumsum(npaths)])}

    def split_schedule(self, n_large, who, sink):
        """The largest labels are the head of the run.  They go to a second stream (as large-LDS workgroups); the rest runs
        on the caller's stream and its results are copied back and handed to `sink` (the Skeleton assembly on the host)
        while the big labels are still being traced.  Returns the task records of all labels."""
        t, eng, nl = self.t, self.eng, self.nl
        cur = t.cuda.current_stream(eng.device)
        if eng._side is None:
            eng._side = t.cuda.Stream(device=eng.device)
        side = eng._side
        side.wait_stream(cur)
        self.launch(0, n_large, C.c_void_p(side.cuda_stream), side, big=(who != "early"), fused=(who != "before"))
        try:
            if who == "early":
                self.searches(n_large, nl - n_large)
            self.launch(n_large, nl - n_large, self.st, fused=(who == "fused"))
            small = self.collect(n_large, nl)
            sink(small)                     # overlaps the big labels' kernel: no device-wide sync in here
        finally:
            cur.wait_stream(side)           # the scratch of this call must outlive the side stream's kernel
            if sys.exc_info()[0] is not None:
                side.synchronize()
        big = self.collect(0, n_large)
        self.mark("paths")
        if self.timed:
            self.kernel_times()
        sink(big)
        self.mark("d2h")
        return np.concatenate([big["tasks"], small["tasks"]])

    def single_schedule(self, who, sink):
        """all labels in one launch on the caller's stream, behind the path gate.  Returns their task records."""
        eng = self.eng
        if eng.path_gate is not None and self.o.streaming:
            eng.sync_stream()
            eng.path_gate()
        self.launch(0, self.nl, self.st, fused=(who == "fused"))
        self.mark("paths")
        res = self.collect(0, self.nl)                  # (its device -> host copies wait for the launch)
        if self.timed:
            self.kernel_times()
        self.mark("d2h")
        sink(res)
        return res["tasks"]
