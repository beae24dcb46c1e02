"""The launch plan of the per-label pipeline as pure numpy: which labels go into which launch, every label's slice of the shared
scratch buffers, the task records' input fields, the targets table, the sweep's levels and event arena.

Nothing here touches the device (no torch, no call into libkimi_hip.so), so every rule -- the 32-bit guards, the window cap, the
pool size, the scratch_scale / scratch_divisor / arena_divisor arithmetic -- can be checked on numbers alone; kimimaro_amd.engine
allocates and launches what this module plans.
"""
from __future__ import annotations

import os
from types import SimpleNamespace
from typing import NamedTuple

import numpy as np

from ._abi import LABEL_T, SWEEP_LDS_LEVELS, is_pow2_exponent

# per-label scratch of the path loop as plan_launches books it: work lists 16 B per voxel, heap 24, event arena ~24, voxel list and DAF
# 8, ghost journal 8, path buffers and saved rail weights ~6 = 86 B, booked as 110; + the fixed parts of a small label (a 32 768-node
# heap, the arena's level chunks, 64 Ki path slots).  Round 2 booked 300 B per voxel (28 GB of event arena per c3 volume then):
# c5 ran as three launches one after the other, 12.4 s of paths; as one launch it is 91 -> ~200 GB of HBM and half the time.
SCRATCH_BYTES_PER_VOXEL = 60        # round 6: voxel list + DAF 8, work lists 16, the pool's share of heap and journal ~5, path buffers ~1,
SCRATCH_BYTES_PER_LABEL = 3 << 19    # booked with slack; per label: the event arena (1.25 x the level window + 320 chunks: 0.6-1.4 MB)
# Round 6: heap and ghost journal come out of one pool per launch, on demand (KH_TRACE_SCRATCH_POOL): this fraction of what all
# labels together could ask for (c3: 141 of 3 402 labels ever run the heap emulation -- 6 % of the nodes --, 360 ever hold a ghost);
# a label the pool cannot serve is traced again with scratch of its own, like every other overflow
SCRATCH_POOL_FRACTION = float(os.environ.get("KH_SCRATCH_POOL_FRACTION", "0.15"))


def plan_launches(counts, budget):
    """Groups of label positions for successive launches of the path loop: largest labels first, a group is closed when the
    next label's scratch (SCRATCH_BYTES_PER_VOXEL per voxel + SCRATCH_BYTES_PER_LABEL) would take it over `budget` bytes; a label
    larger than the budget gets a launch of its own.  One group = everything fits."""
    counts = np.asarray(counts, dtype=np.int64)
    need = counts * SCRATCH_BYTES_PER_VOXEL + SCRATCH_BYTES_PER_LABEL
    if int(need.sum()) <= budget:
        return [list(range(len(counts)))]
    groups, cur, acc = [], [], 0
    for i in np.argsort(-counts, kind="stable").tolist():
        if cur and acc + int(need[i]) > budget:
            groups.append(cur)
            cur, acc = [], 0
        cur.append(i)
        acc += int(need[i])
    groups.append(cur)
    return groups


SCHED_LEVELS = (1 << 17) - 1     # SW_SCHED_LEVELS (csrc/sweep.h): labels with more levels run the sweep unfiltered


def plan_arena(cnt, nlev, filtered, window=None):
    """(log2 slots per chunk, chunks) of the sweep's event arena per label (numpy arrays; csrc/sweep.h: fixed-size chunks of
    8-byte events chained per level; the chunks of a level go back to a free stack when the level has been processed).
    Unfiltered a voxel is handed ~13 events per call; with the pending-deadline filter ~2 (measured at c3: 1.72e9 -> 2.8e8
    events per volume), and a level of a large call holds tens of events instead of hundreds -- smaller chunks, a fraction of
    the event budget.  What has to fit is what is PENDING at one time: one partly filled chunk per level that has events
    (at most `window` levels when the label has a level window, never more levels than the label can get events) plus the
    pending events themselves.  An arena that runs out makes the call fall back to the heap emulation (SW_BAIL_ARENA in
    stat_sweep_why): a matter of speed, not of results."""
    cnt = np.asarray(cnt, dtype=np.int64)
    nlev = np.asarray(nlev, dtype=np.int64)
    filt = np.asarray(filtered, dtype=bool) & (nlev <= SCHED_LEVELS)
    shift = np.where(filt, np.where(cnt >= 65536, 6, 5), np.where(cnt >= 32768, 7, 6)).astype(np.int64)
    per_voxel = np.where(filt, 3, 14)
    levels = np.where(filt, np.minimum(nlev, 3 * cnt + 64), nlev)
    if window is not None:
        window = np.asarray(window, dtype=np.int64)
        levels = np.where(window > 0, np.minimum(levels, window), levels)
    chunks = levels + levels // 2 + ((per_voxel * cnt) >> shift) + 320
    if window is not None:
        # Round 6, measured on c3 (`cyc_push` of the task records = most chunks a label ever had in use): 0.41 x the window on average,
        # 0.94 x at the 99th percentile, 1.21 x at most -- the chunks of a level go back to the label's free stack when the level is
        # done, so what is in use is what is PENDING, and that is bounded by the window, not by the label's size.  The arena was
        # 6.9 GB per c3 volume for 0.55 GB of use, and the volumes in flight are bounded by memory.
        chunks = np.where(window > 0, np.minimum(chunks, window + window // 4 + 320), chunks)
    chunks = np.minimum(chunks, (1 << 20) - 2)    # 20-bit chunk ids (SW_NOCHUNK)
    return shift, chunks


def plan_spill(cnt):
    """entries (a power of two) of the sweep's candidate-spill table per label (csrc/sweep.h: the fifth to eighth possible
    owner of a voxel; 12 bytes per entry at the front of the label's arena).  Few voxels ever need one -- five in the label
    of c3 whose longest call used to be abandoned for them -- so the table is small: Nf / 64, between 256 and 16384 entries."""
    cnt = np.maximum(np.asarray(cnt, dtype=np.int64), 1)
    return 2 ** np.clip(np.ceil(np.log2(cnt / 64.0)), 8, 14).astype(np.int64)


def arena_units(chunks, shift, spill):
    """256-byte units of a label's arena: [spill table: 12 B per entry][free stack: 4 B per chunk][chunks of 8-byte slots]"""
    return (spill * 12 + 255) // 256 + (chunks * 4 + 255) // 256 + ((chunks * 8) << shift) // 256


def level_windows(keys, anisotropy, nlev, lds_levels):
    """kh_label_t.lev_window per label (numpy u32): a power of two above the number of levels an event can lie ahead of the
    level being processed, or 0 when that does not fit `lds_levels` words.  An event's key is the distance of a 26-neighbour
    of the processed voxel from a source whose key of that voxel is not above the current one, so it exceeds the current key
    by one step (the longest neighbour offset) at most: the bound is the largest number of distinct keys in such an interval
    over the label's levels, taken from the sorted key table itself (+ slack for the keys' own rounding)."""
    keys = np.asarray(keys, dtype=np.float64)
    nlev = np.asarray(nlev, dtype=np.int64)
    if keys.size == 0:
        return np.zeros(nlev.shape, dtype=np.uint32)
    step = float(np.sqrt(sum(float(np.float32(a)) ** 2 for a in anisotropy)))
    ahead = np.searchsorted(keys, (keys + step) * (1.0 + 1e-6) + 1e-6, side="right") - 1 - np.arange(keys.size)
    worst = np.maximum.accumulate(ahead)                         # worst[i] = most levels ahead over levels 0..i
    w = worst[np.clip(nlev - 1, 0, keys.size - 1)] + 2
    win = np.maximum(64, 2 ** np.ceil(np.log2(np.maximum(w, 1))).astype(np.int64))
    return np.where((nlev > 0) & (win <= int(lds_levels)), win, 0).astype(np.uint32)


def int_key_mode(anisotropy, rmax):
    """(gq, gx, gy, gz) of the sweep's INTEGER levels (csrc/sweep.h) for balls up to `rmax`, or None when the table of ranks
    has to serve.  With an integral anisotropy the flood's key of an offset (a, b, c) is sqrtf of the exact integer
    T = (wx a)^2 + (wy b)^2 + (wz c)^2 as long as T < 2^24 (every product and partial sum is an integer below 2^24: no rounding
    before the square root), and T = gq * S with gq = gcd(wx^2, wy^2, wz^2), S = gx a^2 + gy b^2 + gz c^2.  sqrtf is monotone; two
    values of T that differ lie at least gq apart, i.e. their roots gq / (2 sqrt T) apart, which exceeds an ulp of sqrt T
    (<= sqrt T * 2^-23) while T < gq * 2^22 -- taken with a factor two of margin.  Then S orders the keys and tells equal ones exactly as
    the floats do, for every offset the sweep evaluates: the voxels of a ball and their neighbours (one step further out)."""
    w = [float(np.float32(a)) for a in anisotropy]
    if any(v < 1.0 or v != int(v) or v > 4096.0 for v in w) or not np.isfinite(rmax) or rmax <= 0:
        return None
    q = [int(v) * int(v) for v in w]
    gq = int(np.gcd.reduce(q))
    step = float(np.sqrt(sum(q)))
    tmax = (float(rmax) + step) ** 2 * (1.0 + 1e-6)
    if tmax >= 2.0 ** 24 or tmax >= gq * 2.0 ** 21:
        return None
    return gq, q[0] // gq, q[1] // gq, q[2] // gq


def int_levels(anisotropy, gq, rmax, lds_levels):
    """per label (numpy arrays over `rmax`): the number of integer levels a ball of that radius can touch and the level window
    (a power of two above the number of levels an event can lie ahead of the level being processed, 0 when that does not fit
    `lds_levels` words).  An event's level is S of a 26-neighbour of the processed voxel from a source whose key of that voxel is
    not above the current one: at most ((d + step)^2 - d^2) / gq levels ahead for d up to the radius."""
    rmax = np.asarray(rmax, dtype=np.float64)
    w = [float(np.float32(a)) for a in anisotropy]
    step = float(np.sqrt(sum(v * v for v in w)))
    ok = np.isfinite(rmax) & (rmax > 0)
    r = np.where(ok, rmax, 0.0)
    nlev = np.where(ok, np.floor(r * r * (1.0 + 1e-6) / gq) + 2, 0).astype(np.int64)
    ahead = np.ceil((2.0 * r * step + step * step) * (1.0 + 1e-6) / gq) + 2
    win = np.maximum(64, 2 ** np.ceil(np.log2(np.maximum(ahead, 1))).astype(np.int64))
    return nlev, np.where(ok & (win <= int(lds_levels)), win, 0).astype(np.int64)


# -- the labels of one call ----------------------------------------------------------------------------------------------------
class LabelSet:
    """The connected components one run_labels call traces, as columns indexed by position: segid, count, dbf_max,
    first_index, xmin, xmax, root (a linear index or 0xFFFFFFFF: the search finds it); targets_before / targets_after: a list of
    linear indices per label (LIFO stacks as in kimimaro/trace.py:225-228) or None; soma: None or a dict of columns
    (soma_mode, fsr, soma_radius, soma_scale, soma_const)."""
    SOMA_COLUMNS = ("soma_mode", "fsr", "soma_radius", "soma_scale", "soma_const")

    def __init__(self, segid, count, dbf_max, first_index, xmin, xmax, root, targets_before=None, targets_after=None, soma=None):
        self.segid = np.asarray(segid, dtype=np.int64)
        self.count = np.asarray(count, dtype=np.int64)
        self.dbf_max = np.asarray(dbf_max, dtype=np.float32)
        self.first_index = np.asarray(first_index)
        self.xmin = np.asarray(xmin)
        self.xmax = np.asarray(xmax)
        self.root = np.asarray(root, dtype=np.uint32)
        self.targets_before = targets_before
        self.targets_after = targets_after
        self.soma = None if soma is None else {k: np.asarray(v) for k, v in soma.items()}

    def __len__(self):
        return len(self.segid)

    def take(self, idx):
        """the labels at positions `idx`, in that order"""
        idx = np.asarray(idx, dtype=np.int64)
        pick = lambda a: None if a is None else [a[i] for i in idx]
        return LabelSet(self.segid[idx], self.count[idx], self.dbf_max[idx], self.first_index[idx], self.xmin[idx], self.xmax[idx],
                        self.root[idx], pick(self.targets_before), pick(self.targets_after),
                        None if self.soma is None else {k: v[idx] for k, v in self.soma.items()})


class LabelStats(NamedTuple):
    """What kh_label_stats computes per component id 0..n, as host columns: counts, first_index, xmin, xmax (u32), dbf_max (f32) and
    yz (u32 [n + 1, 4]: ymin, ymax, zmin, zmax).  An id without a voxel keeps the identities of the minima and maxima."""
    counts: np.ndarray
    dbf_max: np.ndarray
    first_index: np.ndarray
    xmin: np.ndarray
    xmax: np.ndarray
    yz: np.ndarray

    def bbox(self, label):
        """((x0, y0, z0), (x1, y1, z1)), half open, of a label that has voxels: scipy.ndimage.find_objects (kimimaro/utility.py:85-102)"""
        y0, y1, z0, z1 = (int(v) for v in self.yz[label])
        return (int(self.xmin[label]), y0, z0), (int(self.xmax[label]) + 1, y1 + 1, z1 + 1)


def label_order(counts):
    """task slots: big labels first (their workgroups start first), ties in the caller's order"""
    return np.argsort(-np.asarray(counts, dtype=np.int64), kind="stable")


def sweep_radii(dbf_max, params):
    """largest ball radius of each label's invalidations: scale * dbf_max + const in f32 operations, as pyx:393-395"""
    return (np.float32(params["scale"]) * np.asarray(dbf_max, dtype=np.float32) + np.float32(params["const"])).astype(np.float32)


def _exclusive(cap):
    """exclusive prefix sum (int64): where each label's slice of a shared buffer starts"""
    return np.concatenate([[0], np.cumsum(cap)[:-1]]).astype(np.int64)


def plan_sweep(cnt, rmax_t, lv, *, window_cap=0, window_cap_always=False, arena_divisor=1, lds_levels=SWEEP_LDS_LEVELS,
               keep_unfit=False):
    """The sweep fields of the task records and the layout of the event arena, for labels of `cnt` voxels with largest ball radii
    `rmax_t` (f32) and the level arguments `lv` of Engine.sweep_levels (dict(nlev, win, ok, ...) or None: no label can use the
    sweep).  Returns per label nlev, sweep_rmax, ev_offset (256-byte units), ev_chunks, ev_shift, ev_spill, lev_window, and
    ev_total (units), max_nlev (LDS words of the neediest label), sweep_on.
    A label whose levels fit neither a window nor LDS runs on the heap emulation only (the kernel decides the same): it gets no
    arena and no spill table -- unless `keep_unfit`, the record of Engine.single_object, which books both all the same."""
    cnt = np.asarray(cnt, dtype=np.int64)
    zero = np.zeros(cnt.shape, dtype=np.int64)
    out = SimpleNamespace(nlev=zero, sweep_rmax=np.zeros(cnt.shape, dtype=np.float32), ev_offset=zero, ev_chunks=zero, ev_shift=zero,
                          ev_spill=zero, lev_window=zero, ev_total=0, max_nlev=0, sweep_on=False)
    if lv is None or not cnt.size or int(lv["nlev"].max()) <= 0:
        return out
    nlev, win, ok = lv["nlev"], lv["win"], lv["ok"]
    if window_cap and (window_cap_always or np.count_nonzero(win > int(window_cap)) <= max(1, int(0.005 * win.size))):
        # (only when few labels pay for it: a capped label's widest calls are redone by the heap emulation)
        win = np.where(win > 0, np.minimum(win, int(window_cap)), win)
    # fixed-size event chunks, chained per level (csrc/sweep.h): what is pending at one time
    shift, chunks = plan_arena(cnt, nlev, True, win)
    chunks = np.maximum(chunks // int(arena_divisor), 8)
    in_lds = (win > 0) | (nlev <= lds_levels)   # the others: heap emulation only
    booked = (nlev > 0) & (in_lds | bool(keep_unfit))
    # [spill table, 12 B per entry][(the free stack of rounds 4-5, 4 B per chunk: unused since round 6)][chunks]
    spill = plan_spill(cnt)
    units = np.where(booked, arena_units(chunks, shift, spill), 0)
    out.ev_total = int(units.sum())
    if out.ev_total >= 2 ** 32:
        raise ValueError("kimimaro_amd: event arena offsets exceed 32 bits; shard the labels")
    out.nlev = nlev
    out.sweep_rmax = np.where(ok, rmax_t, 0).astype(np.float32)
    out.ev_offset = _exclusive(units)
    out.ev_chunks = np.where(nlev > 0, chunks, 0)
    out.ev_shift = shift
    out.ev_spill = np.where(booked, spill, 0)
    out.lev_window = win
    out.max_nlev = int(np.where(win > 0, win, np.where(in_lds, nlev, 0)).max())     # LDS words each label wants
    out.sweep_on = True
    return out


SWEEP_FIELDS = ("nlev", "sweep_rmax", "ev_offset", "ev_chunks", "ev_shift", "ev_spill", "lev_window")


def plan_tasks(labels, params, lv, *, nlabels, order=None, rmax_t=None, max_paths=None, scratch_scale=1, scratch_divisor=1, scratch_pool=True,
               scratch_pool_fraction=SCRATCH_POOL_FRACTION, window_cap=0, window_cap_always=False, arena_divisor=1,
               lds_levels=SWEEP_LDS_LEVELS):
    """The launch plan of one path-loop launch over `labels` (a LabelSet, not empty): the task records with their input fields,
    every label's slice of the shared scratch buffers, the targets table, the sweep's arena (plan_sweep) and the heap pool.
    `lv`: what Engine.sweep_levels gave for the radii `rmax_t` = sweep_radii of the labels in slot order `order` = label_order
    (the caller hands over the two it asked with; computed here when absent), or None: no sweep.  `nlabels`: the largest
    component id of the volume.  Raises ValueError when an offset does not fit 32 bits."""
    nl = len(labels)
    order = label_order(labels.count) if order is None else order
    slot_of_label = -np.ones(nlabels + 1, dtype=np.int32)
    slot_of_label[labels.segid[order]] = np.arange(nl, dtype=np.int32)

    cnt = labels.count[order]
    total = int(cnt.sum())
    qcap = cnt + 64
    # heap / path scratch are sized for the common case; a label that overflows them is traced again on its own
    # with `scratch_scale` times as much -- the reference has no such limits
    # heap: 3 nodes per voxel for small labels, 1.5 per voxel + 4096 for the others (the deepest heap of c3's largest
    # label holds 0.7 nodes per voxel); never less than the sweep's lists need (11 / 8 nodes per voxel + 1536)
    hbase = np.maximum((3 * cnt) // 2 + 4096, np.minimum(3 * cnt + 2048, 32768))
    hcap = np.maximum(hbase * scratch_scale // scratch_divisor, 64)
    # path buffers: c3's labels write 527 vertices at most, 3 % of their voxels at most (round 5 kept 64 Ki entries for every label
    # above 16 Ki voxels: 2 GB per volume); a label that needs more is traced again with `scratch_scale` x 8
    pcap = np.maximum((cnt // 16 + 2048) * scratch_scale // scratch_divisor, 8)
    if max(total, int(qcap.sum()), int(hcap.sum()), int(pcap.sum())) >= 2 ** 32:
        raise ValueError("kimimaro_amd: scratch offsets exceed 32 bits; shard the labels")
    p = SimpleNamespace(order=order, slot_of_label=slot_of_label, cnt=cnt, total=total, qcap=qcap, hcap=hcap, pcap=pcap,
                        list_off=_exclusive(cnt), q_off=_exclusive(qcap), h_off=_exclusive(hcap), p_off=_exclusive(pcap),
                        jnodes=(2 * qcap + 3) // 4)                        # a label's ghost journal in 16-byte nodes
    # first attempt: heap and journal from a pool (SCRATCH_POOL_FRACTION); retries and test runs with shrunk scratch: slices
    p.use_pool = bool(scratch_pool and scratch_scale == 1 and scratch_divisor == 1 and nl >= 4)
    p.pool_nodes = 0
    if p.use_pool:
        frac = float(scratch_pool_fraction)
        need = hcap + p.jnodes
        p.pool_nodes = min(int(max(frac * float(need.sum()), (2 if frac >= 0.05 else 0) * float(need.max()))) + 1, 2 ** 32 - 2)

    tasks = p.tasks = np.zeros(nl, dtype=LABEL_T)
    tasks["segid"] = labels.segid[order]
    tasks["list_offset"] = p.list_off
    tasks["count"] = cnt
    tasks["xmin"] = labels.xmin[order]
    tasks["xmax"] = labels.xmax[order]
    tasks["source"] = labels.first_index[order]
    tasks["root"] = labels.root[order]
    f = np.float32
    dm = labels.dbf_max[order]
    # M = f32(1 / dbf_max ** 1.01) with numpy scalar semantics, kimimaro/trace.py:335-336
    tasks["M"] = np.array([f(1 / (f(v) ** 1.01)) if v > 0 else f(0) for v in dm], dtype=np.float32)
    tasks["q_offset"] = p.q_off
    tasks["q_capacity"] = qcap
    tasks["heap_offset"] = p.h_off
    tasks["heap_capacity"] = hcap
    tasks["path_offset"] = p.p_off
    tasks["path_capacity"] = pcap
    tasks["max_paths"] = 0 if max_paths is None else int(max_paths)
    if is_pow2_exponent(params["pdrf_exponent"]):     # KH_TRACE_FUSED_EDF: compute_pdrf's parameters travel with the task
        tasks["pdrf_log2e"] = int(params["pdrf_exponent"]).bit_length() - 1
        tasks["pdrf_scale"] = np.float32(params["pdrf_scale"])
    if labels.soma is not None:
        for key in LabelSet.SOMA_COLUMNS:
            tasks[key] = labels.soma[key][order]
    # order-free invalidation sweep: per-label event arenas
    sw = plan_sweep(cnt, sweep_radii(dm, params) if rmax_t is None else rmax_t, lv, window_cap=window_cap, window_cap_always=window_cap_always,
                    arena_divisor=arena_divisor, lds_levels=lds_levels)
    for key in SWEEP_FIELDS:
        tasks[key] = getattr(sw, key)
    p.ev_total, p.max_nlev, p.sweep_on = sw.ev_total, sw.max_nlev, sw.sweep_on      # (the per-label fields: in the records)
    tgt = []
    tgt_off = np.zeros(nl, dtype=np.int64)
    tb, ta = labels.targets_before, labels.targets_after
    for s, o in enumerate(order):
        tgt_off[s] = len(tgt)
        b = list(tb[o]) if tb is not None else []
        a = list(ta[o]) if ta is not None else []
        tasks["n_before"][s] = len(b)
        tasks["n_after"][s] = len(a)
        tgt.extend(b)
        tgt.extend(a)
    tasks["tgt_offset"] = tgt_off
    p.tgt_arr = np.asarray(tgt + [0], dtype=np.uint32)
    return p


# -- a dataset cut into chunks ---------------------------------------------------------------------------------------------------
class ChunkGrid(NamedTuple):
    """What chunk_grid returns: `grid` = chunks per axis; per chunk, x fastest, int64 [n, 3]: `grid_index` (its place in the grid), the half-open
    corners of its core (`core_lo`, `core_hi`) and of its box (`box_lo`, `box_hi`)."""
    grid: tuple
    grid_index: np.ndarray
    core_lo: np.ndarray
    core_hi: np.ndarray
    box_lo: np.ndarray
    box_hi: np.ndarray


def _axis_cuts(n, c, overlap):
    """(starts, core ends, box ends) of one axis of length n cut every c voxels"""
    starts = np.arange(0, max(n - overlap, 1), c, dtype=np.int64)
    core_hi = np.concatenate([starts[1:], [n]]).astype(np.int64)
    return starts, core_hi, np.minimum(starts + c + overlap, n)


def chunk_grid(shape, chunk_shape, overlap=1):
    """The chunks of a dataset of `shape` voxels as a ChunkGrid.  Per axis of length n with chunk length c the starts
    are 0, c, 2c, ... below n - overlap (0 alone when n <= overlap); the CORE of a start reaches to the next start, the last one to n:
    the cores partition the dataset.  The BOX of a start is [start, min(start + c + overlap, n)): the core plus `overlap` voxels on the
    high side, which are the first voxels of the next core -- both chunks see the same face there.  A trailing slab that would hold
    nothing but the previous box's overlap never becomes a chunk (n = 97, c = 48: boxes [0, 49) and [48, 97)).  An entry of
    chunk_shape may exceed n: one chunk, no overlap.  Two-axis shapes get a unit z axis.  ValueError: an entry that is not a
    positive integer, a negative overlap, a shape that has not two or three axes, a chunk_shape of another length than the shape
    (three entries are accepted for two axes)."""
    shape, chunk_shape = tuple(shape), tuple(chunk_shape)
    if len(shape) not in (2, 3):
        raise ValueError("chunk_grid: a dataset has two or three axes. Got: {}".format(shape))
    if len(chunk_shape) != len(shape) and len(chunk_shape) != 3:
        raise ValueError("chunk_grid: chunk_shape {} does not fit a dataset of shape {}".format(chunk_shape, shape))
    for v in shape + chunk_shape:
        if int(v) != v or int(v) <= 0:
            raise ValueError("chunk_grid: extents are positive integers. Got: {} / {}".format(shape, chunk_shape))
    if int(overlap) != overlap or int(overlap) < 0:
        raise ValueError("chunk_grid: overlap must be a non-negative integer. Got: {}".format(overlap))
    shape = tuple(int(v) for v in (shape + (1,))[:3])
    chunk_shape = tuple(int(v) for v in (chunk_shape + (1,))[:3])
    cuts = [_axis_cuts(n, c, int(overlap)) for n, c in zip(shape, chunk_shape)]
    grid = tuple(int(c[0].size) for c in cuts)
    kz, ky, kx = np.meshgrid(np.arange(grid[2]), np.arange(grid[1]), np.arange(grid[0]), indexing="ij")
    index = np.stack([kx.ravel(), ky.ravel(), kz.ravel()], axis=1).astype(np.int64)          # x fastest, then y, then z
    pick = lambda which: np.stack([cuts[ax][which][index[:, ax]] for ax in range(3)], axis=1).astype(np.int64)
    lo = pick(0)
    return ChunkGrid(grid, index, lo, pick(1), lo.copy(), pick(2))


def halo_boxes(shape, chunk_shape, halo):
    """The cores and boxes of cross_sectional_area_chunked -> (core_lo, core_hi, box_lo, box_hi), int64 [n, 3], half
    open, x fastest: the cores of chunk_grid(shape, chunk_shape, overlap=0), which partition the dataset, and per core its box: the
    core widened by `halo` voxels on all six sides, clamped to the dataset.  ValueError as chunk_grid, and for a negative halo."""
    if int(halo) != halo or int(halo) < 0:
        raise ValueError("halo_boxes: halo must be a non-negative integer. Got: {}".format(halo))
    grid = chunk_grid(shape, chunk_shape, overlap=0)
    extent = np.array((tuple(int(v) for v in shape) + (1,))[:3], dtype=np.int64)
    return grid.core_lo, grid.core_hi, np.maximum(grid.core_lo - int(halo), 0), np.minimum(grid.core_hi + int(halo), extent)


def core_of(vox, shape, chunk_shape):
    """vox (n, 3) integer voxels of a dataset of `shape` -> int64 [n]: the row of halo_boxes / chunk_grid(overlap=0) whose core holds
    each voxel, -1 for a voxel outside the dataset.  Two-axis shapes get a unit z axis."""
    vox = np.asarray(vox, dtype=np.int64).reshape(-1, 3)
    extent = np.array((tuple(int(v) for v in shape) + (1,))[:3], dtype=np.int64)
    chunk = np.array((tuple(int(v) for v in chunk_shape) + (1,))[:3], dtype=np.int64)
    inside = np.all((vox >= 0) & (vox < extent), axis=1)
    return np.where(inside, _raster((extent + chunk - 1) // chunk, vox // chunk), -1)


def _raster(grid, at):
    """the row, x fastest, of the chunk at grid position `at` (int64 [..., 3]) in a grid of `grid` chunks per axis"""
    return at[..., 0] + int(grid[0]) * (at[..., 1] + int(grid[1]) * at[..., 2])


def core_index(grid, at):
    """grid positions `at` (int [..., 3]) in a grid of `grid` chunks per axis (ChunkGrid.grid) -> int64 [...]: the row of that chunk
    -- the inverse of ChunkGrid.grid_index --, -1 for a position outside the grid"""
    at = np.asarray(at, dtype=np.int64)
    return np.where(np.all((at >= 0) & (at < np.asarray(grid, dtype=np.int64)), axis=-1), _raster(grid, at), -1)


def neighbor_cores(grid, steps):
    """int64 [chunks, len(steps)]: per chunk of the ChunkGrid `grid` the row of the chunk one step (dx, dy, dz) away in the grid, for each
    of `steps`; -1 where the grid ends"""
    return core_index(grid.grid, grid.grid_index[:, None, :] + np.asarray(steps, dtype=np.int64).reshape(1, -1, 3))


# -- which cores a nearest-voxel query has to look at (synapses_to_targets_chunked) ------------------------------
def box_distance_bounds(core_lo, core_hi, centroids):
    """float64 [n_cores, Q]: the distance from each centroid (f64 [Q, 3], dataset coordinates) to the nearest voxel CENTRE a core
    [core_lo, core_hi) could hold -- p = clip(c, lo, hi - 1), then kh_nearest_label_voxels_box's own expression
    sqrt((dx*dx + dy*dy) + dz*dz) with d = p - c, every operation rounded in float64.  For a voxel v of the core, |v - c| >= |p - c|
    per axis as reals (p is c itself or the end of the core's range on c's side), and subtraction, the square of a magnitude, the
    sum of non-negative terms and the root are all monotone when rounded: the bound is <= the distance the kernel computes for
    every voxel of the core AS FLOATS.  A query is skipped in a core only when bound > its best so far, strictly (an equal distance
    still competes on the index), so a skipped core cannot have changed the result.  A label that occurs nowhere never gets a
    best: its queries stay active in every core -- the whole-volume call, too, looks everywhere to learn that."""
    lo = np.asarray(core_lo, dtype=np.float64).reshape(-1, 1, 3)
    top = np.asarray(core_hi, dtype=np.float64).reshape(-1, 1, 3) - 1.0
    c = np.asarray(centroids, dtype=np.float64).reshape(1, -1, 3)
    dx, dy, dz = (np.clip(c[..., a], lo[..., a], top[..., a]) - c[..., a] for a in range(3))
    return np.sqrt((dx * dx + dy * dy) + dz * dz)


def nearest_first(bounds):
    """the visit order of the cores: ascending by a core's smallest bound over all queries, ties in raster order (stable) -- the
    cores that can hold a winner come first, which lets the rule above skip the others; the result does not depend on it"""
    bounds = np.asarray(bounds, dtype=np.float64)
    return np.argsort(bounds.min(axis=1) if bounds.shape[1] else np.zeros(bounds.shape[0]), kind="stable")
