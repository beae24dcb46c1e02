"""Skeleton segments for a dataset that is never resident as a whole, on the plumbing of kimimaro_amd.boxes (every public name is
kimimaro_amd.post's too):

    oversegment_chunked(dataset, skeletons, chunk_shape, ...)   the skeletons' segments, relaxed box by box
    shell_diff(old, now, core_lo, core_hi), DIRECTIONS          kh_box_shell_diff restated on host boxes
"""
import copy
import time

import numpy as np

from . import _abi, feature, ops, utility
from .boxes import (_load_box, _slices, axes, count_core, count_core_device, down, group_by_core, label_table, label_type, store_like,
                    up, upload_labels)
from .plan import chunk_grid, core_of, halo_boxes, neighbor_cores

# kh_neighbor_mask's directions: bit k of a mask is DIRECTIONS[k]
DIRECTIONS = tuple((dx, dy, dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dx, dy, dz) != (0, 0, 0))


def shell_diff(old, now, core_lo, core_hi):
    """kh_box_shell_diff on host boxes [x, y, z] of 32-bit words -> (directions towards which a changed core voxel lies in the core's
    outermost layer, as bits in DIRECTIONS' order; core voxels that changed; the largest finite non-negative f32 of the core of
    `now`, as bits)"""
    core = _slices(core_lo, core_hi)
    before, after = np.asarray(old)[core].view(np.uint32), np.asarray(now)[core].view(np.uint32)
    changed = before != after
    mask = 0
    if changed.any():
        for k, step in enumerate(DIRECTIONS):
            layer = changed
            for axis, d in enumerate(step):
                if d:
                    layer = np.take(layer, [0 if d < 0 else -1], axis=axis)
            if layer.any():
                mask |= 1 << k
    finite = after[after < 0x7F800000]
    return mask, int(changed.sum()), int(finite.max()) if finite.size else 0


def oversegment_chunked(dataset, skeletons, chunk_shape=(512, 512, 512), anisotropy=(1, 1, 1), progress=False, fill_holes=False,
                        in_place=False, downsample=0, distance_store=None, feature_store=None, timings=None, _box=None):
    """kimimaro_amd.oversegment for a dataset that is never resident as a whole.  The result is DEFINED as what
    oversegment(whole dataset, skeletons, anisotropy) returns, equal voxel for voxel: all_features numbered 1..K by first appearance
    in the Fortran raster of the DATASET, every skeleton's `segments` and extra_attributes entry, the deep copy and the container
    rules, the skip rules (id 0, label absent, label of one voxel in the whole dataset, vertex outside, vertex off its label, several
    vertices on one voxel), the tie rule (the smallest provisional number, numbers in container order) and the KimiHipError when a
    finite distance reaches 2^23 * min(anisotropy).  The dataset may hold 2^32 voxels or more, which oversegment refuses; only a box
    has to stay below that.  PARITY UNPINNED as oversegment.

    dataset: what skeletonize_chunked takes.  skeletons: a dict, a list or one Skeleton, vertices in DATASET coordinates (what
    skeletonize_chunked returns).  fill_holes=True and downsample > 0 raise NotImplementedError as in oversegment; progress and
    in_place have no effect.

    Multi-block relaxation: the cores of plan.halo_boxes(dataset.shape, chunk_shape, 1) partition the dataset, a box is its core
    widened by one voxel, so every CORE voxel has its true neighbour mask in its box.  Phase 1 (distances): every core starts
    dirty; a round visits the dirty cores in raster order; a visit loads the box's labels and its distances from the distance
    store (a core never written counts as +inf), places the core's seeds, runs kh_geodesic_relax to the box's fixpoint, writes the
    CORE back and marks dirty each neighbouring core towards which a changed voxel lies in the core's outermost layer
    (kh_box_shell_diff).  The phase ends when no core is dirty, never by a count.  Phase 2 (features) does the same with
    kh_feature_relax on the final distances and the feature store.  Two sweeps over the cores follow: the first appearances
    (kh_first_appearance_box), then the renumbering and the segments.

    distance_store, feature_store: array-likes of the dataset's shape (three axes), f32 and u32, indexed [x, y, z], read and written
    by slices only -- np.memmap, say.  Default: numpy arrays in host memory.  Either way they cost 8 BYTES PER VOXEL OF THE DATASET
    together.  A feature_store that was passed comes back as all_features, as u32; otherwise all_features is a numpy array of the
    smallest unsigned dtype that holds K with the dataset's own number of axes.  distance_store holds the final distances on return,
    +inf where no seed reaches.  ValueError for a store of another shape or dtype, and for a box of 2^32 voxels or more.
    timings (a dict) receives cores, distance_rounds, distance_visits, feature_rounds, feature_visits, boxes_loaded, voxels_loaded,
    load_s (host: loading from the dataset and the stores, upload, writing back), relax_ms (host milliseconds around the masks, the
    seeds, the sweeps and the diff of every visit, which end in a download), number_s (the two last sweeps) and segments (K).
    _box(labels_box, d_box, f_box, anisotropy, phase) -> the relaxed d_box (phase 1; f_box is None) or f_box (phase 2), on host
    arrays indexed [x, y, z]: runs the boxes instead of the kernels; the diff, the first appearances and the renumbering are then
    numpy and nothing touches the GPU (the host-logic tests).  Without it there is no CPU fallback: HipUnavailableError without the
    library or an MI355X, before anything is loaded."""
    utility._oversegment_check_arguments(downsample, fill_holes)
    eng = ops.engine() if _box is None else None         # raises HipUnavailableError without the library or a gfx950 device
    an = np.array(anisotropy, dtype=np.float32).reshape(-1)
    if an.shape != (3,) or not np.all(np.isfinite(an)) or not np.all(an > 0):
        raise ValueError("anisotropy must be three finite positive numbers")
    shape0, shape, _ = axes(dataset, "oversegment_chunked")
    core_lo, core_hi, box_lo, box_hi = halo_boxes(shape0, chunk_shape, 1)
    n_cores = int(core_lo.shape[0])
    box_voxels = [int(e[0]) * int(e[1]) * int(e[2]) for e in box_hi - box_lo]
    if max(box_voxels) >= 2 ** 32:
        raise ValueError("oversegment_chunked: a box of {} voxels does not fit the 32-bit indices of a volume".format(max(box_voxels)))
    _, is_bool, span = label_type(dataset)
    d_store = store_like(distance_store, shape, np.float32, "distance_store")
    f_store = store_like(feature_store, shape, np.uint32, "feature_store")

    # every vertex of every skeleton gets a provisional number in the container's order, as in oversegment
    skeletons = copy.deepcopy(skeletons)
    skels, labels_of, table, place = label_table(skeletons, is_bool, span)     # (a label outside the span occurs nowhere)
    vox_parts, word_parts = [np.zeros((0, 3), dtype=np.int64)], [np.zeros(0, dtype=np.int64)]
    for s, L in zip(skels, labels_of):
        vox = (np.asarray(s.vertices).reshape(-1, 3) / an).round().astype(np.int64)            # utility.py:610
        vox_parts.append(vox)
        word_parts.append(np.full(vox.shape[0], place.get(L, -1), dtype=np.int64))
        utility._add_property(s, utility.SEGMENTS_ATTRIBUTE)
    vox_all, word_all = np.concatenate(vox_parts), np.concatenate(word_parts)
    total = int(vox_all.shape[0])
    if total >= 2 ** 32 - 1:
        raise ValueError("fewer than 2^32 - 1 vertices in all")
    core_all = core_of(vox_all, shape, chunk_shape)
    active = (core_all >= 0) & (word_all >= 0)           # the vertices that may seed; single-voxel labels leave after phase 1

    inside = np.flatnonzero(core_all >= 0)
    verts_of = group_by_core(core_all[inside], inside)   # the vertices of every core, in ascending order
    near = neighbor_cores(chunk_grid(shape0, chunk_shape, overlap=0), DIRECTIONS)
    none = np.zeros(0, dtype=np.int64)
    counts = np.zeros(len(table), dtype=np.int64)        # voxels per label over the cores, from every core's first visit
    counted = np.zeros(n_cores, dtype=bool)
    core_top = np.zeros(n_cores, dtype=np.uint32)        # per core the largest finite distance, as bits
    total_t = dict(cores=n_cores, boxes_loaded=0, voxels_loaded=0, load_s=0.0, relax_ms=0.0)

    def read_store(store, k, written, fill):
        """the box of core k out of `store` as a Fortran-ordered copy; a core that was never written counts as `fill`, unread"""
        lo, hi = box_lo[k], box_hi[k]
        meets = np.flatnonzero(np.all((core_lo < hi) & (core_hi > lo), axis=1))
        if written[meets].all():
            return np.array(_load_box(store, lo, hi), dtype=store.dtype, order="F")
        box = np.full(tuple(int(v) for v in hi - lo), fill, dtype=store.dtype, order="F")
        for j in meets[written[meets]].tolist():
            a, b = np.maximum(core_lo[j], lo), np.minimum(core_hi[j], hi)
            box[_slices(a - lo, b - lo)] = _load_box(store, a, b)
        return box

    def visit(k, phase, written):
        """one visit of core k -> the directions (bits) whose neighbouring cores have to look again"""
        lo, hi = box_lo[k], box_hi[k]
        ext = tuple(int(v) for v in hi - lo)
        in_lo, in_hi = core_lo[k] - lo, core_hi[k] - lo
        inner = _slices(in_lo, in_hi)
        t0 = time.perf_counter()
        host = _load_box(dataset, lo, hi, "oversegment_chunked")
        total_t["boxes_loaded"] += 1
        total_t["voxels_loaded"] += box_voxels[k]
        mine = verts_of.get(k, none)
        mine = mine[active[mine]]
        local = vox_all[mine] - lo
        store, fill = (d_store, np.float32(np.inf)) if phase == 1 else (f_store, np.uint32(_abi.NO_FEATURE))
        old = read_store(store, k, written, fill)
        dist = read_store(d_store, k, np.ones(n_cores, dtype=bool), None) if phase == 2 else None
        if eng is None:
            if not counted[k]:
                count_core(host[inner], place, counts)
            now = old.copy()
            for i, (x, y, z) in zip(mine.tolist(), local.tolist()):
                if host[x, y, z] == table[word_all[i]]:                   # a vertex off its label seeds nothing
                    now[x, y, z] = 0 if phase == 1 else min(int(now[x, y, z]), i + 1)
            total_t["load_s"] += time.perf_counter() - t0
            t0 = time.perf_counter()
            now = np.asarray(_box(host, now, None, an, 1) if phase == 1 else _box(host, dist, now, an, 2), dtype=old.dtype)
            got = shell_diff(old, now, in_lo, in_hi)
        else:
            d_lab, label_bytes, device_word = upload_labels(eng, host, span, table)
            if not counted[k]:
                count_core_device(eng, d_lab, ext, inner, device_word, place, counts)
            words = np.array([device_word.get(table[w], 0) for w in word_all[mine].tolist()], dtype=np.int64)
            held = words != 0                                              # (renumbered labels: one this box does not hold)
            lin = (local[:, 0] + ext[0] * (local[:, 1] + ext[1] * local[:, 2]))[held].astype(np.uint32)
            d_old = up(eng, old)
            d_now = d_old.clone()
            d_dist = up(eng, dist) if phase == 2 else None
            total_t["load_s"] += time.perf_counter() - t0
            t0 = time.perf_counter()
            feature.seed_at(eng, d_lab, label_bytes, box_voxels[k], lin, (mine[held] + 1).astype(np.uint32), words[held].astype(np.uint32),
                            d_dist=d_now if phase == 1 else None, d_feat=d_now if phase == 2 else None)
            d_nbr = feature.neighbor_mask(eng, d_lab, label_bytes, ext)
            if phase == 1:
                feature.relax_box(eng, d_nbr, ext, an, d_now)
            else:
                feature.relax_box(eng, d_nbr, ext, an, d_dist, d_now)
            got = feature.box_shell_diff(eng, d_old, d_now, ext, in_lo, in_hi)
        total_t["relax_ms"] += (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        if got[1] or not written[k]:                                       # (a download is int32 words where the store holds u32)
            back = now[inner] if eng is None else down(d_now, ext, inner).view(old.dtype)
            store[_slices(core_lo[k], core_hi[k])] = back
        total_t["load_s"] += time.perf_counter() - t0
        counted[k] = written[k] = True
        if phase == 1:
            core_top[k] = got[2]
        return got[0]

    def relax(phase):
        """the rounds of one phase -> (rounds, visits).  The end is "no core is dirty"; the limit -- a round settles one more hop of
        every shortest path, which has fewer hops than the dataset has voxels -- only turns a defect into an error"""
        dirty, written = np.ones(n_cores, dtype=bool), np.zeros(n_cores, dtype=bool)
        rounds, visits, limit = 0, 0, shape[0] * shape[1] * shape[2] + 2
        while dirty.any():
            if rounds >= limit:
                raise _abi.KimiHipError("oversegment_chunked: phase %d has dirty cores after %d rounds over %d cores" % (phase, rounds, n_cores))
            rounds += 1
            for k in range(n_cores):                                      # raster order; a core made dirty further on is visited in this round
                if not dirty[k]:
                    continue
                dirty[k] = False
                towards = visit(k, phase, written)
                visits += 1
                woken = near[k, [bit for bit in range(len(DIRECTIONS)) if (towards >> bit) & 1]]
                dirty[woken[woken >= 0]] = True
        return rounds, visits

    distance_rounds, distance_visits = relax(1)
    # utility.py:141-154: a label of one voxel in the whole dataset is skipped.  Its voxel has an empty mask: nothing depends on it
    single = [w for w in range(len(table)) if counts[w] == 1]
    if single:
        for i in np.flatnonzero(active & np.isin(word_all, single)).tolist():
            v = vox_all[i]
            if _load_box(dataset, v, v + 1)[0, 0, 0] == table[word_all[i]]:
                d_store[_slices(v, v + 1)] = np.float32(np.inf)
            active[i] = False
    top = float(core_top.max(initial=0).view(np.float32)) if n_cores else 0.0
    if top >= float(np.float32(2 ** 23) * an.min()):
        raise _abi.KimiHipError("geodesic distances reach 2^23 steps of the smallest voxel pitch: float32 absorbs further steps")
    feature_rounds, feature_visits = relax(2)

    # the numbering: the smallest DATASET raster index of every provisional number, then 1..K in that order
    t0 = time.perf_counter()
    if eng is None:
        first = np.full(total + 1, np.iinfo(np.int64).max, dtype=np.int64)
    else:
        d_first = feature.first_appearance_table(eng, total)
    for k in range(n_cores):
        lo, hi = core_lo[k], core_hi[k]
        ext = tuple(int(v) for v in hi - lo)
        f = np.asarray(_load_box(f_store, lo, hi), dtype=np.uint32)
        if eng is None:
            index = (np.arange(lo[0], hi[0], dtype=np.int64)[:, None, None] + shape[0] * (
                np.arange(lo[1], hi[1], dtype=np.int64)[None, :, None] + shape[1] * np.arange(lo[2], hi[2], dtype=np.int64)[None, None, :]))
            valid = (f != 0) & (f <= total)
            np.minimum.at(first, f[valid].astype(np.int64), np.broadcast_to(index, f.shape)[valid])
        else:
            feature.first_appearance_box(eng, up(eng, f), ext, (0, 0, 0), ext, lo, shape[0], shape[1], total, d_first)
    if eng is None:
        first[first == np.iinfo(np.int64).max] = -1
    else:
        first = d_first.cpu().numpy()
    lut, K = feature.first_appearance_map(first)
    d_lut = None if eng is None else up(eng, lut)
    seg_all = np.zeros(total, dtype=np.uint64)
    for k in range(n_cores):
        lo, hi = core_lo[k], core_hi[k]
        ext = tuple(int(v) for v in hi - lo)
        f = np.asarray(_load_box(f_store, lo, hi), dtype=np.uint32)
        if eng is None:
            f = lut[np.where(f <= total, f, 0)]
        else:
            d_f = up(eng, f)
            feature.remap_u32(eng, d_f, d_lut, total, ext[0] * ext[1] * ext[2])
            f = down(d_f, ext, _slices((0, 0, 0), ext)).view(np.uint32)
        f_store[_slices(lo, hi)] = f
        mine = verts_of.get(k, none)
        local = vox_all[mine] - lo
        seg_all[mine] = f[local[:, 0], local[:, 1], local[:, 2]]           # utility.py:640-642
    at = 0
    for s, vox in zip(skels, vox_parts[1:]):
        s.segments = seg_all[at:at + vox.shape[0]].copy()
        at += vox.shape[0]
    number_s = time.perf_counter() - t0
    if timings is not None:
        timings.update(total_t, distance_rounds=distance_rounds, distance_visits=distance_visits, feature_rounds=feature_rounds,
                       feature_visits=feature_visits, number_s=number_s, segments=K)
    if feature_store is not None:
        return feature_store, skeletons
    # fastremap.renumber returns the smallest unsigned dtype that holds the largest new label
    out = f_store.astype(np.uint8 if K < 2 ** 8 else np.uint16 if K < 2 ** 16 else np.uint32)
    return out.reshape(shape0, order="F"), skeletons
