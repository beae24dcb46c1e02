"""Device plumbing of the point queries: the voxel of a label nearest to a centroid (kimimaro_amd.intake.synapses_to_targets) and
the edges of a binary image (kimimaro_amd.ops.extract_edges_from_binary_image), both csrc/points.hip, DESIGN.md 3.11, on
whole-volume arrays resident in HBM; and the nearest vertex pairs between the parts of skeleton groups (part_gaps) with the sets
of parts no such pair crosses (part_clusters): csrc/join.hip; kimimaro_amd.post.join_close_components_many.  The
library allocates nothing, the scratch is sized here."""
from __future__ import annotations

import time

import numpy as np

from . import _abi
from .volume import DimensionError, format_labels

NONE64 = 0xFFFFFFFFFFFFFFFF       # the "none" word of kh_nearest_label_voxels
MAX_EDGES = 2 ** 31
GAP_MAX_RECORDS = 1 << 26         # records (16 bytes each) of one kh_part_gaps call: 1 GiB of tables
GAP_MAX_PARTS = 8192              # ... which is one group of this many parts


def connectivity_directions(connectivity):
    """the directions of kh_neighbor_mask's words that skeletontricks.hpp:399-440 visits: the axis offsets always, the face
    diagonals for `connectivity > 6`, the corners for `connectivity > 18` (its own comparisons)"""
    connectivity = int(connectivity)
    if connectivity > 18:
        return 0x3FFFFFF
    if connectivity > 6:
        return 0x3FFFF
    return 0x3F


def nearest_label_voxels(eng, d_lab, label_bytes, shape, words, query_start, centroids):
    """d_lab: the label volume on the device (1-D, Fortran order, label_bytes 1 / 2 / 4 / 8); words: the distinct labels asked for as
    the unsigned words the volume holds, ascending (u64 host array); query_start: u32 [len(words) + 1]; centroids: f64 [Q, 3], the
    queries of words[k] at rows [query_start[k], query_start[k + 1]).  One call for all of them.  Returns the u64 host array [Q] of
    the winners' C-order indices x*sy*sz + y*sz + z, NONE64 for a label that does not occur."""
    t, P = eng.torch, eng.ptr
    sx, sy, sz = (int(v) for v in shape)
    words = np.ascontiguousarray(words, dtype=np.uint64)
    query_start = np.ascontiguousarray(query_start, dtype=np.uint32)
    centroids = np.ascontiguousarray(centroids, dtype=np.float64).reshape(-1, 3)
    nq = int(centroids.shape[0])
    assert words.size >= 1 and query_start.size == words.size + 1 and int(query_start[-1]) == nq and nq >= 1
    assert np.all(words[1:] > words[:-1])
    if not np.all(np.isfinite(centroids)):
        raise ValueError("centroids must be finite")
    d_words = t.from_numpy(words.view(np.int64)).to(eng.device)
    d_start = t.from_numpy(query_start.view(np.int32)).to(eng.device)
    d_cen = t.from_numpy(centroids).to(eng.device)
    d_best = eng.empty(nq, t.int64)
    d_vox = eng.empty(nq, t.int64)
    _abi.check(eng.lib.kh_nearest_label_voxels(P(d_lab), label_bytes, sx, sy, sz, P(d_words), P(d_start), int(words.size), P(d_cen), nq,
                                               P(d_best), P(d_vox), eng.stream()))
    return d_vox.cpu().numpy().view(np.uint64)


def nearest_label_voxels_box(eng, d_lab, label_bytes, extent, lo, dataset_shape, words, query_start, centroids, query_index, d_best,
                             d_vox):
    """One visit of one box of a dataset (kh_nearest_label_voxels_box).  d_lab: the box on the device (1-D, Fortran
    order) of `extent` voxels with its low corner at `lo` of a dataset of `dataset_shape`; words / query_start / centroids as in
    nearest_label_voxels for the queries of THIS visit, centroids in dataset coordinates; query_index: u32 [Q], the row of each of
    them in the running arrays d_best / d_vox (int64 device tensors holding u64 words, set to ~0 once by the caller), distinct.  The
    listed rows are lowered in place to the lexicographic minimum of what came in and what the box holds; nothing is returned and
    nothing waits for the device."""
    t, P = eng.torch, eng.ptr
    ex, ey, ez = (int(v) for v in extent)
    lox, loy, loz = (int(v) for v in lo)
    _, dsy, dsz = (int(v) for v in dataset_shape)
    words = np.ascontiguousarray(words, dtype=np.uint64)
    query_start = np.ascontiguousarray(query_start, dtype=np.uint32)
    centroids = np.ascontiguousarray(centroids, dtype=np.float64).reshape(-1, 3)
    query_index = np.ascontiguousarray(query_index, dtype=np.uint32)
    nq = int(centroids.shape[0])
    assert words.size >= 1 and query_start.size == words.size + 1 and int(query_start[-1]) == nq and nq >= 1
    assert np.all(words[1:] > words[:-1])
    assert query_index.size == nq and np.unique(query_index).size == nq and int(query_index.max()) < min(d_best.numel(), d_vox.numel())
    assert int(d_lab.numel()) == ex * ey * ez and d_lab.element_size() == label_bytes
    if not np.all(np.isfinite(centroids)):
        raise ValueError("centroids must be finite")
    d_words = t.from_numpy(words.view(np.int64)).to(eng.device)
    d_start = t.from_numpy(query_start.view(np.int32)).to(eng.device)
    d_cen = t.from_numpy(centroids).to(eng.device)
    d_index = t.from_numpy(query_index.view(np.int32)).to(eng.device)
    d_scratch = eng.empty(nq, t.int64)
    _abi.check(eng.lib.kh_nearest_label_voxels_box(P(d_lab), label_bytes, ex, ey, ez, lox, loy, loz, dsy, dsz, P(d_words), P(d_start),
                                                   int(words.size), P(d_cen), P(d_index), nq, P(d_best), P(d_vox), P(d_scratch),
                                                   eng.stream()))


def binary_edges(eng, d_img, shape, connectivity=26):
    """d_img: u8 device tensor [nvox] in Fortran order, foreground = 1 (0 / 1 only: the neighbour masks compare labels).
    Returns (vertices u32 (n, 3), edges u32 (m, 2)) as host arrays in the canonical order: vertices by ascending Fortran index,
    edges (a, b) with a < b sorted by a, then b.  A foreground voxel without a foreground neighbour is no vertex."""
    t, P = eng.torch, eng.ptr
    sx, sy, sz = (int(v) for v in shape)
    nvox = sx * sy * sz
    none = np.zeros((0, 3), dtype=np.uint32), np.zeros((0, 2), dtype=np.uint32)
    if nvox == 0:
        return none
    dirs = connectivity_directions(connectivity)
    d_nbr = eng.empty(nvox, t.int32)
    _abi.check(eng.lib.kh_neighbor_mask(P(d_img), 1, sx, sy, sz, P(d_nbr), eng.stream()))
    d_isv = eng.empty(nvox, t.uint8)
    d_own = eng.empty(nvox, t.uint8)
    d_tot = eng.empty(2, t.int64)
    _abi.check(eng.lib.kh_binary_edge_count(P(d_nbr), nvox, dirs, P(d_isv), P(d_own), P(d_tot), eng.stream()))
    nvert, nedge = (int(v) for v in d_tot.cpu().numpy())
    if nedge > MAX_EDGES:
        raise ValueError("the image has %d edges, more than 2^31: a skeleton image is sparse" % nedge)
    if nedge == 0:
        return none
    d_vscan = t.cumsum(d_isv, 0, dtype=t.int64)
    d_escan = t.cumsum(d_own, 0, dtype=t.int64)
    del d_isv, d_own
    d_vert = eng.empty(3 * nvert, t.int32)
    d_edge = eng.empty(2 * nedge, t.int32)
    _abi.check(eng.lib.kh_binary_edge_emit(P(d_nbr), sx, sy, sz, dirs, P(d_vscan), P(d_escan), P(d_vert), P(d_edge), eng.stream()))
    return (d_vert.cpu().numpy().view(np.uint32).reshape(nvert, 3), d_edge.cpu().numpy().view(np.uint32).reshape(nedge, 2))


def check_binary_image(image):
    """The checks that need no GPU: the dtype (bool or integers) and the dimensions (a fourth non-trivial axis is a DimensionError).
    numpy -> the u8 array of 0 / 1 with three axes, Fortran ordered; a torch tensor comes back with at most three axes."""
    if hasattr(image, "permute") and hasattr(image, "device"):          # a torch tensor
        if image.dtype.is_floating_point or image.dtype.is_complex:
            raise TypeError("the image must be bool or integers")
        extents = tuple(int(v) for v in image.shape)
        if any(e != 1 for e in extents[3:]):
            raise DimensionError("Input labels may be no more than three non-trivial dimensions. Got: {}".format(extents))
        return image.reshape(extents[:3]) if len(extents) > 3 else image
    arr = np.asarray(image)
    if arr.dtype != np.bool_ and arr.dtype.kind not in "ui":
        raise TypeError("the image must be bool or integers")
    return format_labels(arr != 0, in_place=True)


def device_binary_image(eng, image):
    """what check_binary_image returned -> (u8 device tensor of 0 / 1 in Fortran order, (sx, sy, sz)); a tensor (indexed [x, y(, z)])
    must live on the engine's device and gets trailing axes up to three"""
    t = eng.torch
    if isinstance(image, np.ndarray):
        return eng.to_device(image), tuple(int(v) for v in image.shape)
    if image.device != eng.device:
        raise ValueError("an image tensor must live on the engine's device (%s)" % eng.device)
    vol = image
    while vol.ndim < 3:
        vol = vol.unsqueeze(-1)
    return (vol != 0).permute(2, 1, 0).contiguous().reshape(-1).to(t.uint8), tuple(int(v) for v in vol.shape)


def gap_launches(counts):
    """counts: parts per group -> the groups of every kh_part_gaps call, in order, so that the tables of one call (counts[g]^2 records
    per group) stay within GAP_MAX_RECORDS; a single group beyond that is a ValueError"""
    launches, used = [], 0
    for g, n in enumerate(counts):
        n = int(n)
        if n > GAP_MAX_PARTS:
            raise ValueError("a group has %d parts: more than %d, whose table of nearest pairs exceeds 1 GiB" % (n, GAP_MAX_PARTS))
        if not launches or used + n * n > GAP_MAX_RECORDS:
            launches.append([])
            used = 0
        launches[-1].append(g)
        used += n * n
    return launches


def part_boxes(parts):
    """parts: vertex arrays f32 [k, 3], k >= 1 -> (xyz f32 [V, 3] back to back, part_start i64 [P + 1], box f32 [P, 6] = min x, y, z,
    max x, y, z): the arrays kh_part_gaps and kh_part_clusters read"""
    sizes = np.array([p.shape[0] for p in parts], dtype=np.int64)
    if sizes.min() < 1:
        raise ValueError("a part without vertices")
    if int(sizes.sum()) >= 2 ** 32:
        raise ValueError("the parts of one call hold %d vertices, more than 2^32 - 1" % int(sizes.sum()))
    part_start = np.concatenate([[0], np.cumsum(sizes)])
    xyz = np.concatenate(parts, axis=0)
    box = np.concatenate([np.minimum.reduceat(xyz, part_start[:-1], axis=0), np.maximum.reduceat(xyz, part_start[:-1], axis=0)], axis=1)
    return xyz, part_start, np.ascontiguousarray(box, dtype=np.float32)


def sweep_order(boxes, group_start, axis):
    """the `order` of kh_part_clusters: per group its parts by the low end of their box along `axis`, ties by part index"""
    n = int(boxes.shape[0])
    group_of = np.repeat(np.arange(group_start.size - 1), np.diff(group_start))
    return np.lexsort((np.arange(n), boxes[:, axis], group_of)).astype(np.uint32)


def part_clusters(eng, boxes, group_start, bound2, axis=None, timings=None):
    """boxes: f32 [n, 6], the bounding boxes (min x, y, z, max x, y, z) of the parts of all groups, group after group; group_start:
    [G + 1], indexing parts; bound2: f64 [G].  Returns cluster u32 [n] (kh_part_clusters, include/kimi_hip.h): the smallest part
    index, in this call's numbering, among the parts connected to the part through pairs of ONE group whose boxes are nearer than
    the group's bound.  One call for all groups.  axis: the axis the parts are swept along (None: the one over which the boxes' low
    ends spread most, summed over the groups); the result does not depend on it.  timings (a dict): cluster_ms (HIP events) is
    added to."""
    t, P = eng.torch, eng.ptr
    boxes = np.ascontiguousarray(boxes, dtype=np.float32).reshape(-1, 6)
    group_start = np.ascontiguousarray(group_start, dtype=np.int64)
    bound2 = np.ascontiguousarray(bound2, dtype=np.float64)
    n, ngroups = int(boxes.shape[0]), int(bound2.size)
    if group_start.size != ngroups + 1 or int(group_start[0]) != 0 or int(group_start[-1]) != n or np.any(np.diff(group_start) < 0):
        raise ValueError("part_clusters: group_start must ascend from 0 to the %d parts for %d groups" % (n, ngroups))
    if n >= 2 ** 31:
        raise ValueError("part_clusters: %d parts, more than 2^31 - 1" % n)
    if n == 0:
        return np.zeros(0, dtype=np.uint32)
    if axis is None:
        filled = group_start[:-1][np.diff(group_start) > 0]
        low = boxes[:, :3].astype(np.float64)
        axis = int(np.argmax((np.maximum.reduceat(low, filled, axis=0) - np.minimum.reduceat(low, filled, axis=0)).sum(axis=0)))
    axis = int(axis)
    if axis not in (0, 1, 2):
        raise ValueError("part_clusters: axis must be 0, 1 or 2")
    order = sweep_order(boxes, group_start, axis)
    d_box = t.from_numpy(boxes).to(eng.device)
    d_gstart = t.from_numpy(group_start.astype(np.uint32).view(np.int32)).to(eng.device)
    d_bound = t.from_numpy(bound2).to(eng.device)
    d_order = t.from_numpy(order.view(np.int32)).to(eng.device)
    d_cluster = eng.empty(n, t.int32)
    if timings is not None:
        begin, end = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
        begin.record()
    _abi.check(eng.lib.kh_part_clusters(P(d_box), P(d_gstart), P(d_bound), P(d_order), ngroups, n, axis, P(d_cluster), eng.stream()))
    if timings is not None:
        end.record()
        end.synchronize()
        timings["cluster_ms"] = timings.get("cluster_ms", 0.0) + begin.elapsed_time(end)
    return d_cluster.cpu().numpy().view(np.uint32)


def part_gaps(eng, groups, bound2, timings=None):
    """groups: per group the list of its parts' vertices (f32 [k, 3], k >= 1); bound2: per group the f64 bound on d2 (+inf: none).
    Returns per group (d2 f64 [n, n], idx u32 [n, n, 2]): the records of kh_part_gaps (include/kimi_hip.h), row = tree part, column =
    query part, idx = (kt, kq); "none" is d2 = +inf and both indices 0xFFFFFFFF.  One call of the kernel for all groups, or a few
    under gap_launches.  timings (a dict): gets kernel_ms (HIP events around the calls) and copy_s (the tables' way to the host)."""
    t, P = eng.torch, eng.ptr
    out = [None] * len(groups)
    kernel_ms, copy_s = 0.0, 0.0
    for launch in gap_launches([len(g) for g in groups]):
        parts = [np.ascontiguousarray(p, dtype=np.float32).reshape(-1, 3) for g in launch for p in groups[g]]
        counts = np.array([len(groups[g]) for g in launch], dtype=np.int64)
        rec_start = np.concatenate([[0], np.cumsum(counts * counts)]).astype(np.int64)
        nrec = int(rec_start[-1])
        if nrec == 0:
            for g in launch:
                out[g] = np.zeros((0, 0), dtype=np.float64), np.zeros((0, 0, 2), dtype=np.uint32)
            continue
        xyz, part_start, box = part_boxes(parts)
        group_start = np.concatenate([[0], np.cumsum(counts)])
        d_xyz = t.from_numpy(xyz).to(eng.device)
        d_pstart = t.from_numpy(part_start.astype(np.uint32).view(np.int32)).to(eng.device)
        d_box = t.from_numpy(box).to(eng.device)
        d_gstart = t.from_numpy(group_start.astype(np.uint32).view(np.int32)).to(eng.device)
        d_bound = t.from_numpy(np.array([bound2[g] for g in launch], dtype=np.float64)).to(eng.device)
        d_rstart = t.from_numpy(rec_start).to(eng.device)
        d_d2 = eng.empty(nrec, t.int64)
        d_idx = eng.empty(2 * nrec, t.int32)
        if timings is not None:
            begin, end = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
            begin.record()
        _abi.check(eng.lib.kh_part_gaps(P(d_xyz), P(d_pstart), P(d_box), P(d_gstart), P(d_bound), P(d_rstart), len(launch), nrec,
                                        P(d_d2), P(d_idx), eng.stream()))
        if timings is not None:
            end.record()
            end.synchronize()
            kernel_ms += begin.elapsed_time(end)
            t0 = time.perf_counter()
        d2 = d_d2.cpu().numpy().view(np.float64)
        idx = d_idx.cpu().numpy().view(np.uint32)
        if timings is not None:
            copy_s += time.perf_counter() - t0
        for k, g in enumerate(launch):
            n = int(counts[k])
            out[g] = (d2[rec_start[k]:rec_start[k + 1]].reshape(n, n), idx[2 * rec_start[k]:2 * rec_start[k + 1]].reshape(n, n, 2))
    if timings is not None:
        timings["kernel_ms"] = timings.get("kernel_ms", 0.0) + kernel_ms
        timings["copy_s"] = timings.get("copy_s", 0.0) + copy_s
    return out
