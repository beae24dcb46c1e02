"""Point queries for a dataset that is never resident as a whole, on the plumbing of kimimaro_amd.boxes (every public name is
kimimaro_amd.post's too):

    synapses_to_targets_chunked(dataset, synapses, chunk_shape)         synapse detections to the extra targets of skeletonize_chunked,
                                                                        the dataset in boxes
"""
import time

import numpy as np

from . import intake, ops, points
from .boxes import _load_box, label_type
from .plan import box_distance_bounds, chunk_grid, nearest_first
from .volume import DimensionError, _device_labels


def synapses_to_targets_chunked(dataset, synapses, chunk_shape=(512, 512, 512), progress=False, stats=None, _visit=None, _order=None):
    """synapses_to_targets for a dataset that is never resident as a whole: {(x, y, z): swc_label}, DEFINED as what
    synapses_to_targets(dataset, synapses) returns for the whole dataset, item for item and in the same insertion order -- scipy's
    float64 distances, among equally near voxels the first in C order of the DATASET, labels in the order of `synapses`, a label
    that occurs nowhere contributes nothing, a label the dtype cannot hold and a repeated label word as there.  The result is what
    skeletonize_chunked(extra_targets_after=) takes.

    The cores of plan.chunk_grid(shape, chunk_shape, overlap=0) partition the dataset.  They are visited nearest first
    (plan.nearest_first of plan.box_distance_bounds); per query the best (distance, C-order index) so far stays on the device and
    every visit lowers it (kh_nearest_label_voxels_box).  A query is ACTIVE in a core unless the core's bound exceeds its best
    distance so far, strictly; a visit is handed the active queries only and a core without one is not loaded.  A label that occurs
    nowhere keeps its queries active in every core: the whole-volume call, too, has to look everywhere to learn that.

    dataset: numpy of any order, an np.memmap, a tensor on the GPU, or any object with .shape and slicing over a tuple of slices;
      three axes (DimensionError otherwise), any label dtype synapses_to_targets takes.  It may hold 2^32 voxels or more; 2^63 or
      more are a ValueError (the dataset's C-order index is a u64 whose ~0 is the "none" word).
    synapses: {label: [(centroid, swc_label), ...]}, centroids in dataset voxel coordinates, inside or outside the dataset;
      non-finite ones are a ValueError.  Empty: {} without touching the GPU.
    progress: accepted, no effect.
    stats (a dict) receives cores, cores_visited, cores_skipped, pairs (active (core, query) pairs summed over the visited cores),
      load_s and visit_s (seconds).
    _visit(box, lo, shape, words, query_start, centroids, query_index, best_distance, best_voxel) replaces the kernel call on host
      arrays (u64 running arrays, lowered in place): with it nothing here touches the GPU (the host-logic tests run the whole
      driver on numpy).  Without it there is no CPU fallback.  _order(bounds) -> the visit order replaces plan.nearest_first."""
    name = "synapses_to_targets_chunked"
    shape = tuple(int(v) for v in dataset.shape)
    if len(shape) != 3:
        raise DimensionError("{} needs a dataset of three axes. Got: {}".format(name, shape))
    if shape[0] * shape[1] * shape[2] >= 2 ** 63:
        raise ValueError("{}: a dataset of {} holds 2^63 voxels or more".format(name, shape))
    if len(synapses) == 0:
        return {}
    eng = ops.engine() if _visit is None else None       # raises HipUnavailableError without the library or a gfx950 device
    grid = chunk_grid(shape, chunk_shape, overlap=0)
    dtype, _, span = label_type(dataset)
    queries = intake.synapse_queries(synapses, span, dtype.itemsize)
    if queries is None:
        return {}
    groups, words, query_start, centroids = queries
    if not np.all(np.isfinite(centroids)):
        raise ValueError("centroids must be finite")
    nq = int(centroids.shape[0])
    label_of = np.repeat(np.arange(words.size), np.diff(query_start.astype(np.int64)))     # per query its row of `words`

    bounds = box_distance_bounds(grid.core_lo, grid.core_hi, centroids)
    order = (nearest_first if _order is None else _order)(bounds)
    best = np.full(nq, points.NONE64, dtype=np.uint64)    # the running distances as the host knows them: bits of non-negative f64
    if eng is None:
        winners = np.full(nq, points.NONE64, dtype=np.uint64)
    else:
        d_best = eng.torch.full((nq,), -1, dtype=eng.torch.int64, device=eng.device)
        d_vox = eng.torch.full((nq,), -1, dtype=eng.torch.int64, device=eng.device)
    visited, pairs, load_s, visit_s = 0, 0, 0.0, 0.0
    for k in (int(v) for v in order):
        none = best == points.NONE64
        active = np.flatnonzero(none | ~(bounds[k] > np.where(none, 0, best).view(np.float64)))
        if active.size == 0:
            continue
        visited += 1
        pairs += int(active.size)
        lo, hi = grid.core_lo[k], grid.core_hi[k]
        t0 = time.perf_counter()
        box = _load_box(dataset, lo, hi, name)
        load_s += time.perf_counter() - t0
        t0 = time.perf_counter()
        rows, counts = np.unique(label_of[active], return_counts=True)
        args = (words[rows], np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32), centroids[active], active.astype(np.uint32))
        if eng is None:
            _visit(box, lo, shape, *args, best, winners)
        else:
            d_box, itemsize, _, extent, _, _ = _device_labels(eng, box)
            points.nearest_label_voxels_box(eng, d_box, itemsize, extent, lo, shape, *args, d_best, d_vox)
            best = d_best.cpu().numpy().view(np.uint64)
            del d_box
        visit_s += time.perf_counter() - t0
    if eng is not None:
        winners = d_vox.cpu().numpy().view(np.uint64)
    if stats is not None:
        n = int(grid.core_lo.shape[0])
        stats.update(cores=n, cores_visited=visited, cores_skipped=n - visited, pairs=pairs, load_s=load_s, visit_s=visit_s)
    return intake.synapse_targets(groups, words, query_start, winners, shape[1], shape[2])
