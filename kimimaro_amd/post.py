"""Row f4: stitching the skeletons of adjacent chunks -- the counterpart of kimimaro/post.py.

    postprocess(skeleton, dust_threshold=1500, tick_threshold=3000)     kimimaro/post.py:49-87
    join_close_components(skeletons, radius=inf, restrict_by_radius)    kimimaro/post.py:89-218
    remove_dust / remove_loops / remove_ticks                            kimimaro/post.py:222-260, 436-563

    join_close_components_many(groups, radius=inf, restrict_by_radius)  the join of many groups at once
    postprocess_many(skeletons, dust_threshold=1500, tick_threshold=3000)
    skeletonize_chunked(dataset, chunk_shape, ...)                      a dataset in chunks to whole skeletons
    cross_sectional_area_chunked(dataset, skeletons, chunk_shape, halo) their sections, the dataset in boxes
    cross_sectional_area_filled_chunked(dataset, skeletons, ...)        the same of the filled labels, on
    region_graph_chunked(dataset, chunk_shape, region_store)            the region graph of a dataset from its cores, and hole_lists
    oversegment_chunked(dataset, skeletons, chunk_shape, ...)           their segments, relaxed box by box

Host code on graphs of 10^2..10^5 nodes: the reference is Python here and so are the single-skeleton
functions; nothing in them touches the GPU path.  The two *_many functions do: the nearest pairs between all parts of all groups
come from one kernel call (csrc/join.hip through kimimaro_amd.points.part_gaps), the merge sequence from host C that reads only
that table (kh_host_join_plan); they have no CPU fallback.  Written from the behaviour of the reference, including the parts that are visible in its
results: which cycle its depth-first search reports first (skeletontricks.hpp:209-300: neighbours in the order the
edges list them, the search starts at the first edge), float32 branch lengths accumulated outward from the smallest
terminal node (skeletontricks.hpp:303-380), superedges fused at a branch point that drops to two edges and from then
on treated as removable whatever their ends are (post.py:324-336).  Where the reference leaves a choice to the
iteration order of a Python set (equal-length ticks, post.py:339) the smallest (length, nodes) pair is taken.
Pinned by tests/golden/post.npz: outputs of the reference's own post.py run on the vectors' inputs (generator and the
stand-ins it needs: tests/golden/make_golden.py `post`).
"""
from __future__ import annotations

import copy
import time
from collections import defaultdict, namedtuple

import numpy as np

from . import _abi, feature, intake, ops, points, section, utility
from .holes import enclosed_regions
from .lanes import Lanes, lanes_for
from .plan import chunk_grid, core_of, halo_boxes
from .skeleton import Skeleton
from .volume import _device_labels, ranges


def postprocess(skeleton, dust_threshold=1500.0, tick_threshold=3000.0):
    """kimimaro/post.py:49-87: dust components out, loops out, close components joined, ticks out."""
    label = skeleton.id
    skel = skeleton.consolidate(remove_disconnected_vertices=True)
    skel = remove_dust(skel, dust_threshold)
    skel = remove_loops(skel)
    skel = join_close_components(skel, restrict_by_radius=True)
    skel = remove_ticks(skel, tick_threshold)
    skel.id = label
    return skel.consolidate(remove_disconnected_vertices=True)


# ---------------------------------------------------------------------------------------------------------------
def remove_dust(skeleton, dust_threshold):
    """components whose cable length does not exceed the threshold are dropped (post.py:222-233)."""
    if skeleton.empty() or dust_threshold == 0:
        return skeleton
    return Skeleton.simple_merge([c for c in skeleton.components() if c.cable_length() > dust_threshold])


# ---------------------------------------------------------------------------------------------------------------
def join_close_components(skeletons, radius=np.inf, restrict_by_radius=False):
    """Repeatedly connects the two components whose nearest vertices are closest (post.py:89-218).  With
    restrict_by_radius the search radius becomes twice the largest vertex radius and a pair only qualifies when its
    gap is at most the sum of the two vertices' radii."""
    from scipy.spatial import cKDTree
    if radius is None:
        radius = np.inf
    if radius <= 0:
        raise ValueError("radius must be greater than zero: " + str(radius))
    if isinstance(skeletons, Skeleton):
        skeletons = [skeletons]
    parts = []
    for s in skeletons:
        parts.extend(c.consolidate(remove_disconnected_vertices=True) for c in s.components())
    parts = [p for p in parts if not p.empty()]
    if len(parts) == 1:
        return parts[0]
    if not parts:
        return Skeleton()
    if restrict_by_radius:
        radius = max(2 * max(float(np.max(p.radii)) for p in parts), 0)

    def gap(tree, a, b):
        """nearest pair between parts a (in `tree`) and b: (distance as the float32 the reference stores, index in a, in b)"""
        dist, hit = tree.query(b.vertices, k=1, distance_upper_bound=radius + 0.000001)
        kb = int(np.argmin(dist))
        ka = int(hit[kb])
        d = dist[kb]
        if restrict_by_radius and np.isfinite(d) and d > (a.radii[ka] + b.radii[kb]):
            d = np.inf
        return np.float32(d), ka, kb

    # gaps[i][j] for i < j only (the reference fills both triangles of its matrix and reads the first minimum in row-major
    # order, which lies in the upper one)
    n = len(parts)
    gaps = {}
    for i in range(n):
        tree = cKDTree(parts[i].vertices)
        for j in range(i + 1, n):
            gaps[(i, j)] = gap(tree, parts[i], parts[j])
    while len(parts) > 1:
        n = len(parts)
        best = min(((gaps[(i, j)][0], i, j) for i in range(n) for j in range(i + 1, n)), key=lambda t: (t[0], t[1], t[2]))
        if not np.isfinite(best[0]) or best[0] > radius:
            break
        _, i, j = best
        _, ka, kb = gaps[(i, j)]
        a, b = parts[i], parts[j]
        fused = Skeleton.simple_merge([a, b])
        fused.edges = np.concatenate([fused.edges, np.array([[ka, kb + a.vertices.shape[0]]], dtype=np.uint32)])
        rest = [k for k in range(n) if k not in (i, j)]
        renum = {old: new + 1 for new, old in enumerate(rest)}
        gaps = {(renum[p], renum[q]): v for (p, q), v in gaps.items() if p in renum and q in renum}
        parts = [fused] + [parts[k] for k in rest]
        tree = cKDTree(fused.vertices)
        for j in range(1, len(parts)):
            gaps[(0, j)] = gap(tree, fused, parts[j])
    return Skeleton.simple_merge(parts).consolidate(remove_disconnected_vertices=True)


# ---------------------------------------------------------------------------------------------------------------
def join_parts(skeletons):
    """the parts join_close_components works on: the components of every skeleton, in order, consolidated, the empty ones dropped"""
    if isinstance(skeletons, Skeleton):
        skeletons = [skeletons]
    parts = []
    for s in skeletons:
        parts.extend(c.consolidate(remove_disconnected_vertices=True) for c in s.components())
    return [p for p in parts if not p.empty()]


def join_plan(part_sizes, d2, idx, radii, radius, restrict_by_radius):
    """kh_host_join_plan (host C, no GPU needed; include/kimi_hip.h): the edges u32 [m, 2], in the numbering of the concatenated parts,
    that join_close_components adds to one group, from the table of nearest pairs (d2 f64 [n, n], idx u32 [n, n, 2]) of its parts."""
    sizes = np.ascontiguousarray(part_sizes, dtype=np.uint32)
    n = int(sizes.size)
    d2 = np.ascontiguousarray(d2, dtype=np.float64)
    idx = np.ascontiguousarray(idx, dtype=np.uint32)
    radii = np.ascontiguousarray(radii, dtype=np.float32)
    if d2.size != n * n or idx.size != 2 * n * n or radii.size != int(sizes.sum(dtype=np.int64)):
        raise ValueError("join_plan: tables of %d and %d entries, %d radii for %d parts" % (d2.size, idx.size, radii.size, n))
    edges = np.zeros((max(n - 1, 1), 2), dtype=np.uint32)
    p = _abi.np_ptr
    m = _abi.lib().kh_host_join_plan(n, p(sizes), p(d2), p(idx), p(radii), float(radius), int(bool(restrict_by_radius)), p(edges))
    if m == -2:
        raise MemoryError("kh_host_join_plan failed")
    if m < 0:
        raise ValueError("kh_host_join_plan: a record names a vertex outside its part")
    return edges[:m]


def join_close_components_many(groups, radius=np.inf, restrict_by_radius=False, timings=None):
    """join_close_components for many groups at once: each group is a Skeleton or a sequence of them, the result per
    group what join_close_components(group, radius, restrict_by_radius) returns -- Skeleton.simple_merge of its parts plus one edge
    per merge, consolidated.  The nearest pairs between the parts of ALL groups come from one kernel call (a few when their tables
    exceed 1 GiB; a single group of more than 8 192 parts is a ValueError), every group with its own radius and bound under
    restrict_by_radius; the merge sequence of a group is decided on its table alone.  Where several tree vertices are equally near
    the winning query vertex the smallest index is taken (cKDTree makes its own choice there).  No CPU fallback:
    HipUnavailableError without the library or an MI355X.  timings (a dict): kernel_ms, copy_s, plan_s of the call."""
    if radius is None:
        radius = np.inf
    if radius <= 0:
        raise ValueError("radius must be greater than zero: " + str(radius))
    eng = ops.engine()                                   # raises HipUnavailableError without the library or a gfx950 device
    groups = list(groups)
    parts = [join_parts(g) for g in groups]
    radius_of = [float(radius)] * len(groups)
    if restrict_by_radius:
        radius_of = [max(2 * max(float(np.max(p.radii)) for p in ps), 0) if ps else 0.0 for ps in parts]
    todo = [g for g in range(len(groups)) if len(parts[g]) >= 2]
    tables = points.part_gaps(eng, [[p.vertices for p in parts[g]] for g in todo],
                              [(radius_of[g] + 0.000001) * (radius_of[g] + 0.000001) for g in todo], timings=timings)
    out = [ps[0] if ps else Skeleton() for ps in parts]
    t0 = time.perf_counter()
    for g, (d2, idx) in zip(todo, tables):
        ps = parts[g]
        merged = Skeleton.simple_merge(ps)
        added = join_plan([p.vertices.shape[0] for p in ps], d2, idx, merged.radii, radius_of[g], restrict_by_radius)
        merged.edges = np.concatenate([merged.edges, added])
        out[g] = merged.consolidate(remove_disconnected_vertices=True)
    if timings is not None:
        timings["plan_s"] = timings.get("plan_s", 0.0) + time.perf_counter() - t0
    return out


def postprocess_many(skeletons, dust_threshold=1500.0, tick_threshold=3000.0):
    """postprocess for many skeletons: dust and loops out per skeleton on the host, the join of ALL of them in one
    join_close_components_many(restrict_by_radius=True) call, ticks out per skeleton on the host."""
    skeletons = list(skeletons)
    ops.engine()                                         # raises HipUnavailableError without the library or a gfx950 device
    cleaned = []
    for skeleton in skeletons:
        skel = skeleton.consolidate(remove_disconnected_vertices=True)
        skel = remove_dust(skel, dust_threshold)
        cleaned.append(remove_loops(skel))
    out = []
    for skeleton, skel in zip(skeletons, join_close_components_many(cleaned, restrict_by_radius=True)):
        skel = remove_ticks(skel, tick_threshold)
        skel.id = skeleton.id
        out.append(skel.consolidate(remove_disconnected_vertices=True))
    return out


# ---------------------------------------------------------------------------------------------------------------
def place_fragment(skeleton, box_low, anisotropy, label=None):
    """The skeleton of one box (physical space, vertices = f32(voxel) * anisotropy) moved to where the box lies in the dataset: a new
    Skeleton with vertices f32(voxel + box_low) * anisotropy -- the very floats a run over the whole dataset stores for those voxels, so
    that the seam vertices of neighbouring boxes are bit-equal and consolidate() fuses them.  (Adding f32(box_low) * anisotropy to the
    vertices instead rounds twice and misses that value for most anisotropies that are no small integers.)  The voxel of a vertex v
    is i = rint(v / anisotropy); ValueError when f32(i) * anisotropy != v for some vertex: it does not lie on the voxel lattice.
    Edges, radii, vertex types and transform are the skeleton's; id = `label` (default: the skeleton's), space = "physical"."""
    an = np.asarray(anisotropy, dtype=np.float32).reshape(3)
    low = np.asarray(box_low, dtype=np.int64).reshape(3)
    v = np.asarray(skeleton.vertices, dtype=np.float32).reshape(-1, 3)
    voxel = np.rint(v.astype(np.float64) / an.astype(np.float64)).astype(np.int64)
    back = np.multiply(voxel.astype(np.float32), an, dtype=np.float32)
    if not np.array_equal(back, v):
        k = int(np.flatnonzero((back != v).any(axis=1))[0])
        raise ValueError("place_fragment: vertex %d = %s is not f32(voxel) * anisotropy for anisotropy %s" % (k, v[k].tolist(), an.tolist()))
    placed = np.multiply((voxel + low).astype(np.float32), an, dtype=np.float32)
    return Skeleton(placed, np.array(skeleton.edges), np.array(skeleton.radii), np.array(skeleton.vertex_types),
                    segid=skeleton.id if label is None else label, transform=np.array(skeleton.transform), space="physical")


def route_targets(targets, grid, shape):
    """Extra targets given as voxels of the dataset -> per chunk of `grid` the list of those its box contains, as (x, y, z) tuples
    relative to the box's low corner.  A point on an overlap plane goes to both boxes.  Two coordinates get z = 0.  IndexError, naming
    the point, for one outside a dataset of `shape`."""
    shape = (tuple(int(v) for v in shape) + (1,))[:3]
    out = [[] for _ in range(grid.box_lo.shape[0])]
    for target in targets:
        pt = tuple(int(v) for v in target)
        if len(pt) == 2:
            pt += (0,)
        if len(pt) != 3 or any(not 0 <= v < s for v, s in zip(pt, shape)):
            raise IndexError("point {} is outside a dataset of shape {}".format(tuple(target), shape))
        p = np.asarray(pt, dtype=np.int64)
        for k in np.flatnonzero(((grid.box_lo <= p) & (p < grid.box_hi)).all(axis=1)).tolist():
            out[k].append(tuple(int(v) for v in p - grid.box_lo[k]))
    return out


def _load_box(dataset, lo, hi):
    """dataset[lo:hi] as a host array with three axes: numpy arrays of any order and memmaps, a tensor (copied from where it lives),
    anything that takes a tuple of slices (the h5py / zarr form)"""
    cut = dataset[tuple(slice(int(a), int(b)) for a, b in zip(lo, hi))[:len(dataset.shape)]]
    if hasattr(cut, "cpu") and hasattr(cut, "numpy"):
        cut = cut.cpu().numpy()
    cut = np.asarray(cut)
    return cut.reshape(cut.shape + (1,) * (3 - cut.ndim))


def count_labels(dataset, grid):
    """{label: voxels in the whole dataset}, zero included, from one pass over the cores of `grid` (they partition the dataset)"""
    total = defaultdict(int)
    for lo, hi in zip(grid.core_lo, grid.core_hi):
        values, counts = np.unique(_load_box(dataset, lo, hi), return_counts=True)
        for value, count in zip(values.tolist(), counts.tolist()):
            total[value] += count
    return dict(total)


def skeletonize_chunked(dataset, chunk_shape=(512, 512, 512), teasar_params=None, anisotropy=(1, 1, 1), object_ids=None,
                        dust_threshold=1000, dust_global=False, post_dust_threshold=1500.0, tick_threshold=3000.0, merge=True,
                        fix_branching=True, fix_borders=True, fill_holes=False, fix_avocados=False, extra_targets_before=[],
                        extra_targets_after=[], progress=False, lanes=None, width=None, timings=None, _skeletonize=None,
                        _postprocess=None, cross_sectional_area=None):
    """A dataset in chunks to whole skeletons, {label: Skeleton} in ascending label order: what igneous does around
    kimimaro.skeletonize and kimimaro.postprocess, in one call.

    The dataset is cut by plan.chunk_grid(dataset.shape, chunk_shape): every box shares its last plane with the next core, so with
    fix_borders a label that crosses a cut gets the same path end in both boxes.  Every box goes through skeletonize with several
    in flight (kimimaro_amd.lanes; a box is loaded by the lane that takes it, so loading overlaps tracing); the fragments are
    moved into dataset coordinates (place_fragment) and, per label, fused: Skeleton.simple_merge(fragments).consolidate().  ONE
    postprocess_many(fused skeletons, post_dust_threshold, tick_threshold) follows; a label whose result is empty is dropped.  The
    result is DEFINED as this composition; it is not skeletonize() of the whole volume.

    dataset: a numpy array of any memory order, an np.memmap, a tensor on the GPU, or any object with .shape and __getitem__ over a
      tuple of slices; two or three axes.  It may hold 2^32 voxels or more: only a box has to stay below that.
    teasar_params, anisotropy, object_ids, fix_branching, fix_borders, fill_holes, fix_avocados: handed to skeletonize per box.
    dust_threshold: skeletonize's, per box and component (the reference's meaning) -- unless
    dust_global: a label is kept when it has more than dust_threshold voxels in the WHOLE dataset (counted in a first pass over the
      cores); every box is traced with dust_threshold=0 and object_ids = the kept labels present in it (intersected with a given
      object_ids), a box without one is skipped.  A label cut into pieces that are each below the threshold survives only this way.
    extra_targets_before / _after: voxels of the dataset; each goes to every box that contains it.  IndexError for one outside.
    merge=False: {label: [placed fragments in chunk order]}, nothing further is run.
    cross_sectional_area: None, or a dict of keyword arguments for cross_sectional_area_chunked(dataset, result, ...), which then gives
      every returned skeleton its sections (`anisotropy` defaults to this call's); ignored with merge=False.
    lanes, width: as in skeletonize_many -- a Lanes object to reuse, else `width` lanes are made (default: lanes_for() on the
      largest box), never more than there are chunks.
    progress: accepted, no effect.
    timings (a dict) receives count_s, chunks_s, place_s, fuse_s, post_s (seconds), chunks (boxes traced), fragments and vertices
      (of the placed fragments).
    _skeletonize(labels, **kwargs) -> {label: Skeleton} runs the boxes one after the other in place of the lanes,
    _postprocess(skeletons, dust_threshold, tick_threshold) -> list replaces postprocess_many: with both, nothing here touches the GPU
      (the host-logic tests run the whole driver on the CPU oracle).  Without them there is no CPU fallback."""
    params = intake.DEFAULT_TEASAR_PARAMS if teasar_params is None else teasar_params
    if _skeletonize is None or (merge and _postprocess is None):
        ops.engine()                                     # raises HipUnavailableError without the library or a gfx950 device
    shape = tuple(int(v) for v in dataset.shape)
    if len(shape) not in (2, 3):
        raise intake.DimensionError("skeletonize_chunked needs a dataset of two or three axes. Got: {}".format(shape))
    grid = chunk_grid(shape, chunk_shape)
    n = int(grid.box_lo.shape[0])
    extents = grid.box_hi - grid.box_lo
    largest = tuple(int(v) for v in extents[int(np.argmax(np.prod(extents, axis=1)))])
    if largest[0] * largest[1] * largest[2] >= 2 ** 32:
        raise ValueError("skeletonize_chunked: a box of {} voxels does not fit the 32-bit indices of a volume".format(largest))
    before = route_targets(extra_targets_before, grid, shape)
    after = route_targets(extra_targets_after, grid, shape)
    wanted = None if object_ids is None else set(int(v) for v in object_ids)

    t0 = time.perf_counter()
    kept = None
    if dust_global:
        kept = {label for label, count in count_labels(dataset, grid).items() if label != 0 and count > dust_threshold}
        if wanted is not None:
            kept &= wanted
    count_s = time.perf_counter() - t0

    def one(k, run):
        labels = _load_box(dataset, grid.box_lo[k], grid.box_hi[k])
        ids, dust = object_ids, dust_threshold
        if kept is not None:
            ids = sorted(kept.intersection(np.unique(labels).tolist()))
            dust = 0
            if not ids:
                return None
        return run(labels, teasar_params=params, anisotropy=anisotropy, object_ids=ids, dust_threshold=dust, progress=False,
                   fix_branching=fix_branching, fix_borders=fix_borders, fill_holes=fill_holes, fix_avocados=fix_avocados,
                   extra_targets_before=before[k], extra_targets_after=after[k])

    t0 = time.perf_counter()
    if _skeletonize is not None:
        results = [one(k, _skeletonize) for k in range(n)]
    else:
        own = lanes is None
        if own:
            if width is None:
                import torch
                width = lanes_for(largest, torch.cuda.mem_get_info()[0])
            lanes = Lanes(max(1, min(n, int(width))))

        def job(eng, k):
            return one(k, lambda labels, **kw: intake.skeletonize(labels, _engine=eng, **kw))

        try:
            results = [res for _, res in lanes.run(job, n)]
        finally:
            if own:
                lanes.close()
    chunks_s = time.perf_counter() - t0

    t0 = time.perf_counter()
    fragments = defaultdict(list)
    for k, res in enumerate(results):
        for label, skel in (res or {}).items():
            if not skel.empty():
                fragments[label].append(place_fragment(skel, grid.box_lo[k], anisotropy, label=label))
    fragments = {label: fragments[label] for label in sorted(fragments)}
    place_s = time.perf_counter() - t0
    if timings is not None:
        timings.update(count_s=count_s, chunks_s=chunks_s, place_s=place_s, fuse_s=0.0, post_s=0.0,
                       chunks=sum(res is not None for res in results), fragments=sum(len(f) for f in fragments.values()),
                       vertices=sum(s.vertices.shape[0] for f in fragments.values() for s in f))
    if not merge:
        return fragments

    t0 = time.perf_counter()
    fused = [Skeleton.simple_merge(f).consolidate() for f in fragments.values()]
    fuse_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    done = []
    if fused:
        done = (postprocess_many if _postprocess is None else _postprocess)(fused, post_dust_threshold, tick_threshold)
    post_s = time.perf_counter() - t0
    if timings is not None:
        timings.update(fuse_s=fuse_s, post_s=post_s)
    out = {label: skel for label, skel in zip(fragments, done) if not skel.empty()}
    if cross_sectional_area is not None:
        cross_sectional_area_chunked(dataset, out, **dict({"anisotropy": anisotropy}, **cross_sectional_area))
    return out


# ---------------------------------------------------------------------------------------------------------------
XS_CLIPPED = 64          # cross_sectional_area_contacts: the section was still clipped by the largest box that could be loaded


def _xs_box_budget(eng, itemsize, region_bytes=0):
    """The default max_box_voxels: what the free HBM pays for.  While a box is resident a voxel costs the label itself and, in round
    0, the copy of the core that is counted (2 x itemsize); labels of eight bytes are renumbered per box (utility._narrow_labels:
    torch.unique with its inverse -- the sorted copy, the permutation, the inverse and the shifted ids at 8 bytes each, the u32 ids,
    a mask: 56 bytes with the volume).  region_bytes: what else a voxel costs (cross_sectional_area_filled_chunked: 4, the box of
    the region store).  Kept back: the kernel's scratch (section.SCRATCH_BUDGET) and 1 GiB for the 2^24-voxel pieces of the count."""
    free = int(eng.torch.cuda.mem_get_info(eng.device)[0])
    return max(0, (free - section.SCRATCH_BUDGET - (1 << 30)) // ((2 * itemsize if itemsize < 8 else 56) + region_bytes))


# ---------------------------------------------------------------------------------------------------------------
RegionGraph = namedtuple("RegionGraph", "store value face pairs bases member_offsets members info")


def _merge_regions(value, face, core_pairs, seam_keys):
    """The host merge of region_graph_chunked on provisional ids 1..N (value u64, face u8: [N + 1]; core_pairs: the cores' adjacency
    keys in provisional ids; seam_keys: low << 32 | high of every cross-cut pair).  A seam pair of equal value joins two pieces of one
    region (union-find, numpy: roots are hooked to the smaller root and the forest is flattened, until every pair agrees), one of
    unequal value is an adjacency.  -> (merged u32 [N + 1]: the merged id 1..G of a provisional id, value, face [G + 1], pairs)"""
    n = int(value.size) - 1
    low, high = seam_keys >> np.uint64(32), seam_keys & np.uint64(0xFFFFFFFF)
    same = value[low] == value[high]
    joined, index = np.unique(np.concatenate([low[same], high[same]]), return_inverse=True)      # union-find on the ids that occur
    index = np.asarray(index).reshape(-1)
    a, b = index[:index.size // 2], index[index.size // 2:]
    parent = np.arange(joined.size, dtype=np.int64)
    while True:
        ra, rb = parent[a], parent[b]
        apart = ra != rb
        if not apart.any():
            break
        ra, rb = ra[apart], rb[apart]
        small = np.minimum(ra, rb)
        np.minimum.at(parent, ra, small)
        np.minimum.at(parent, rb, small)
        while True:
            up = parent[parent]
            if np.array_equal(up, parent):
                break
            parent = up
    root = np.arange(n + 1, dtype=np.int64)
    root[joined.astype(np.int64)] = joined[parent].astype(np.int64)
    roots, merged = np.unique(root[1:], return_inverse=True)
    merged = np.concatenate([np.zeros(1, dtype=np.int64), np.asarray(merged).reshape(-1) + 1])
    g = int(roots.size)
    m_value = np.zeros(g + 1, dtype=np.uint64)
    m_value[merged] = value                                                 # (all members carry one value)
    m_face = (np.bincount(merged[1:], weights=face[1:], minlength=g + 1) > 0).astype(np.uint8)
    keys = np.concatenate([core_pairs, seam_keys[~same]])
    p, q = merged[(keys >> np.uint64(32)).astype(np.int64)], merged[(keys & np.uint64(0xFFFFFFFF)).astype(np.int64)]
    assert np.all(p != q), "region_graph_chunked: a pair joins a merged region with itself"
    pairs = np.unique((np.minimum(p, q).astype(np.uint64) << np.uint64(32)) | np.maximum(p, q).astype(np.uint64))
    return merged.astype(np.uint32), m_value, m_face, pairs


def hole_lists(graph, words):
    """hole(L) on a RegionGraph for each of the label words `words` (the unsigned words the dataset's dtype holds): per word the
    u32 PROVISIONAL ids of its hole regions, ascending -- kh_host_enclosed_regions on the merged graph, every merged region
    replaced by its members.  The ids of one core are one range (graph.bases), so a box's share of a list is a filter."""
    offsets, regions = enclosed_regions(graph.value, graph.face, graph.pairs, np.array(list(words), dtype=np.uint64))
    out = []
    for i in range(len(offsets) - 1):
        mine = regions[int(offsets[i]):int(offsets[i + 1])].astype(np.int64)
        first = graph.member_offsets[mine]
        out.append(np.sort(graph.members[ranges(first, graph.member_offsets[mine + 1] - first)]))
    return out


def region_graph_chunked(dataset, chunk_shape=(512, 512, 512), region_store=None, timings=None, _regions=None):
    """The region graph (the 6-connected components of equal value, 0 included, and which of them share a voxel face)
    of a dataset that is never resident as a whole, from one sweep over the cores of plan.halo_boxes(shape, chunk_shape, 0) in raster
    order.  A core is loaded, uploaded as it is (1, 2, 4 or 8 bytes per label; bool as bytes) and handed to
    Engine.region_graph with the mask of its faces that are faces of the DATASET (kh_region_table_box); its region r gets the
    PROVISIONAL id base_k + r, base_k = the regions of all earlier cores.  The provisional ids go, per voxel, into the region store.
    For each axis on which the core has a lower neighbour its lowest plane of ids is paired with the facing plane of the store
    (kh_region_seam_pairs).  The host then joins the pieces that a seam pair of equal value connects (numpy union-find) into the
    merged regions 1..G.

    region_store: an array-like of the dataset's shape (three axes), u32, indexed [x, y, z], read and written by slices only --
    e.g. an np.memmap; default: a numpy array in host memory.  It costs 4 BYTES PER VOXEL OF THE DATASET.  Id 0 never occurs.
    Returns RegionGraph(store; value u64, face u8: [G + 1], entry 0 unused, face = the region owns a voxel on a face of the dataset,
    an axis of extent 1 putting every voxel on one; pairs: u64, smaller merged id << 32 | larger, each once; bases: int64
    [cores + 1], core k owns the provisional ids bases[k] + 1 .. bases[k + 1]; member_offsets, members: the provisional ids of merged
    region g are members[member_offsets[g] : member_offsets[g + 1]], ascending; info: the figures `timings` receives).
    ValueError for 2^32 regions or more in all.
    timings (a dict) receives regions_s (the sweep: loading, upload, Engine.region_graph, the store), seam_ms (of that, the seams:
    host milliseconds around the upload of the store's plane, the kernel and the download of its keys), merge_s, provisional_regions,
    merged_regions, seam_pairs (distinct cross-cut pairs) and cores.
    _regions: a function with Engine.region_graph's contract on a HOST array -- _regions(core [x, y, z], label_bytes, shape, 3,
    mark, faces) -> (region ids 1..R per voxel as an array of that shape, value, count, face, pairs, info) -- that runs instead of
    the engine; the seams are then made by numpy and nothing touches the GPU (the host-logic tests)."""
    shape = tuple(int(v) for v in dataset.shape)
    if len(shape) not in (2, 3):
        raise intake.DimensionError("region_graph_chunked needs a dataset of two or three axes. Got: {}".format(shape))
    core_lo, core_hi, _, _ = halo_boxes(shape, chunk_shape, 0)
    shape = (shape + (1,))[:3]
    extent = np.array(shape, dtype=np.int64)
    eng = ops.engine() if _regions is None else None
    store = np.zeros(shape, dtype=np.uint32, order="F") if region_store is None else region_store
    if tuple(int(v) for v in store.shape) != shape or np.dtype(store.dtype) != np.uint32:
        raise ValueError("region_store: u32 of shape {}. Got: {} of shape {}".format(shape, store.dtype, tuple(store.shape)))
    bases = np.zeros(core_lo.shape[0] + 1, dtype=np.int64)
    values, faces, core_pairs, seams = [np.zeros(1, dtype=np.uint64)], [np.zeros(1, dtype=np.uint8)], [], []
    seam_ms, base = 0.0, 0
    t0 = time.perf_counter()
    for k in range(core_lo.shape[0]):                                       # raster order (x fastest): a lower neighbour comes first
        lo, hi = core_lo[k], core_hi[k]
        ext = tuple(int(v) for v in hi - lo)
        host = _load_box(dataset, lo, hi)
        if host.shape != ext:
            raise ValueError("region_graph_chunked: dataset[{}:{}] has shape {}".format(lo.tolist(), hi.tolist(), host.shape))
        if host.dtype == np.bool_:
            host = host.view(np.uint8)
        if host.dtype.kind not in "ui":
            raise TypeError("labels must be integers or bool")
        on_face = sum(1 << (2 * a) for a in range(3) if lo[a] == 0) | sum(2 << (2 * a) for a in range(3) if hi[a] == extent[a])
        if eng is None:
            region, value, _, face, pairs, _ = _regions(host, host.dtype.itemsize, ext, 3, lambda name: None, on_face)
            region = np.asarray(region).reshape(ext, order="F")
        else:
            d_flat, itemsize, _, _, _, _ = _device_labels(eng, host)
            region, value, _, face, pairs, _ = eng.region_graph(d_flat, itemsize, ext, 3, faces=on_face)
        n_regions = int(value.size) - 1
        if base + n_regions >= 2 ** 32:
            raise ValueError("region_graph_chunked: fewer than 2^32 regions in all (core {} ends at {})".format(k, base + n_regions))
        if eng is None:
            ids = (region.astype(np.int64) + base).astype(np.uint32)
        else:
            d_ids = region + (base - 2 ** 32 if base >= 2 ** 31 else base)  # (u32 words in an int32 tensor: the sum wraps)
            ids = d_ids.cpu().numpy().view(np.uint32).reshape(ext, order="F")
        store[tuple(slice(int(a), int(b)) for a, b in zip(lo, hi))] = ids
        values.append(value[1:])
        faces.append(face[1:])
        shift = np.uint64(base)
        core_pairs.append((((pairs >> np.uint64(32)) + shift) << np.uint64(32)) | ((pairs & np.uint64(0xFFFFFFFF)) + shift))
        t1 = time.perf_counter()
        for axis in range(3):
            if lo[axis] == 0:
                continue
            at = [slice(int(a), int(b)) for a, b in zip(lo, hi)]
            at[axis] = slice(int(lo[axis]) - 1, int(lo[axis]))
            low = np.take(_load_box(store, [s.start for s in at], [s.stop for s in at]), 0, axis=axis)
            if eng is None:
                high = np.take(ids, 0, axis=axis)
                keys = np.unique((low.astype(np.uint64) << np.uint64(32)) | high.astype(np.uint64))
            else:
                cube = d_ids.view(ext[2], ext[1], ext[0])                   # (the device array is Fortran ordered: [z, y, x] here)
                d_high = cube.select(2 - axis, 0).contiguous().view(-1)
                d_low = eng.torch.from_numpy(np.ascontiguousarray(low.T).view(np.int32).reshape(-1)).to(eng.device)
                keys, _, _ = eng.region_seam_pairs(d_low, d_high)
            seams.append(keys)
        seam_ms += (time.perf_counter() - t1) * 1e3
        base += n_regions
        bases[k + 1] = base
    regions_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    cat = lambda parts, dtype: np.concatenate(parts) if parts else np.zeros(0, dtype=dtype)
    seam_keys = cat(seams, np.uint64)
    merged, value, face, pairs = _merge_regions(np.concatenate(values), np.concatenate(faces), cat(core_pairs, np.uint64), seam_keys)
    by_region = np.argsort(merged[1:], kind="stable").astype(np.uint32) + np.uint32(1)
    member_offsets = np.concatenate([np.zeros(2, dtype=np.int64), np.cumsum(np.bincount(merged[1:], minlength=value.size)[1:])])
    merge_s = time.perf_counter() - t0
    info = dict(regions_s=regions_s, seam_ms=seam_ms, merge_s=merge_s, provisional_regions=int(base), merged_regions=int(value.size) - 1,
                seam_pairs=int(seam_keys.size), cores=int(core_lo.shape[0]))
    if timings is not None:
        timings.update(info)
    return RegionGraph(store, value, face, pairs, bases, member_offsets, by_region, info)


def cross_sectional_area_chunked(dataset, skeletons, chunk_shape=(512, 512, 512), halo=64, anisotropy=(1, 1, 1), smoothing_window=1,
                                 step=1, multipass=False, repair_contacts=False, max_box_voxels=None, progress=False, timings=None,
                                 fill_holes=False, visualize_section_planes=False, _sections=None):
    """kimimaro_amd.cross_sectional_area for a dataset that is never resident as a whole: the other half of what
    igneous does around kimimaro.  The result is DEFINED as what cross_sectional_area(whole dataset, skeletons, ...) returns, bit for
    bit in cross_sectional_area and equal in cross_sectional_area_contacts (whose bits name the faces of the DATASET), wherever a
    box large enough could be loaded; the dataset may hold 2^32 voxels or more, which cross_sectional_area refuses.

    dataset: what skeletonize_chunked takes.  skeletons: a dict, a list or one Skeleton, vertices in DATASET coordinates (what
    skeletonize_chunked returns); changed in place and returned.  anisotropy, smoothing_window, step, multipass, repair_contacts,
    the attributes, the extra_attributes entries and the skip rules: cross_sectional_area's.

    The (vertex, normal) pairs are made once from the whole skeletons, so a path that crosses a cut has the normals of an unchunked
    run.  The cores of plan.halo_boxes(dataset.shape, chunk_shape, halo) partition the dataset.  Round 0 visits every core once,
    loads its box (the core widened by `halo` voxels, clamped), counts the skeletons' labels in the core and runs the sections whose
    vertex lies in the core in one launch (kh_cross_sections_box).  A section that reached a face of its box that is a cut through
    the dataset (clip != 0) is run again in round r = 1, 2, ... in the box of its core at halo * 2^r, those sections alone, until
    none is clipped: a box equal to the dataset clips nothing.  Boxes run one after the other on one engine.

    max_box_voxels: the largest box that is loaded (default: sized from the free HBM, _xs_box_budget); never 2^32 - 1 voxels or more.
    A section whose next box would exceed it keeps its last values and gets bit 64 in cross_sectional_area_contacts: "clipped by
    the largest box tried, the area may be an underestimate" (bits 1..32 keep cross_sectional_area's meaning).  ValueError when
    a box of round 0 does not fit already, and for halo < 1.
    Where cross_sectional_area launches again (a vertex whose area came back 0 and that occurs again on another path), the boxes
    start again at `halo`.  fill_holes=True raises NotImplementedError here: cross_sectional_area_filled_chunked is that option.
    visualize_section_planes=True raises NotImplementedError too; progress: no effect.
    timings (a dict) receives calls (per launch of the driver loop a dict of `boxes` loaded and `items` run, one entry per growth
    round), cores, boxes_loaded, voxels_loaded, items (round 0), items_rerun (growth rounds), capped_items, kernel_ms (HIP events),
    load_s (host: loading, upload, counting), and rounds, vertices, occurrences of the driver loop.
    _sections: a function with the signature of section.cross_sections_box that runs the boxes instead; it is handed the box as the
    host array and the labels themselves as words, and nothing here touches the GPU (the host-logic tests).  Without it there is no
    CPU fallback: HipUnavailableError without the library or an MI355X."""
    utility._xs_check_arguments(step, smoothing_window, visualize_section_planes)
    if fill_holes:
        raise NotImplementedError("cross_sectional_area_chunked(fill_holes=True) keeps raising at this entry point; the sections of "
                                  "filled labels of a dataset in boxes are cross_sectional_area_filled_chunked, which takes the same "
                                  "arguments and a region_store")
    return _xs_chunked("cross_sectional_area_chunked", False, None, dataset, skeletons, chunk_shape, halo, anisotropy, smoothing_window,
                       step, multipass, repair_contacts, max_box_voxels, timings, _sections, None)


def cross_sectional_area_filled_chunked(dataset, skeletons, chunk_shape=(512, 512, 512), halo=64, anisotropy=(1, 1, 1),
                                        smoothing_window=1, step=1, multipass=False, repair_contacts=False, max_box_voxels=None,
                                        progress=False, timings=None, visualize_section_planes=False, region_store=None,
                                        _sections=None, _regions=None):
    """kimimaro_amd.cross_sectional_area_filled for a dataset that is never resident as a whole: the result is DEFINED
    as what cross_sectional_area_filled(whole dataset, skeletons, ...) returns -- bit for bit in cross_sectional_area, equal in
    cross_sectional_area_contacts -- wherever a box large enough could be loaded.  hole(L) is taken on the DATASET: a cavity that
    reaches a cut between two cores is a hole if it is closed in the dataset, and one that is closed in a core's view but joined to
    a face of the dataset through another core is none.  A dataset with an axis of extent 1 has no holes.

    Every argument, the rounds, the growth of the boxes, bit 64 and the skip rules (which count the label as given) are
    cross_sectional_area_chunked's.  In front of the boxes one more sweep over the cores builds the region graph of the dataset
    (region_graph_chunked; only when a skeleton has a label) and kh_host_enclosed_regions lists hole(L) for the skeletons' labels;
    every box then loads its slice of the region store beside its labels and runs kh_cross_sections_filled_box with the lists cut
    down to the cores the box intersects.  A vertex in a hole voxel of its label is a valid seed, in a box that holds no voxel of
    the label too.

    region_store: where the region id of every voxel is kept between the sweep and the boxes: an array-like of the dataset's shape
    (three axes), u32, indexed [x, y, z], read and written by slices -- an np.memmap, say.  Default: a numpy array in host memory.
    Either way it costs 4 BYTES PER VOXEL OF THE DATASET.  max_box_voxels' default counts 4 more bytes per voxel, the region box.
    timings receives cross_sectional_area_chunked's entries and regions_s, seam_ms, merge_s, provisional_regions, merged_regions,
    seam_pairs (region_graph_chunked), enclosed_ms (the host search) and listed_ids (hole regions over all labels, provisional ids).
    _sections: a function with the signature of section.cross_sections_filled_box, handed the box and its region box as host arrays
    [x, y, z], the labels themselves as words and the lists as a host array; _regions: region_graph_chunked's.  With both nothing
    touches the GPU (the host-logic tests).  Without them there is no CPU fallback."""
    utility._xs_check_arguments(step, smoothing_window, visualize_section_planes)
    return _xs_chunked("cross_sectional_area_filled_chunked", True, region_store, dataset, skeletons, chunk_shape, halo, anisotropy,
                       smoothing_window, step, multipass, repair_contacts, max_box_voxels, timings, _sections, _regions)


def _xs_chunked(name, filled, region_store, dataset, skeletons, chunk_shape, halo, anisotropy, smoothing_window, step, multipass,
                repair_contacts, max_box_voxels, timings, _sections, _regions):
    """the body of cross_sectional_area_chunked and cross_sectional_area_filled_chunked (filled), after the argument checks"""
    if int(halo) != halo or int(halo) < 1:
        raise ValueError("{}: halo must be a positive integer. Got: {}".format(name, halo))
    if filled and (_sections is None) != (_regions is None):
        raise ValueError("{}: _sections and _regions come together".format(name))
    eng = ops.engine() if _sections is None else None    # raises HipUnavailableError without the library or a gfx950 device
    run_sections = (section.cross_sections_filled_box if filled else section.cross_sections_box) if _sections is None else _sections
    an = utility._xs_anisotropy(anisotropy)
    an64 = an.astype(np.float64)
    shape = tuple(int(v) for v in dataset.shape)
    if len(shape) not in (2, 3):
        raise intake.DimensionError("{} needs a dataset of two or three axes. Got: {}".format(name, shape))
    core_lo, core_hi, _, _ = halo_boxes(shape, chunk_shape, 0)
    shape = (shape + (1,))[:3]
    extent = np.array(shape, dtype=np.int64)
    n_cores = int(core_lo.shape[0])
    dtype = _load_box(dataset, (0, 0, 0), (1, 1, 1)).dtype
    if dtype != np.bool_ and dtype.kind not in "ui":
        raise TypeError("labels must be integers or bool")
    is_bool = dtype == np.bool_
    span = (0, 1) if is_bool else (int(np.iinfo(dtype).min), int(np.iinfo(dtype).max))
    limit = 2 ** 32 - 2
    if max_box_voxels is None and eng is not None:
        max_box_voxels = _xs_box_budget(eng, dtype.itemsize, 4 if filled else 0)
    if max_box_voxels is not None:
        limit = min(limit, int(max_box_voxels))

    skels = utility._skeleton_list(skeletons)
    labels_of = [utility._label_of(s, is_bool) for s in skels]
    table = sorted({L for L in labels_of if L is not None})              # a job's word: the place of its label here
    place = {L: k for k, L in enumerate(table)}
    jobs = [(s, place[L], (0, 0, 0)) for s, L in zip(skels, labels_of) if L is not None]
    kept = [(getattr(s, "cross_sectional_area", None), getattr(s, "cross_sectional_area_contacts", None)) for s, _, _ in jobs]
    counts = np.zeros(len(table), dtype=np.int64)                        # voxels per label, from the cores of the first sweep
    total = dict(calls=[], cores=n_cores, boxes_loaded=0, voxels_loaded=0, items=0, items_rerun=0, capped_items=0, load_s=0.0)
    stats, state = {}, {"counted": False}
    none = np.zeros(0, dtype=np.int64)

    graph, hole_ids = None, [np.zeros(0, dtype=np.uint32)] * len(table)  # (filled) per entry of `table`: hole(L), provisional ids
    if filled and jobs:
        graph = region_graph_chunked(dataset, chunk_shape, region_store, total, _regions)
        known = [L for L in table if span[0] <= L <= span[1]]
        t0 = time.perf_counter()
        for L, ids in zip(known, hole_lists(graph, [L % (1 << (8 * dtype.itemsize)) for L in known])):
            hole_ids[place[L]] = ids
        total["enclosed_ms"] = (time.perf_counter() - t0) * 1e3
        total["listed_ids"] = int(sum(ids.size for ids in hole_ids))

    def box_holes(lo, hi):
        """-> (per entry of `table` where its list starts and how many ids it has, the lists): hole(L) cut down to the regions of
        the cores that the box [lo, hi) intersects -- no other region has a voxel in the box"""
        meets = np.all((core_lo < hi) & (core_hi > lo), axis=1)
        parts, begin, count = [], np.zeros(len(table), dtype=np.uint32), np.zeros(len(table), dtype=np.uint32)
        for w, ids in enumerate(hole_ids):
            if ids.size:
                ids = ids[meets[np.searchsorted(graph.bases, ids, side="left") - 1]]       # core k owns bases[k] + 1 .. bases[k + 1]
                begin[w], count[w] = sum(p.size for p in parts), ids.size
                parts.append(ids)
        return begin, count, np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint32)

    def box_labels(host, lo, k, count):
        """-> (the box for run_sections, bytes per label, per entry of `table` the word it has in this box or -1)"""
        words = np.full(len(table), -1, dtype=np.int64)
        inner = tuple(slice(int(a), int(b)) for a, b in zip(core_lo[k] - lo, core_hi[k] - lo))
        if eng is None:
            d_lab, label_bytes = host, host.dtype.itemsize
            for L in table:
                if span[0] <= L <= span[1]:
                    words[place[L]] = L % (1 << 32)
            if count:
                values, found = np.unique(host[inner], return_counts=True)
                for v, c in zip(values.tolist(), found.tolist()):
                    if int(v) in place:
                        counts[place[int(v)]] += c
            return d_lab, label_bytes, words
        d_flat, itemsize, _, ext, _, _ = _device_labels(eng, host)
        d_lab, label_bytes, device_word = utility._narrow_labels(eng, d_flat, itemsize, span, table)
        for L, w in device_word.items():
            words[place[L]] = w
        if count and device_word:
            core = d_lab.view(ext[2], ext[1], ext[0])[inner[2], inner[1], inner[0]].reshape(-1)
            found = utility._label_voxel_counts(eng, core, device_word.values())
            for L, w in device_word.items():
                counts[place[L]] += found[w]
        return d_lab, label_bytes, words

    def run_box(k, reach, vox, wrd, nrm, count):
        """the sections (vox, wrd, nrm) in the box of core k at halo `reach` -> (area, contact, clip), None when it may not be loaded"""
        lo, hi = np.maximum(core_lo[k] - reach, 0), np.minimum(core_hi[k] + reach, extent)
        ext = tuple(int(v) for v in hi - lo)
        if ext[0] * ext[1] * ext[2] > limit:
            return None
        t0 = time.perf_counter()
        host = _load_box(dataset, lo, hi)
        if host.shape != ext:
            raise ValueError("{}: dataset[{}:{}] has shape {}".format(name, lo.tolist(), hi.tolist(), host.shape))
        d_lab, label_bytes, words = box_labels(host, lo, k, count)
        total["load_s"] += time.perf_counter() - t0
        total["boxes_loaded"] += 1
        total["voxels_loaded"] += ext[0] * ext[1] * ext[2]
        seed = section.seed_index(vox - lo, ext)
        if not filled:
            want = words[wrd]
            seed[want < 0] = section.OUTSIDE                             # a label this box cannot hold
            area, contact, clip, _ = run_sections(eng, d_lab, label_bytes, lo, ext, shape, an64, seed,
                                                  np.maximum(want, 0).astype(np.uint32), nrm, stats)
            return area, contact, clip
        t0 = time.perf_counter()
        begin, listed, ids = box_holes(lo, hi)
        regions = _load_box(graph.store, lo, hi)
        # a label the box cannot hold may still have hole voxels in it, and a seed in one is valid: such a label
        # gets a word that no voxel of the box carries.  Only renumbered labels (eight bytes) can lack a word for a label they hold
        lost = (words < 0) & (listed > 0)
        if lost.any():
            words[lost] = int(d_lab.max().item()) + 1
        want = words[wrd]
        seed[want < 0] = section.OUTSIDE                                 # neither the label nor one of its holes
        if eng is not None:
            t = eng.torch
            regions = t.from_numpy(np.asfortranarray(regions).reshape(-1, order="F").view(np.int32)).to(eng.device)
            ids = t.from_numpy((ids if ids.size else np.zeros(1, dtype=np.uint32)).view(np.int32)).to(eng.device)
        total["load_s"] += time.perf_counter() - t0
        area, contact, clip, _ = run_sections(eng, d_lab, label_bytes, lo, ext, shape, an64, seed, np.maximum(want, 0).astype(np.uint32),
                                              nrm, (regions, begin[wrd], listed[wrd], ids), stats)
        return area, contact, clip

    def hook(vox, wrd, nrm):
        cores = core_of(vox, shape, chunk_shape)

        def launch(which):
            which = np.asarray(which, dtype=np.int64)
            area, contact = np.zeros(which.size, dtype=np.float32), np.zeros(which.size, dtype=np.uint8)
            call = dict(boxes=[], items=[])
            total["calls"].append(call)
            pending, reach, grown = np.arange(which.size, dtype=np.int64), int(halo), 0
            sweep = not state["counted"]                                 # the first launch visits every core, for the counts
            while pending.size or sweep:
                at = cores[which[pending]]
                order = np.argsort(at, kind="stable")
                ks, first = np.unique(at[order], return_index=True)
                group = dict(zip(ks.tolist(), np.split(pending[order], first[1:])))
                clipped, boxes = [none], 0
                for k in (range(n_cores) if sweep else ks.tolist()):
                    sel = group.get(k, none)
                    got = run_box(k, reach, vox[which[sel]], wrd[which[sel]], nrm[which[sel]], sweep)
                    if got is None:
                        if grown == 0:
                            raise ValueError("{}: the box of core {} at halo {} exceeds max_box_voxels = {}".format(name, k, reach, limit))
                        contact[sel] |= XS_CLIPPED
                        total["capped_items"] += int(sel.size)
                        continue
                    boxes += 1
                    area[sel], contact[sel] = got[0], got[1]
                    clipped.append(sel[got[2] != 0])
                call["boxes"].append(boxes)
                call["items"].append(int(pending.size))
                total["items" if grown == 0 else "items_rerun"] += int(pending.size)
                state["counted"], sweep = True, False
                pending = np.sort(np.concatenate(clipped))
                reach, grown = 2 * reach, grown + 1
            return area, contact

        return launch

    if jobs:
        utility._xs_run(None, None, None, shape, an, jobs, smoothing_window, step, multipass, repair_contacts, stats, launch_hook=hook)
        if not state["counted"]:                                         # (no vertex lies on a path: the counts decide -1 or 0 all the same)
            hook(np.zeros((0, 3), dtype=np.int64), np.zeros(0, dtype=np.uint32), np.zeros((0, 3)))(none)
        for (s, word, _), (area, contact) in zip(jobs, kept):           # utility.py:141-154, once the counts are known
            if counts[word] < 2:
                for name, value in (("cross_sectional_area", area), ("cross_sectional_area_contacts", contact)):
                    if value is None:
                        delattr(s, name)
                    else:
                        setattr(s, name, value)
    utility._xs_finish(skels)
    if timings is not None:
        timings.update(total, kernel_ms=stats.get("kernel_ms", 0.0), rounds=stats.get("rounds", 0), vertices=stats.get("vertices", 0),
                       occurrences=stats.get("occurrences", 0))
    return skeletons


# ---------------------------------------------------------------------------------------------------------------
# kh_neighbor_mask's directions: bit k of a mask is DIRECTIONS[k]
DIRECTIONS = tuple((dx, dy, dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dx, dy, dz) != (0, 0, 0))


def _slices(lo, hi):
    return tuple(slice(int(a), int(b)) for a, b in zip(lo, hi))


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
    shape0 = tuple(int(v) for v in dataset.shape)
    if len(shape0) not in (2, 3):
        raise intake.DimensionError("oversegment_chunked needs a dataset of two or three axes. Got: {}".format(shape0))
    core_lo, core_hi, box_lo, box_hi = halo_boxes(shape0, chunk_shape, 1)
    shape = (shape0 + (1,))[:3]
    extent = np.array(shape, dtype=np.int64)
    chunk = np.array((tuple(int(v) for v in chunk_shape) + (1,))[:3], dtype=np.int64)
    cores_per_axis = (extent + chunk - 1) // chunk
    n_cores = int(core_lo.shape[0])
    box_voxels = [int(e[0]) * int(e[1]) * int(e[2]) for e in box_hi - box_lo]
    if max(box_voxels) >= 2 ** 32:
        raise ValueError("oversegment_chunked: a box of {} voxels does not fit the 32-bit indices of a volume".format(max(box_voxels)))
    dtype = _load_box(dataset, (0, 0, 0), (1, 1, 1)).dtype
    if dtype != np.bool_ and dtype.kind not in "ui":
        raise TypeError("labels must be integers or bool")
    is_bool = dtype == np.bool_
    span = (0, 1) if is_bool else (int(np.iinfo(dtype).min), int(np.iinfo(dtype).max))
    stores = []
    for name, given, kind in (("distance_store", distance_store, np.float32), ("feature_store", feature_store, np.uint32)):
        store = np.empty(shape, dtype=kind, order="F") if given is None else given
        if tuple(int(v) for v in store.shape) != shape or np.dtype(store.dtype) != np.dtype(kind):
            raise ValueError("{}: {} of shape {}. Got: {} of shape {}".format(name, np.dtype(kind).name, shape, store.dtype, tuple(store.shape)))
        stores.append(store)
    d_store, f_store = stores

    # every vertex of every skeleton gets a provisional number in the container's order, as in oversegment
    skeletons = copy.deepcopy(skeletons)
    skels = utility._skeleton_list(skeletons)
    labels_of = [utility._label_of(s, is_bool) for s in skels]
    table = sorted({L for L in labels_of if L is not None and span[0] <= L <= span[1]})    # (one outside the span occurs nowhere)
    place = {L: w for w, L in enumerate(table)}
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
    core_all = core_of(vox_all, shape, tuple(chunk))
    active = (core_all >= 0) & (word_all >= 0)           # the vertices that may seed; single-voxel labels leave after phase 1

    def of_core(which):
        """the entries of `which` (indices into the vertices) per core, in ascending order"""
        order = which[np.argsort(core_all[which], kind="stable")]
        ks, first = np.unique(core_all[order], return_index=True)
        return dict(zip(ks.tolist(), np.split(order, first[1:])))

    verts_of = of_core(np.flatnonzero(core_all >= 0))
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

    def up(box):
        """a Fortran-ordered host box of 32-bit words -> device, float32 as it is, u32 as int32 words"""
        flat = box.reshape(-1, order="F")
        return eng.torch.from_numpy(flat.view(np.int32) if flat.dtype == np.uint32 else flat).to(eng.device)

    def core_down(d_box, ext, inner):
        """the core of a device box -> host [x, y, z]"""
        cut = d_box.view(ext[2], ext[1], ext[0])[inner[2], inner[1], inner[0]].contiguous().cpu().numpy()
        return cut.transpose(2, 1, 0)

    def visit(k, phase, written):
        """one visit of core k -> the directions (bits) whose neighbouring cores have to look again"""
        lo, hi = box_lo[k], box_hi[k]
        ext = tuple(int(v) for v in hi - lo)
        in_lo, in_hi = core_lo[k] - lo, core_hi[k] - lo
        inner = _slices(in_lo, in_hi)
        t0 = time.perf_counter()
        host = _load_box(dataset, lo, hi)
        if host.shape != ext:
            raise ValueError("oversegment_chunked: dataset[{}:{}] has shape {}".format(lo.tolist(), hi.tolist(), host.shape))
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
                values, found = np.unique(host[inner], return_counts=True)
                for v, c in zip(values.tolist(), found.tolist()):
                    if int(v) in place:
                        counts[place[int(v)]] += c
            now = old.copy()
            for i, (x, y, z) in zip(mine.tolist(), local.tolist()):
                if host[x, y, z] == table[word_all[i]]:                   # a vertex off its label seeds nothing
                    now[x, y, z] = 0 if phase == 1 else min(int(now[x, y, z]), i + 1)
            total_t["load_s"] += time.perf_counter() - t0
            t0 = time.perf_counter()
            now = np.asarray(_box(host, now, None, an, 1) if phase == 1 else _box(host, dist, now, an, 2), dtype=old.dtype)
            got = shell_diff(old, now, in_lo, in_hi)
            total_t["relax_ms"] += (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            if got[1] or not written[k]:
                store[_slices(core_lo[k], core_hi[k])] = now[inner]
        else:
            d_flat, itemsize, _, _, _, _ = _device_labels(eng, host)
            d_lab, label_bytes, device_word = utility._narrow_labels(eng, d_flat, itemsize, span, table)
            if not counted[k] and device_word:
                core = d_lab.view(ext[2], ext[1], ext[0])[inner[2], inner[1], inner[0]].reshape(-1)
                found = utility._label_voxel_counts(eng, core, device_word.values())
                for L, w in device_word.items():
                    counts[place[L]] += found[w]
            words = np.array([device_word.get(table[w], 0) for w in word_all[mine].tolist()], dtype=np.int64)
            held = words != 0                                              # (renumbered labels: one this box does not hold)
            lin = (local[:, 0] + ext[0] * (local[:, 1] + ext[1] * local[:, 2]))[held].astype(np.uint32)
            d_old = up(old)
            d_now = d_old.clone()
            d_dist = up(dist) if phase == 2 else None
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
            if got[1] or not written[k]:
                back = core_down(d_now, ext, inner)
                store[_slices(core_lo[k], core_hi[k])] = back.view(np.uint32) if phase == 2 else back
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
                at = np.array([k % cores_per_axis[0], (k // cores_per_axis[0]) % cores_per_axis[1], k // (cores_per_axis[0] * cores_per_axis[1])])
                for bit, step in enumerate(DIRECTIONS):
                    if (towards >> bit) & 1:
                        q = at + step
                        if np.all(q >= 0) and np.all(q < cores_per_axis):
                            dirty[int(q[0] + cores_per_axis[0] * (q[1] + cores_per_axis[1] * q[2]))] = True
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
            feature.first_appearance_box(eng, up(np.asfortranarray(f)), ext, (0, 0, 0), ext, lo, shape[0], shape[1], total, d_first)
    if eng is None:
        first[first == np.iinfo(np.int64).max] = -1
    else:
        first = d_first.cpu().numpy()
    lut, K = feature.first_appearance_map(first)
    d_lut = None if eng is None else up(lut)
    seg_all = np.zeros(total, dtype=np.uint64)
    for k in range(n_cores):
        lo, hi = core_lo[k], core_hi[k]
        ext = tuple(int(v) for v in hi - lo)
        f = np.asarray(_load_box(f_store, lo, hi), dtype=np.uint32)
        if eng is None:
            f = lut[np.where(f <= total, f, 0)]
        else:
            d_f = up(np.asfortranarray(f))
            feature.remap_u32(eng, d_f, d_lut, total, ext[0] * ext[1] * ext[2])
            f = core_down(d_f, ext, _slices((0, 0, 0), ext)).view(np.uint32)
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


# ---------------------------------------------------------------------------------------------------------------
def find_cycle(edges):
    """The cycle the reference's search reports for this edge list (skeletontricks.hpp:209-300), as a node sequence whose
    first and last entries are the same node; empty when the search meets no visited node.  Depth first from edges[0][0],
    neighbours in first-mention order, a node's whole neighbour list goes on the stack at once."""
    edges = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    if edges.shape[0] == 0:
        return []
    nbrs = defaultdict(dict)       # dict = insertion-ordered set
    for a, b in edges.tolist():
        nbrs[a][b] = None
        nbrs[b][a] = None
    todo = [(int(edges[0, 0]), -1, 0)]
    trail = []
    seen = set()
    node = -1
    while todo:
        node, via, depth = todo.pop()
        del trail[depth:]
        trail.append(node)
        if node in seen:
            break
        seen.add(node)
        todo.extend((c, node, depth + 1) for c in nbrs[node] if c != via)
    if len(trail) <= 1:
        return []
    first = next((k for k in range(len(trail) - 1) if trail[k] == node), len(trail) - 1)
    return trail[first:] if len(trail) - first >= 3 else []


def _drop_edges(edges, doomed):
    """edges (rows sorted) without every row that equals a row of `doomed` (post.py:576-588)."""
    edges = np.sort(edges, axis=1)
    if edges.size == 0 or len(doomed) == 0:
        return edges
    doomed = {(int(a), int(b)) for a, b in np.sort(np.asarray(doomed, dtype=np.int64).reshape(-1, 2), axis=1)}
    keep = np.fromiter(((int(a), int(b)) not in doomed for a, b in edges), dtype=bool, count=edges.shape[0])
    return edges[keep]


def _remove_loops_component(skel):
    """post.py:446-563 on one connected component."""
    nodes = skel.vertices
    edges = skel.edges.astype(np.int64)
    while True:
        cyc = find_cycle(edges)
        if not cyc:
            break
        ring = np.sort(np.stack([cyc[:-1], cyc[1:]], axis=1), axis=1)      # the cycle's edges, in walk order
        on_ring = np.unique(ring)
        ids, deg = np.unique(edges, return_counts=True)
        gates = on_ring[np.isin(on_ring, ids[deg >= 3])]                    # cycle nodes where something else attaches
        if gates.size == 0:                      # an isolated ring: gone
            edges = _drop_edges(edges, ring)
        elif gates.size == 1:                    # a ring on a stalk: replaced by a line to its farthest node
            d2 = np.sum((nodes[on_ring] - nodes[gates]) ** 2, axis=1)
            far = int(on_ring[int(np.argmax(d2))])
            edges = np.concatenate([_drop_edges(edges, ring), np.array([[int(gates[0]), far]], dtype=np.int64)])
        elif gates.size == 2:                    # a way in and a way out: the arc with fewer nodes stays
            walk = np.asarray(cyc[1:])
            at = np.flatnonzero(np.isin(walk, gates))
            if (at[1] - at[0]) < len(walk) / 2:
                arc = walk[at[0]:at[1] + 1]
            else:
                arc = np.concatenate([walk[at[1]:], walk[:at[0] + 1]])
            kept = {(int(a), int(b)) for a, b in np.sort(np.stack([arc[:-1], arc[1:]], axis=1), axis=1)}
            edges = _drop_edges(edges, [e for e in ring.tolist() if (e[0], e[1]) not in kept])
        else:                                    # many ways in: collapse onto the vertex nearest the gates' centroid ...
            centroid = np.mean(nodes[gates], axis=0)
            off = nodes - centroid
            hub = int(np.argmin(np.sum(off * off, axis=1)))
            reach = np.sqrt(np.max(np.sum((nodes[gates] - nodes[hub]) ** 2, axis=1)))
            if reach > skel.radii[hub]:          # ... unless that vertex is too thin to be the hub: snip one edge instead
                edges = _drop_edges(edges, ring[:1])
                continue
            spokes = np.array([[int(g), hub] for g in gates if int(g) != hub], dtype=np.int64).reshape(-1, 2)
            edges = np.concatenate([_drop_edges(edges, ring), spokes])
    skel.edges = edges.astype(np.uint32)
    return skel


def remove_loops(skeleton):
    """skeletons are trees: every cycle is removed, by the rule its number of outside connections selects (post.py:436-563)."""
    if skeleton.empty():
        return skeleton
    return Skeleton.simple_merge([_remove_loops_component(c) for c in skeleton.components()]).consolidate(
        remove_disconnected_vertices=False)   # post.py:260


# ---------------------------------------------------------------------------------------------------------------
def distance_graph(skel):
    """{(larger node, smaller node): float32 path length} between the critical points (terminal and branch nodes) of a
    tree, accumulated outward from its smallest terminal node (skeletontricks.pyx:122-170 -> skeletontricks.hpp:303-380)."""
    v = skel.vertices.astype(np.float32)
    edges = skel.edges.astype(np.int64)
    ids, deg = np.unique(edges, return_counts=True)
    critical = set(ids[(deg == 1) | (deg >= 3)].tolist())
    terminals = ids[deg == 1]
    if terminals.size == 0:
        raise ValueError("distance_graph: the component has no terminal node (it contains a cycle)")
    nbrs = defaultdict(list)
    for a, b in edges.tolist():
        nbrs[a].append(b)
        nbrs[b].append(a)
    start = int(terminals[0])
    out = {}
    seen = set()
    todo = [(start, -1, np.float32(0.0), start)]
    while todo:
        node, via, dist, root = todo.pop()
        if node in seen:
            raise ValueError("distance_graph: cycle detected at node %d" % node)
        seen.add(node)
        if node in critical and node != root:
            out[(max(root, node), min(root, node))] = float(dist)
            dist, root = np.float32(0.0), node
        for c in nbrs[node]:
            if c == via:
                continue
            d = v[node] - v[c]
            d = d * d
            step = np.sqrt(np.float32(np.float32(d[0] + d[1]) + d[2]))
            todo.append((c, node, np.float32(dist + step), root))
    return out


def _remove_ticks_component(skel, threshold):
    """post.py:262-362 on one tree."""
    if skel.empty():
        return skel
    span = distance_graph(skel)                     # superedge -> length, in creation order
    ids, deg = np.unique(skel.edges, return_counts=True)
    terminals = set(ids[deg == 1].tolist())
    arity = defaultdict(int)
    for node, d in zip(ids.tolist(), deg.tolist()):
        if d >= 3:
            arity[node] = d
    nbrs = defaultdict(set)
    for a, b in skel.edges.tolist():
        nbrs[a].add(b)
        nbrs[b].add(a)
    removable = {e for e in span if e[0] in terminals or e[1] in terminals}

    def fuse(x):
        """x is down to two superedges: they become one, which is removable from now on (post.py:324-336)"""
        joined = [e for e in span if x in e]
        total = 0.0
        ends = set()
        for e in joined:
            removable.discard(e)
            total += span.pop(e)
            ends.update(e)
        ends.discard(x)
        e = tuple(sorted(ends, reverse=True))
        span[e] = total
        removable.add(e)
        arity[x] = 0

    while len(span) > 1:
        tick = min(removable, key=lambda e: (span[e], e))
        a, b = tick
        if (arity[a] == 1 and arity[b] == 1) or span[tick] >= threshold:
            break
        # the unique path a .. b in what is left of the tree
        back = {a: None}
        todo = [a]
        while todo:
            node = todo.pop()
            if node == b:
                break
            for c in nbrs[node]:
                if c not in back:
                    back[c] = node
                    todo.append(c)
        node = b
        while back[node] is not None:
            nbrs[node].discard(back[node])
            nbrs[back[node]].discard(node)
            node = back[node]
        del span[tick]
        removable.remove(tick)
        arity[a] -= 1
        arity[b] -= 1
        if arity[a] == 2:
            fuse(a)
        if arity[b] == 2:
            fuse(b)
    out = skel.clone()
    left = sorted({(min(a, b), max(a, b)) for a in nbrs for b in nbrs[a]})
    out.edges = np.asarray(left, dtype=np.uint32).reshape(-1, 2)
    return out


def remove_ticks(skeleton, threshold):
    """Terminal branches shorter than `threshold` are removed one at a time, shortest first, the topology being
    re-evaluated after each removal (post.py:235-362)."""
    if skeleton.empty() or threshold == 0:
        return skeleton
    return Skeleton.simple_merge([_remove_ticks_component(c, threshold) for c in skeleton.components()]).consolidate(
        remove_disconnected_vertices=False)   # post.py:444
