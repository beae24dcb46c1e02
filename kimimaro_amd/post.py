"""Row f4: stitching the skeletons of adjacent chunks -- the counterpart of kimimaro/post.py.

    postprocess(skeleton, dust_threshold=1500, tick_threshold=3000)     kimimaro/post.py:49-87
    join_close_components(skeletons, radius=inf, restrict_by_radius)    kimimaro/post.py:89-218
    remove_dust / remove_loops / remove_ticks                            kimimaro/post.py:222-260, 436-563

    join_close_components_many(groups, radius=inf, restrict_by_radius)  the join of many groups at once,
    split_by_cluster, lift_edges                                        a group cut into the clusters that join independently
    postprocess_many(skeletons, dust_threshold=1500, tick_threshold=3000)
    skeletonize_chunked(dataset, chunk_shape, ...)                      a dataset in chunks to whole skeletons,
    place_fragment                                                      which composes postprocess_many with every box driver
    voxel_connectivity_graph_chunked(dataset, chunk_shape, out, ...)    the voxel graph of a dataset, box by box
    skeletonize_graph_chunked(dataset, chunk_shape, voxel_graph= | supervoxels=, merges=, ...)
                                                                        skeletonize_chunked with a voxel graph for every box

What else is done to a dataset in boxes lives in kimimaro_amd.boxes and the four driver modules on it, below this one, and is
imported here, so that every name stays reachable as kimimaro_amd.post.NAME (also what only a moved function used):

    boxes           the plumbing: route_targets, count_labels (and _load_box, axes, label_type, which skeletonize_chunked uses)
    region_boxes    the region graph and what fills from it: region_graph_chunked, hole_lists, RegionGraph, _merge_regions,
                    fill_all_holes_chunked
    section_boxes   the sections: cross_sectional_area_chunked, cross_sectional_area_filled_chunked, XS_CLIPPED
    segment_boxes   the segments: oversegment_chunked, shell_diff, DIRECTIONS
    point_boxes     the point queries: synapses_to_targets_chunked

The voxel graph of a dataset in boxes lives here, next to the driver it feeds: voxel_connectivity_graph_chunked, and
skeletonize_graph_chunked, which calls skeletonize_chunked through its _box_kwargs hook.

Host code on graphs of 10^2..10^5 nodes: the reference is Python here and so are the single-skeleton
functions; nothing in them touches the GPU path.  The two *_many functions do: the nearest pairs between all parts of all groups
come from one kernel call (csrc/join.hip through kimimaro_amd.points.part_gaps), the merge sequence from host C that reads only
that table (kh_host_join_plan), a group too large for one table is cut into independent clusters by a third (kh_part_clusters
through points.part_clusters); they have no CPU fallback.  Written from the behaviour of the reference, including the parts that are visible in its
results: which cycle its depth-first search reports first (skeletontricks.hpp:209-300: neighbours in the order the
edges list them, the search starts at the first edge), float32 branch lengths accumulated outward from the smallest
terminal node (skeletontricks.hpp:303-380), superedges fused at a branch point that drops to two edges and from then
on treated as removable whatever their ends are (post.py:324-336).  Where the reference leaves a choice to the
iteration order of a Python set (equal-length ticks, post.py:339) the smallest (length, nodes) pair is taken.
Pinned by tests/golden/post.npz: outputs of the reference's own post.py run on the vectors' inputs (generator and the
stand-ins it needs: tests/golden/make_golden.py `post`).
"""
from __future__ import annotations

import time
from collections import defaultdict

import numpy as np

from . import _abi, forest, intake, ops, points
from .boxes import _load_box, _store_box, axes, clip_graph, count_labels, down, label_type, route_targets, store_like
from .lanes import Lanes, lanes_for
from .plan import box_distance_bounds, chunk_grid, halo_boxes, nearest_first  # noqa: F401
from .point_boxes import synapses_to_targets_chunked
from .region_boxes import RegionGraph, _merge_regions, fill_all_holes_chunked, hole_lists, region_graph_chunked  # noqa: F401
from .section_boxes import XS_CLIPPED, cross_sectional_area_chunked, cross_sectional_area_filled_chunked  # noqa: F401
from .segment_boxes import DIRECTIONS, oversegment_chunked, shell_diff  # noqa: F401
from .skeleton import Skeleton
from .volume import DimensionError, _device_labels  # noqa: F401


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


def join_parts_many(groups):
    """join_parts for every group, the components of ALL their skeletons from one components_many call.  A component
    comes out of it consolidated -- vertices sorted and unique, edge rows sorted and unique, no vertex without an edge -- so the
    consolidate() of join_parts would hand back the same arrays and is not repeated."""
    groups = [[g] if isinstance(g, Skeleton) else list(g) for g in groups]
    comps = iter(components_many([s for g in groups for s in g]))
    return [[c for _ in g for c in next(comps) if not c.empty()] for g in groups]


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


def split_by_cluster(parts, cluster):
    """parts: the parts of ONE group; cluster: an id per part, equal for the parts of one cluster (any integers: the ids of
    kh_part_clusters are part numbers of a whole call).  Returns the sub-groups of the group, one per cluster of at least two parts,
    as a list of (members, their parts): members = the int64 indices into `parts` of the cluster's parts, ascending; the sub-groups
    are ordered by their first member.  A part alone in its cluster joins nothing and appears in no sub-group."""
    cluster = np.asarray(cluster).reshape(-1)
    if cluster.size != len(parts):
        raise ValueError("split_by_cluster: %d cluster ids for %d parts" % (cluster.size, len(parts)))
    if cluster.size == 0:
        return []
    by_id = np.argsort(cluster, kind="stable")           # the parts of a cluster next to each other, ascending among themselves
    cuts = np.flatnonzero(np.diff(cluster[by_id]) != 0) + 1
    runs = [run.astype(np.int64) for run in np.split(by_id, cuts) if run.size >= 2]
    runs.sort(key=lambda run: int(run[0]))
    return [(run, [parts[k] for k in run.tolist()]) for run in runs]


def lift_edges(edges, members, part_sizes):
    """edges: u32 [m, 2] in the numbering of a sub-group's concatenated parts (join_plan on the sub-group); members: the sub-group's
    parts as indices into the group (split_by_cluster); part_sizes: vertices per part of the GROUP.  Returns the same edges, u32
    [m, 2], in the numbering of the group's concatenated parts."""
    edges = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    members = np.asarray(members, dtype=np.int64).reshape(-1)
    sizes = np.asarray(part_sizes, dtype=np.int64).reshape(-1)
    first = np.concatenate([[0], np.cumsum(sizes)])      # of every part in the group's numbering
    own = np.concatenate([[0], np.cumsum(sizes[members])])          # of every member in the sub-group's
    if edges.size and (edges.min() < 0 or edges.max() >= own[-1]):
        raise ValueError("lift_edges: an edge names a vertex outside the sub-group's %d vertices" % int(own[-1]))
    k = np.searchsorted(own, edges, side="right") - 1    # the member a vertex belongs to (members are not empty)
    return (first[members[k]] + (edges - own[k])).astype(np.uint32).reshape(-1, 2)


def join_close_components_many(groups, radius=np.inf, restrict_by_radius=False, timings=None, split=None, parts_from="device"):
    """join_close_components for many groups at once: each group is a Skeleton or a sequence of them, the result per
    group what join_close_components(group, radius, restrict_by_radius) returns -- Skeleton.simple_merge of its parts plus one edge
    per merge, consolidated.  The nearest pairs between the parts of ALL groups come from one kernel call (a few when their tables
    exceed 1 GiB), every group with its own radius and bound under restrict_by_radius; the merge sequence of a group is decided on
    its table alone.  Where several tree vertices are equally near the winning query vertex the smallest index is taken (cKDTree
    makes its own choice there).  No CPU fallback: HipUnavailableError without the library or an MI355X.

    split: a group with a finite bound may first be cut into the sets of parts that are connected through pairs of boxes nearer than
    its bound (kh_part_clusters, one call for all such groups); every set of two or more parts is then joined as a group of its
    own, with the radius and bound of the WHOLE group, in the same kernel calls as the other groups, and its edges are put back.
    The result is the same (no record and no merge crosses two sets), the tables are the sets' squares instead of the group's.
    None (default): only the groups of more than 8 192 parts, which have no table of their own; True: every group with a finite
    bound; False: none.  A set of more than 8 192 parts is a ValueError, and so is a group of that size that is not split (an
    infinite radius, or split=False).
    parts_from: "device" (default): the parts of all groups come from one components_many call (join_parts_many);
    "host": from Skeleton.components() skeleton by skeleton (join_parts).  They are the same parts.
    timings (a dict): kernel_ms, copy_s, plan_s of the call; parts_s, the seconds spent making the parts; cluster_ms (HIP events
    around kh_part_clusters), clusters (the sets of two or more parts that were joined on their own) and largest_cluster (parts in the
    largest set; 0 when nothing was split)."""
    if radius is None:
        radius = np.inf
    if radius <= 0:
        raise ValueError("radius must be greater than zero: " + str(radius))
    eng = ops.engine()                                   # raises HipUnavailableError without the library or a gfx950 device
    groups = list(groups)
    if parts_from not in ("device", "host"):
        raise ValueError("parts_from must be 'device' or 'host': " + repr(parts_from))
    t0 = time.perf_counter()
    parts = join_parts_many(groups) if parts_from == "device" else [join_parts(g) for g in groups]
    parts_s = time.perf_counter() - t0
    radius_of = [float(radius)] * len(groups)
    if restrict_by_radius:
        radius_of = [max(2 * max(float(np.max(p.radii)) for p in ps), 0) if ps else 0.0 for ps in parts]
    bound2_of = [(r + 0.000001) * (r + 0.000001) for r in radius_of]
    todo = [g for g in range(len(groups)) if len(parts[g]) >= 2]
    cut = [g for g in todo if split is not False and np.isfinite(bound2_of[g])
           and (split or len(parts[g]) > points.GAP_MAX_PARTS)]
    members_of = {}                                      # group -> the members of its sub-groups
    clusters = largest = 0
    cluster_ms = {}
    if cut:
        _, _, boxes = points.part_boxes([p.vertices for g in cut for p in parts[g]])
        group_start = np.concatenate([[0], np.cumsum([len(parts[g]) for g in cut])])
        cluster = points.part_clusters(eng, boxes, group_start, [bound2_of[g] for g in cut], timings=cluster_ms)
        for k, g in enumerate(cut):
            ids = cluster[group_start[k]:group_start[k + 1]]
            members_of[g] = [members for members, _ in split_by_cluster(parts[g], ids)]
            sizes = np.unique(ids, return_counts=True)[1]
            if int(sizes.max()) > points.GAP_MAX_PARTS:
                raise ValueError("group %d: a cluster of %d parts connected through pairs nearer than the bound %r: more than %d, whose "
                                 "table of nearest pairs exceeds 1 GiB" % (g, int(sizes.max()), radius_of[g] + 0.000001,
                                                                           points.GAP_MAX_PARTS))
            clusters += len(members_of[g])
            largest = max(largest, int(sizes.max()))
    # what is joined on a table of its own: (group, None) for a whole group, (group, members) for a sub-group
    units = [(g, members) for g in todo for members in members_of.get(g, [None])]
    tables = points.part_gaps(eng, [[p.vertices for p in (parts[g] if members is None else [parts[g][k] for k in members.tolist()])]
                                    for g, members in units], [bound2_of[g] for g, _ in units], timings=timings)
    t0 = time.perf_counter()
    added = {g: [] for g in todo}
    sizes_of = {g: np.array([p.vertices.shape[0] for p in parts[g]], dtype=np.int64) for g in todo}
    for (g, members), (d2, idx) in zip(units, tables):
        ps = parts[g] if members is None else [parts[g][k] for k in members.tolist()]
        edges = join_plan(sizes_of[g] if members is None else sizes_of[g][members], d2, idx, np.concatenate([p.radii for p in ps]),
                          radius_of[g], restrict_by_radius)
        added[g].append(edges if members is None else lift_edges(edges, members, sizes_of[g]))
    out = [ps[0] if ps else Skeleton() for ps in parts]
    for g in todo:
        merged = Skeleton.simple_merge(parts[g])
        merged.edges = np.concatenate([merged.edges] + added[g])
        out[g] = merged.consolidate(remove_disconnected_vertices=True)
    if timings is not None:
        timings["plan_s"] = timings.get("plan_s", 0.0) + time.perf_counter() - t0
        timings["parts_s"] = timings.get("parts_s", 0.0) + parts_s
        timings["cluster_ms"] = timings.get("cluster_ms", 0.0) + cluster_ms.get("cluster_ms", 0.0)
        timings["clusters"] = timings.get("clusters", 0) + clusters
        timings["largest_cluster"] = max(timings.get("largest_cluster", 0), largest)
    return out


def components_many(skeletons):
    """Skeleton.components() for every skeleton of the list, from one device labelling of all of them (kh_forest_components, DESIGN.md
    3.22): per skeleton the list of its components, ordered by their smallest vertex, each with the arrays components() gives it.
    No CPU fallback: HipUnavailableError without the library or an MI355X."""
    eng = ops.engine()
    packed = [forest.consolidated(s) for s in skeletons]
    out = []
    for part in forest.batches(packed):
        f = forest.pack(packed[part])
        out.extend(forest.unpack_components(f, forest.labels(eng, f)))
    return out


def paths_many(skeletons, return_indices=True, stats=None):
    """[s.paths(return_indices=...) for s in skeletons], array for array, every tree of the list walked in one pass on the device
    (kh_walk_orient, kh_walk_emit).  The skeletons are taken AS GIVEN, not consolidated: vertex numbers are the
    caller's, and self loops, repeated, reversed and unsorted rows and vertices without an edge mean what Skeleton._neighbours makes
    of them.  Where the depth-first walk cuts a cycle is sequential: a skeleton with a cyclic component is walked by Skeleton.paths
    whole.  stats (a dict): walk_host (those skeletons), paths, occurrences (the vertices on all paths), walk_s (the device calls)
    and pack_s (the numpy around them) are added to.  No CPU fallback: HipUnavailableError without the library or an MI355X."""
    eng = ops.engine()
    skeletons = list(skeletons)
    out = []
    for part in forest.walk_batches(skeletons):
        group = skeletons[part]
        w = forest.walk(eng, group, stats=stats)
        for k, s in enumerate(group):
            paths = s.paths(return_indices=True) if w.host[k] else w.paths(k)
            out.append(paths if return_indices else [s.vertices[p] for p in paths])
        if stats is not None:
            stats["paths"] = stats.get("paths", 0) + int(w.pstart.size - 1)
            stats["occurrences"] = stats.get("occurrences", 0) + int(w.occ.size)
    return out


def remove_dust_many(skeletons, dust_threshold, stats=None):
    """remove_dust(skeleton, dust_threshold) for every skeleton of the list; an empty skeleton, and every skeleton
    under a zero threshold, comes back as the object it is.  The cable length of every component is summed on the device in another
    order than numpy's float32 sum, so the device decides a component only when |cable - T| > cable * ne * 2^-23 -- twice the bound
    (ne - 1) * 2^-24 on the relative error of a float32 sum of ne non-negative terms in any order, which also covers the order of
    the device's own f64 sum -- and the host's cable_length() > T decides the others and every component of 2^20 edges or more.
    stats (a dict): `components` and `dust_host_decided` are added to.  No CPU fallback."""
    eng = ops.engine()
    out = list(skeletons)
    todo = [k for k, s in enumerate(out) if not (s.empty() or dust_threshold == 0)]
    packed = [forest.consolidated(out[k]) for k in todo]
    ncomp = nhost = 0
    for part in forest.batches(packed):
        f = forest.pack(packed[part])
        m = forest.measure(eng, f)
        g = forest.Groups(f, m.comp)
        cable, ne = m.cable[g.root], m.ne[g.root].astype(np.float64)
        keep = cable > dust_threshold
        unsure = ~(np.abs(cable - dust_threshold) > cable * ne * 2.0 ** -23) | (ne >= forest.HOST_DUST_EDGES)
        for k in np.flatnonzero(unsure & (ne > 0)).tolist():
            keep[k] = forest.component_cable(f, g, k) > dust_threshold
            nhost += 1
        ncomp += int(np.count_nonzero(ne > 0))
        for k, skel in zip(todo[part], forest.unpack_dust(f, g, keep & (ne > 0))):
            out[k] = skel
    if stats is not None:
        stats["components"] = stats.get("components", 0) + ncomp
        stats["dust_host_decided"] = stats.get("dust_host_decided", 0) + nhost
    return out


def _all_trees(f, m):
    """per skeleton of the forest: it has edges and every component of it is a tree (ne == nv - 1, counted on the device)"""
    roots = np.flatnonzero(m.nv)
    cyclic = m.ne[roots].astype(np.int64) != m.nv[roots].astype(np.int64) - 1
    bad = np.zeros(len(f.skeletons), dtype=bool)
    bad[f.skeleton_of_vertex(roots[cyclic])] = True
    return ~bad & (np.diff(f.estart) > 0)


def remove_loops_many(skeletons, stats=None):
    """remove_loops(skeleton) for every skeleton of the list.  Whether a component holds a cycle is counted on the
    device; a skeleton of trees is returned as skeleton.consolidate(), which is what remove_loops makes of a forest (the skeleton
    itself where it is consolidated already: forest.consolidated), and a skeleton
    with a cyclic component goes through the host's remove_loops whole: the four cycle rules stay host code.  An empty skeleton comes
    back as the object it is.  stats (a dict): `loops_host`, the skeletons that took the host path, is added to.  No CPU fallback."""
    eng = ops.engine()
    out = list(skeletons)
    todo = [k for k, s in enumerate(out) if not s.empty()]
    packed = [forest.consolidated(out[k]) for k in todo]
    nhost = 0
    for part in forest.batches(packed):
        f = forest.pack(packed[part])
        trees = _all_trees(f, forest.measure(eng, f))
        for k, skel, ok in zip(todo[part], packed[part], trees.tolist()):
            if not ok:
                nhost += 1
            out[k] = skel if ok else remove_loops(out[k])
    if stats is not None:
        stats["loops_host"] = stats.get("loops_host", 0) + nhost
    return out


def remove_ticks_many(skeletons, threshold):
    """remove_ticks(skeleton, threshold) for every skeleton of the list, every tree of all of them in one kh_forest_ticks call
    (DESIGN.md 3.22): consolidated, the vertices that lost all their edges kept.  An empty skeleton, and every skeleton under a zero
    threshold, comes back as the object it is; a component with a cycle raises the ValueError of distance_graph.  No CPU fallback."""
    eng = ops.engine()
    out = list(skeletons)
    todo = [k for k, s in enumerate(out) if not (s.empty() or threshold == 0)]
    packed = [forest.consolidated(out[k]) for k in todo]
    for part in forest.batches(packed):
        f = forest.pack(packed[part])
        m = forest.measure(eng, f)
        trees = _all_trees(f, m)
        for skel, ok in zip(packed[part], trees.tolist()):
            if not ok and not skel.empty():
                for c in skel.components():
                    distance_graph(c)
                raise ValueError("distance_graph: a component contains a cycle")
        done = forest.unpack_ticks(f, forest.ticks(eng, f, m, threshold))
        for k, skel, ok in zip(todo[part], done, trees.tolist()):
            out[k] = skel if ok else remove_ticks(out[k], threshold)      # (without edges once consolidated: the host's answer)
    return out


def postprocess_many(skeletons, dust_threshold=1500.0, tick_threshold=3000.0, stages="device", stats=None):
    """postprocess for many skeletons: dust and loops out, the join of ALL of them in one join_close_components_many(
    restrict_by_radius=True) call, ticks out.
    stages="device" (default): remove_dust_many, remove_loops_many and remove_ticks_many around the join, each one pass over all
    skeletons; stats (a dict) is handed to them.  stages="host": the three per skeleton on the host.  The results
    are equal: every *_many function is defined as what the host function returns."""
    if stages not in ("device", "host"):
        raise ValueError("stages must be 'device' or 'host': " + repr(stages))
    skeletons = list(skeletons)
    ops.engine()                                         # raises HipUnavailableError without the library or a gfx950 device
    if stages == "device":
        cleaned = remove_loops_many(remove_dust_many([s.consolidate(remove_disconnected_vertices=True) for s in skeletons],
                                                     dust_threshold, stats=stats), stats=stats)
        joined = remove_ticks_many(join_close_components_many(cleaned, restrict_by_radius=True), tick_threshold)
        out = []
        for skeleton, skel in zip(skeletons, joined):
            skel.id = skeleton.id
            out.append(skel.consolidate(remove_disconnected_vertices=True))
        return out
    cleaned = []
    for skeleton in skeletons:
        skel = skeleton.consolidate(remove_disconnected_vertices=True)
        skel = remove_dust(skel, dust_threshold)
        cleaned.append(remove_loops(skel))
    out = []
    for skeleton, skel in zip(skeletons, join_close_components_many(cleaned, restrict_by_radius=True, parts_from="host")):
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


def skeletonize_chunked(dataset, chunk_shape=(512, 512, 512), teasar_params=None, anisotropy=(1, 1, 1), object_ids=None,
                        dust_threshold=1000, dust_global=False, post_dust_threshold=1500.0, tick_threshold=3000.0, merge=True,
                        fix_branching=True, fix_borders=True, fill_holes=False, fix_avocados=False, extra_targets_before=[],
                        extra_targets_after=[], progress=False, lanes=None, width=None, timings=None, _skeletonize=None,
                        _postprocess=None, _box_kwargs=None, cross_sectional_area=None, fill_holes_global=False, filled_store=None,
                        region_store=None, _fill=None, synapses=None, _synapse_targets=None):
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
    fill_holes_global: the holes of every label are filled on the DATASET first (fill_all_holes_chunked) and the
      result is DEFINED as skeletonize_chunked of the filled dataset with fill_holes=False: a cavity that a cut runs through is
      filled, what lay in it gets no skeleton.  fill_all_holes_chunked(dataset, chunk_shape, out=filled_store,
      region_store=region_store, return_fill_count=True) runs in front of everything; the dataset is not modified.  The labels of
      dust_global are counted on the filled store, every box is cut out of it and traced with fill_holes=False whatever
      `fill_holes` says, and cross_sectional_area= takes its sections on it.
    filled_store: where the filled dataset is kept, an array-like of the dataset's shape and dtype written and read by slices;
      default: a numpy array in host memory.  region_store: fill_all_holes_chunked's (4 bytes per voxel of the dataset).
    synapses: None, or {label: [(centroid, swc_label), ...]} in dataset voxel coordinates: the targets of
      synapses_to_targets_chunked(dataset, synapses, chunk_shape) are appended to extra_targets_after.  They are taken on the dataset
      as passed, not on the filled store of fill_holes_global: a label's own voxels are the same in both.
    progress: accepted, no effect.
    timings (a dict) receives count_s, chunks_s, place_s, fuse_s, post_s (seconds), chunks (boxes traced), fragments and vertices
      (of the placed fragments); with fill_holes_global also fill_s and filled (the fill count).
    _fill replaces fill_all_holes_chunked, _synapse_targets replaces synapses_to_targets_chunked (the host-logic tests hand them
      their hooks).
    _box_kwargs(eng, k, box_lo, box_hi) -> dict: further keyword arguments for the skeletonize call of box k, made by the lane that
      takes the box (eng: its engine; None under _skeletonize) -- how skeletonize_graph_chunked hands every box its voxel_graph.
    _skeletonize(labels, **kwargs) -> {label: Skeleton} runs the boxes one after the other in place of the lanes,
    _postprocess(skeletons, dust_threshold, tick_threshold) -> list replaces postprocess_many: with both, nothing here touches the GPU
      (the host-logic tests run the whole driver on the CPU oracle).  Without them there is no CPU fallback."""
    params = intake.DEFAULT_TEASAR_PARAMS if teasar_params is None else teasar_params
    if _skeletonize is None or (merge and _postprocess is None):
        ops.engine()                                     # raises HipUnavailableError without the library or a gfx950 device
    shape, _, _ = axes(dataset, "skeletonize_chunked")
    grid = chunk_grid(shape, chunk_shape)
    n = int(grid.box_lo.shape[0])
    extents = grid.box_hi - grid.box_lo
    largest = tuple(int(v) for v in extents[int(np.argmax(np.prod(extents, axis=1)))])
    if largest[0] * largest[1] * largest[2] >= 2 ** 32:
        raise ValueError("skeletonize_chunked: a box of {} voxels does not fit the 32-bit indices of a volume".format(largest))
    if synapses is not None:
        found = (synapses_to_targets_chunked if _synapse_targets is None else _synapse_targets)(dataset, synapses, chunk_shape)
        extra_targets_after = list(extra_targets_after) + list(found)
    before = route_targets(extra_targets_before, grid, shape)
    after = route_targets(extra_targets_after, grid, shape)
    wanted = None if object_ids is None else set(int(v) for v in object_ids)

    fill_s, filled = 0.0, 0
    if fill_holes_global:
        t0 = time.perf_counter()
        if filled_store is None:
            filled_store = np.empty(shape, dtype=label_type(dataset)[0], order="F")
        dataset, filled = (fill_all_holes_chunked if _fill is None else _fill)(dataset, chunk_shape, out=filled_store,
                                                                              region_store=region_store, return_fill_count=True)
        fill_holes = False
        fill_s = time.perf_counter() - t0

    t0 = time.perf_counter()
    kept = None
    if dust_global:
        kept = {label for label, count in count_labels(dataset, grid).items() if label != 0 and count > dust_threshold}
        if wanted is not None:
            kept &= wanted
    count_s = time.perf_counter() - t0

    def one(k, run, eng=None):
        labels = _load_box(dataset, grid.box_lo[k], grid.box_hi[k])
        ids, dust = object_ids, dust_threshold
        if kept is not None:
            ids = sorted(kept.intersection(np.unique(labels).tolist()))
            dust = 0
            if not ids:
                return None
        more = {} if _box_kwargs is None else _box_kwargs(eng, k, grid.box_lo[k], grid.box_hi[k])
        return run(labels, teasar_params=params, anisotropy=anisotropy, object_ids=ids, dust_threshold=dust, progress=False,
                   fix_branching=fix_branching, fix_borders=fix_borders, fill_holes=fill_holes, fix_avocados=fix_avocados,
                   extra_targets_before=before[k], extra_targets_after=after[k], **more)

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
            return one(k, lambda labels, **kw: intake.skeletonize(labels, _engine=eng, **kw), eng)

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
        if fill_holes_global:
            timings.update(fill_s=fill_s, filled=int(filled))
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
def voxel_connectivity_graph_chunked(dataset, chunk_shape=(512, 512, 512), out=None, connectivity=26, merges=None, stats=None):
    """voxel_connectivity_graph for a dataset that is never resident as a whole: DEFINED as what
    voxel_connectivity_graph(dataset, connectivity, merges) returns for the whole dataset, word for word.

    The cores of plan.halo_boxes(shape, chunk_shape, 1) partition the dataset; every core is loaded with one voxel around it (clamped
    to the dataset), goes through kh_voxel_graph, and the words of the core are written to `out`: a word needs the 26 neighbours of
    its voxel and nothing else.
    dataset: numpy of any order, an np.memmap, a tensor on the GPU, or any object with .shape and slicing over a tuple of slices; two
      or three axes, integers or bool.  It may hold 2^32 voxels or more: only a box has to stay below that.
    out: an array-like of the dataset's shape and dtype uint32, written by slices; default: a Fortran-ordered numpy array in host
      memory, 4 bytes per voxel of the dataset.  It is returned.
    connectivity, merges: as voxel_connectivity_graph.
    stats (a dict) receives cores, voxels_loaded, kernel_ms (HIP events around the kernel), load_s and store_s (seconds).
    No CPU fallback: HipUnavailableError without the library or an MI355X."""
    name = "voxel_connectivity_graph_chunked"
    if connectivity not in (6, 18, 26):
        raise ValueError("connectivity must be 6, 18 or 26. Got: {}".format(connectivity))
    shape0, _, _ = axes(dataset, name)
    core_lo, core_hi, box_lo, box_hi = halo_boxes(shape0, chunk_shape, 1)
    extents = box_hi - box_lo
    largest = tuple(int(v) for v in extents[int(np.argmax(np.prod(extents, axis=1)))])
    if largest[0] * largest[1] * largest[2] >= 2 ** 32:
        raise ValueError("{}: a box of {} voxels does not fit the 32-bit indices of a volume".format(name, largest))
    eng = ops.engine()                                   # raises HipUnavailableError without the library or a gfx950 device
    dtype, _, span = label_type(dataset)
    d_pairs = ops.pairs_to_device(eng, ops.merge_pairs(merges, span, dtype.itemsize))
    out = store_like(out, shape0, np.uint32, name)
    events = []
    loaded, load_s, store_s = 0, 0.0, 0.0
    for k in range(int(core_lo.shape[0])):
        t0 = time.perf_counter()
        box = _load_box(dataset, box_lo[k], box_hi[k], name)
        load_s += time.perf_counter() - t0
        loaded += int(box.size)
        d_box, itemsize, _, extent, _, _ = _device_labels(eng, box)
        start, end = (eng.torch.cuda.Event(enable_timing=True) for _ in range(2))
        start.record()
        d_graph = eng.voxel_graph(d_box, itemsize, extent, connectivity, d_pairs)
        end.record()
        events.append((start, end))
        inner = tuple(slice(int(a - b), int(c - b)) for a, b, c in zip(core_lo[k], box_lo[k], core_hi[k]))
        core = down(d_graph, extent, inner).view(np.uint32)
        t0 = time.perf_counter()
        _store_box(out, core_lo[k], core_hi[k], core)
        store_s += time.perf_counter() - t0
        del d_box, d_graph
    if stats is not None:
        eng.sync_stream()
        stats.update(cores=int(core_lo.shape[0]), voxels_loaded=loaded, kernel_ms=sum(a.elapsed_time(b) for a, b in events),
                     load_s=load_s, store_s=store_s)
    return out


def skeletonize_graph_chunked(dataset, chunk_shape=(512, 512, 512), voxel_graph=None, supervoxels=None, merges=None, teasar_params=None,
                              anisotropy=(1, 1, 1), object_ids=None, dust_threshold=1000, dust_global=False, post_dust_threshold=1500.0,
                              tick_threshold=3000.0, merge=True, fix_branching=True, fix_borders=True, fill_holes=False,
                              fix_avocados=False, extra_targets_before=[], extra_targets_after=[], progress=False, lanes=None,
                              width=None, timings=None, _skeletonize=None, _postprocess=None, cross_sectional_area=None, synapses=None,
                              _synapse_targets=None, _graph_of=None):
    """skeletonize_chunked with a voxel connectivity graph: DEFINED as the composition of DESIGN.md 3.15 with every
    box traced by skeletonize(box, voxel_graph=G_box, ...).  Exactly one of

    voxel_graph: the graph of the dataset, an array-like of the dataset's shape read by slices (uint32, cc3d's bit layout; what
      voxel_connectivity_graph_chunked writes, walls added by the caller included).  G_box = the slice of a box with every bit that
      leaves the box cleared (boxes.clip_graph): skeletonize reads such bits of a box that holds one value everywhere;
    supervoxels: a finer segmentation of the dataset, an array-like of its shape, with
    merges: the (m, 2) pairs of supervoxel values that belong together (NOT transitive; ops.voxel_connectivity_graph).  G_box =
      voxel_connectivity_graph(supervoxel box, 26, merges), built on the device by the lane that takes the box, from the box alone:
      no halo, no 4 B per voxel store.  A supervoxel boundary that `merges` does not list is a wall -- the self-touches (autapses)
      of an agglomerated label stay apart.

    Cleared of the leaving bits, both are the same function of the box: supervoxels=S, merges=M gives what
    voxel_graph=voxel_connectivity_graph_chunked(S, merges=M) gives.  Every other keyword is skeletonize_chunked's and means the
    same; fill_holes_global, filled_store, region_store and _fill are not accepted (a graph of the original voxels does not
    describe a filled dataset), and fix_avocados=True is a NotImplementedError before anything is loaded, as in skeletonize.
    ValueError: both or neither of voxel_graph / supervoxels, merges without supervoxels, one of them of another shape than the
    dataset.  _graph_of(box, merges=merges) -> uint32 graph replaces the device builder (the host-logic tests run the whole driver
    on the CPU oracle); without the hooks there is no CPU fallback."""
    name = "skeletonize_graph_chunked"
    if fix_avocados:
        raise NotImplementedError("{}(fix_avocados=True): the avocado pass re-labels components, which a graph of the ORIGINAL voxels "
                                  "does not describe".format(name))
    if (voxel_graph is None) == (supervoxels is None):
        raise ValueError("{}: exactly one of voxel_graph and supervoxels".format(name))
    if merges is not None and supervoxels is None:
        raise ValueError("{}: merges belongs to supervoxels".format(name))
    source = voxel_graph if voxel_graph is not None else supervoxels
    if tuple(int(v) for v in source.shape) != tuple(int(v) for v in dataset.shape):
        raise ValueError("{}: {} of shape {} for a dataset of shape {}".format(name, "voxel_graph" if voxel_graph is not None else "supervoxels",
                                                                               tuple(source.shape), tuple(dataset.shape)))
    pairs = None
    if supervoxels is not None and _graph_of is None:
        ops.engine()                                     # raises HipUnavailableError without the library or a gfx950 device
        dtype, _, span = label_type(supervoxels)
        pairs = ops.merge_pairs(merges, span, dtype.itemsize)

    def box_kwargs(eng, k, lo, hi):
        box = _load_box(source, lo, hi, name)
        if voxel_graph is not None:
            return {"voxel_graph": clip_graph(box)}
        if _graph_of is not None:
            return {"voxel_graph": _graph_of(box, merges=merges)}
        own = eng if eng is not None else ops.engine()
        d_box, itemsize, _, extent, _, _ = _device_labels(own, box)
        d_graph = own.voxel_graph(d_box, itemsize, extent, 26, ops.pairs_to_device(own, pairs))
        # (a lane's skeletonize takes the device words as they are; a caller's _skeletonize gets a host array)
        return {"voxel_graph": d_graph if eng is not None else down(d_graph, extent).view(np.uint32)}

    return skeletonize_chunked(dataset, chunk_shape, teasar_params=teasar_params, anisotropy=anisotropy, object_ids=object_ids,
                               dust_threshold=dust_threshold, dust_global=dust_global, post_dust_threshold=post_dust_threshold,
                               tick_threshold=tick_threshold, merge=merge, fix_branching=fix_branching, fix_borders=fix_borders,
                               fill_holes=fill_holes, fix_avocados=False, extra_targets_before=extra_targets_before,
                               extra_targets_after=extra_targets_after, progress=progress, lanes=lanes, width=width, timings=timings,
                               _skeletonize=_skeletonize, _postprocess=_postprocess, cross_sectional_area=cross_sectional_area,
                               synapses=synapses, _synapse_targets=_synapse_targets, _box_kwargs=box_kwargs)


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
