"""The voxel connectivity graph of DESIGN.md 3.21 / kh_voxel_graph (include/kimi_hip.h) restated with numpy slices -- nothing of the
product is imported here.  The word's layout is tests/prep_ref.py's CC3D_STEP_OF_BIT: bit b of a voxel's word allows the step
CC3D_STEP_OF_BIT[b] away from it.  Volumes are (x, y, z) arrays; two axes get a unit z axis and come back with two."""
import numpy as np

from prep_ref import CC3D_STEP_OF_BIT

CONNECTIVITY_BITS = {6: 6, 18: 18, 26: 26}       # the first n bits of the word are the steps of connectivity n


def _sides(step, shape):
    """slices (the voxels that have a neighbour at +step inside the volume, those neighbours)"""
    here = tuple(slice(max(0, -d), n - max(0, d)) for d, n in zip(step, shape))
    there = tuple(slice(max(0, d), n - max(0, -d)) for d, n in zip(step, shape))
    return here, there


def pair_list(merges):
    """`merges` -> the set of unordered pairs {a, b} it stands for, as a sorted list of (a, b) with a < b, Python ints: a pair that
    names 0 or one value twice is dropped; order and duplicates do not matter"""
    if merges is None:
        return []
    rows = np.asarray(merges).reshape(-1, 2).tolist() if np.asarray(merges).size else []
    return sorted({(min(int(a), int(b)), max(int(a), int(b))) for a, b in rows if int(a) != 0 and int(b) != 0 and int(a) != int(b)})


def graph_of(labels, connectivity=26, merges=None):
    """uint32 array of the labels' shape, Fortran ordered: the bit of a step is set iff the step is among the `connectivity`
    neighbours, the neighbour lies inside the array, and the two values are equal (0 == 0 included) or listed together in `merges`
    -- as they are listed: {a, b} and {b, c} say nothing about a and c"""
    lab0 = np.asarray(labels)
    lab = lab0.reshape(lab0.shape + (1,) * (3 - lab0.ndim))
    # every value by its rank among the volume's values; a listed pair of ranks (either order) as one number.  A pair that names a
    # value the volume does not hold joins nothing.
    values, rank = np.unique(lab, return_inverse=True)
    rank = rank.reshape(lab.shape).astype(np.int64)
    n = int(values.size)
    rank_of = {int(v): k for k, v in enumerate(values.tolist())}
    listed = np.array(sorted({rank_of[p] * n + rank_of[q] for p, q in pair_list(merges) if p in rank_of and q in rank_of}
                             | {rank_of[q] * n + rank_of[p] for p, q in pair_list(merges) if p in rank_of and q in rank_of}), dtype=np.int64)
    out = np.zeros(lab.shape, dtype=np.uint32, order="F")
    for bit, step in enumerate(CC3D_STEP_OF_BIT[:CONNECTIVITY_BITS[connectivity]]):
        here, there = _sides(step, lab.shape)
        joined = lab[here] == lab[there]
        if listed.size:
            joined = joined | np.isin(rank[here] * n + rank[there], listed)
        out[here] |= joined.astype(np.uint32) << np.uint32(bit)
    return out.reshape(lab0.shape, order="F")


def clip(box_graph):
    """the graph of a box cut out of a larger graph, as a copy with every bit cleared whose step leaves the box"""
    g0 = np.asarray(box_graph)
    g = np.array(g0.reshape(g0.shape + (1,) * (3 - g0.ndim)), dtype=np.uint32, order="F")
    keep = np.zeros(g.shape, dtype=np.uint32)
    for bit, step in enumerate(CC3D_STEP_OF_BIT):
        here, _ = _sides(step, g.shape)
        keep[here] |= np.uint32(1 << bit)
    return (g & keep).reshape(g0.shape, order="F")


def allowed_step(graph, u, v):
    """whether the graph allows the step from voxel u to voxel v (integer triples): they are 26-neighbours and the bit of v - u is
    set in u's word"""
    step = tuple(int(b) - int(a) for a, b in zip(u, v))
    if step not in CC3D_STEP_OF_BIT:
        return False
    return bool((int(graph[tuple(int(c) for c in u)]) >> CC3D_STEP_OF_BIT.index(step)) & 1)


def wall(graph, axis, at):
    """a copy of the graph with a wall between index `at` and `at + 1` along `axis`: every step across it is cleared, both ways"""
    g = np.array(graph, dtype=np.uint32, order="F")
    low, high = [slice(None)] * 3, [slice(None)] * 3
    low[axis], high[axis] = at, at + 1
    up = sum(1 << b for b, s in enumerate(CC3D_STEP_OF_BIT) if s[axis] > 0)
    down = sum(1 << b for b, s in enumerate(CC3D_STEP_OF_BIT) if s[axis] < 0)
    g[tuple(low)] &= np.uint32(~up & 0xFFFFFFFF)
    g[tuple(high)] &= np.uint32(~down & 0xFFFFFFFF)
    return g
