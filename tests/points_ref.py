"""The two contracts of DESIGN.md 3.11, stated the textbook way on the CPU (numpy, scipy, plain Python; nothing of the product is
imported here):

  synapses_to_targets  per label the point cloud of its voxels in C order, scipy's cdist to the centroids of one swc label, argmin
                       per centroid, the distinct winners in ascending order, dict updates in that order.
  extract_edges        thirteen shifted-array comparisons, one per "later" offset of the 26-neighbourhood, np.unique over the pairs;
                       vertices = the voxels on a pair by ascending Fortran index, edges (a, b), a < b, sorted by a, then b.
"""
import itertools

import numpy as np
from scipy.spatial.distance import cdist


def synapses_to_targets(labels, synapses):
    """{ (x, y, z): swc_label } with tuples of ints, in insertion order"""
    labels = np.asarray(labels)
    while labels.ndim > 3:
        labels = labels[..., 0]
    targets = {}
    for label, pairs in synapses.items():
        cloud = np.argwhere(labels == label)                 # rows (x, y, z) in C order, whatever the memory layout
        if cloud.shape[0] == 0:
            continue
        by_swc = {}
        for centroid, swc_label in pairs:
            by_swc.setdefault(swc_label, []).append(centroid)
        for swc_label, centroids in by_swc.items():
            nearest = np.argmin(cdist(cloud, np.asarray(centroids, dtype=np.float64).reshape(-1, 3)), axis=0)
            for k in np.unique(nearest):
                targets[tuple(int(v) for v in cloud[k])] = swc_label
    return targets


# the offsets (dx, dy, dz) whose neighbour comes LATER in the Fortran raster x + sx*(y + sy*z): 13 of the 26
LATER_OFFSETS = [d for d in itertools.product((-1, 0, 1), repeat=3) if (d[2], d[1], d[0]) > (0, 0, 0)]
assert len(LATER_OFFSETS) == 13


def offsets_of(connectivity):
    """6: the three axis offsets; 18: also the six face diagonals; 26: also the four corners"""
    most = {6: 1, 18: 2, 26: 3}[connectivity]
    return [d for d in LATER_OFFSETS if sum(c != 0 for c in d) <= most]


def _halves(delta):
    """slices (voxel, its neighbour at +delta) along one axis"""
    if delta == 0:
        return slice(None), slice(None)
    return (slice(0, -1), slice(1, None)) if delta > 0 else (slice(1, None), slice(0, -1))


def edge_index_pairs(image, connectivity=26):
    """int64 (m, 2): the Fortran indices (lower, higher) of every neighbouring pair of foreground voxels, sorted, unique"""
    fg = np.asarray(image) != 0
    while fg.ndim < 3:
        fg = fg[..., np.newaxis]
    index = np.arange(fg.size, dtype=np.int64).reshape(fg.shape, order="F")
    found = [np.zeros((0, 2), dtype=np.int64)]
    for delta in offsets_of(connectivity):
        here, there = zip(*[_halves(c) for c in delta])
        both = fg[here] & fg[there]
        found.append(np.stack([index[here][both], index[there][both]], axis=1))
    return np.unique(np.concatenate(found), axis=0)


def extract_edges(image, connectivity=26):
    """(vertices uint32 (n, 3), edges uint32 (m, 2)) in the canonical order"""
    fg = np.asarray(image)
    shape = (tuple(fg.shape) + (1, 1, 1))[:3]
    pairs = edge_index_pairs(image, connectivity)
    on_edge = np.unique(pairs)
    vertices = np.stack([on_edge % shape[0], (on_edge // shape[0]) % shape[1], on_edge // (shape[0] * shape[1])], axis=1)
    edges = np.searchsorted(on_edge, pairs)
    return vertices.astype(np.uint32).reshape(-1, 3), edges.astype(np.uint32).reshape(-1, 2)


def coordinate_pairs(vertices, edges):
    """the numbering-free form of a result: int64 rows (x0, y0, z0, x1, y1, z1), the lexicographically smaller end first, rows
    sorted -- NOT made unique: a pair listed twice shows"""
    v = np.asarray(vertices, dtype=np.int64).reshape(-1, 3)
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    rows = np.array(sorted(min(tuple(v[a]) + tuple(v[b]), tuple(v[b]) + tuple(v[a])) for a, b in e), dtype=np.int64)
    return rows.reshape(-1, 6)
