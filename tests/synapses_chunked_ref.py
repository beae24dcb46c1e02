"""The statement of one visit of kh_nearest_label_voxels_box in numpy, and the inputs the host and the GPU tier
of synapses_to_targets_chunked share.  The truth of the whole feature is tests/points_ref.py::synapses_to_targets of the whole
dataset; nothing of the product is imported here but its grid arithmetic (kimimaro_amd.plan, device-free)."""
import functools

import numpy as np

NONE64 = 0xFFFFFFFFFFFFFFFF
SHAPE = (37, 29, 23)
CHUNKS = ((16, 13, 11), (8, 8, 8), (5, 29, 7), (64, 64, 64))       # 27 cores, 60 cores, slabs, one chunk larger than the dataset
ABSENT = 4242                                                        # a label that occurs nowhere in dataset()
ORDERS = {"near_first": None, "raster": lambda bounds: np.arange(bounds.shape[0]),
          "reversed": lambda bounds: np.arange(bounds.shape[0])[::-1]}


@functools.lru_cache(maxsize=None)
def dataset():
    from shapes import voronoi_labels
    lab = voronoi_labels(SHAPE, 6, seed=21, pts_per_label=3, step=7.0)
    lab[0, 0, 0] = 7                     # a label of one voxel, in the first core of every grid
    lab.setflags(write=False)
    return lab


def distance_bits(voxels, centroid):
    """u64 [n]: the bits of sqrt((dx*dx + dy*dy) + dz*dz), d = (double)voxel - centroid, every operation rounded in float64"""
    v = np.asarray(voxels, dtype=np.int64).reshape(-1, 3).astype(np.float64)
    c = np.asarray(centroid, dtype=np.float64).reshape(3)
    dx, dy, dz = v[:, 0] - c[0], v[:, 1] - c[1], v[:, 2] - c[2]
    return np.sqrt((dx * dx + dy * dy) + dz * dz).view(np.uint64)


def c_index(voxel, shape):
    """the dataset's C-order index of a voxel, as a Python int"""
    x, y, z = (int(v) for v in voxel)
    return (x * int(shape[1]) + y) * int(shape[2]) + z


def visit(box, lo, shape, words, query_start, centroids, query_index, best_distance, best_voxel):
    """One visit: for every listed query q, row g = query_index[q] of the running arrays becomes the lexicographic minimum of the
    pair that came in and, over the box's voxels of the query's label, (bits of d, C-order index in the dataset).  box: host array
    [x, y, z] of any integer dtype or bool, its low corner at `lo` of a dataset of `shape`; words: the labels as the unsigned words
    the box holds.  The running arrays are u64 host arrays, changed in place; rows that are not listed are not touched."""
    box = np.asarray(box)
    held = box.view("u%d" % box.dtype.itemsize)
    lo = np.asarray(lo, dtype=np.int64).reshape(3)
    for k, word in enumerate(np.asarray(words, dtype=np.uint64).tolist()):
        cloud = np.argwhere(held == word) + lo             # rows (x, y, z) of the dataset, in its C order
        if cloud.shape[0] == 0:
            continue
        for q in range(int(query_start[k]), int(query_start[k + 1])):
            g = int(query_index[q])
            bits = distance_bits(cloud, centroids[q])
            first = int(np.argmin(bits))                    # the first of the nearest in C order
            found = (int(bits[first]), c_index(cloud[first], shape))
            best = min(found, (int(best_distance[g]), int(best_voxel[g])))
            best_distance[g], best_voxel[g] = np.uint64(best[0]), np.uint64(best[1])


def host_driver(data, synapses, chunk_shape, **kwargs):
    from kimimaro_amd import post
    return post.synapses_to_targets_chunked(data, synapses, chunk_shape, _visit=visit, **kwargs)


# ------------------------------------------------------------------------------------------------------------------ the synapses
def scattered(lab):
    """(a) centroids on the 1/8 grid all over the dataset and outside it, plus a label that occurs nowhere"""
    from test_points_host import dyadic_synapses
    synapses = dyadic_synapses(lab, 31)
    synapses[ABSENT] = [((3.0, 4.0, 5.0), 1), ((30.5, 20.0, 11.25), 0)]
    return synapses


def clustered(lab, labels=None, per_label=6, seed=5):
    """(b) centroids next to their label: a voxel of the label plus a jitter of up to 1.5 voxels on the 1/8 grid"""
    rng = np.random.default_rng(seed)
    synapses = {}
    for label in np.unique(lab).tolist():
        cloud = np.argwhere(lab == label)
        picks = cloud[rng.integers(0, cloud.shape[0], size=per_label)]
        jitter = rng.integers(-12, 13, size=(per_label, 3)) / 8.0
        pairs = [(tuple((p + j).tolist()), int(rng.integers(0, 3))) for p, j in zip(picks, jitter)]
        if labels is None or label in labels:
            synapses[label] = pairs
    return synapses


def cut_planes(shape, chunk_shape):
    """[(axis, cut)]: the planes between the cores of chunk_grid(shape, chunk_shape, overlap=0)"""
    return [(axis, cut) for axis in range(3) for cut in range(int(chunk_shape[axis]), int(shape[axis]), int(chunk_shape[axis]))]


def cut_ties(lab, chunk_shape, per_plane=3, seed=9):
    """(c) for every cut plane, centroids at cut - 0.5 on the cut axis and integers on the other two, placed where the voxels on
    both sides of the cut carry one label: those two voxels are equally near (0.5), nothing is nearer, and they lie in two cores"""
    rng = np.random.default_rng(seed)
    synapses = {}
    for axis, cut in cut_planes(lab.shape, chunk_shape):
        below, above = np.take(lab, cut - 1, axis=axis), np.take(lab, cut, axis=axis)
        spots = np.argwhere(below == above)
        assert spots.shape[0] >= per_plane
        for u, v in spots[rng.choice(spots.shape[0], size=per_plane, replace=False)].tolist():
            centroid = [float(u), float(v)]
            centroid.insert(axis, cut - 0.5)
            synapses.setdefault(int(below[u, v]), []).append((tuple(centroid), int(rng.integers(0, 3))))
    return synapses


def nearest_sets(lab, synapses):
    """per (label, centroid) of `synapses`: the voxels (rows x, y, z) of the label at the smallest computed distance"""
    out = []
    for label, pairs in synapses.items():
        cloud = np.argwhere(lab == label)
        for centroid, _ in pairs:
            bits = distance_bits(cloud, centroid)
            out.append(cloud[bits == bits.min()])
    return out
