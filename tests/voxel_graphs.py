"""Voxel connectivity graphs of cc3d's layout for the tests: the direction-to-bit table and random graphs with some bits cleared."""
import numpy as np

# the 26 directions in the order of dijkstra_invalidation.hpp:60-124 and the bit of each in cc3d's layout (:152-190)
DIRS = [(-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1), (-1, -1, 0), (-1, 1, 0), (1, -1, 0), (1, 1, 0),
        (0, -1, -1), (0, -1, 1), (0, 1, -1), (0, 1, 1), (-1, 0, -1), (-1, 0, 1), (1, 0, -1), (1, 0, 1),
        (-1, -1, -1), (1, -1, -1), (-1, 1, -1), (-1, -1, 1), (1, 1, -1), (1, -1, 1), (-1, 1, 1), (1, 1, 1)]
GRAPH_BIT = [1, 0, 3, 2, 5, 4, 9, 7, 8, 6, 17, 13, 16, 12, 15, 11, 14, 10, 25, 24, 23, 21, 22, 20, 19, 18]


def random_graph(shape, rng, drop, symmetric):
    """a voxel_graph of cc3d's layout with a fraction of the direction bits cleared; symmetric: an edge is cleared both ways"""
    full = (1 << 26) - 1
    g = np.full(shape, full, dtype=np.uint32, order="F")
    for i in range(26):
        cut = np.asfortranarray(rng.random(shape) < drop)
        g[cut] &= np.uint32(~(1 << GRAPH_BIT[i]) & 0xFFFFFFFF)
        if symmetric:
            # the neighbour in direction i loses the opposite bit
            dx, dy, dz = DIRS[i]
            j = DIRS.index((-dx, -dy, -dz))
            src = np.argwhere(cut)
            dst = src + np.array([dx, dy, dz])
            ok = np.all((dst >= 0) & (dst < np.array(shape)), axis=1)
            dst = dst[ok]
            g[dst[:, 0], dst[:, 1], dst[:, 2]] &= np.uint32(~(1 << GRAPH_BIT[j]) & 0xFFFFFFFF)
    return g
