"""Inputs of the component-bookkeeping tests (which component a target, a label and a skeleton id belong to), shared by the GPU tier
(test_gpu_component_bookkeeping.py) and the oracle-only tier (test_kat_oracle.py)."""
import numpy as np

AVOCADO_AN = (4, 4, 4)
# target -> the skeleton it must become a vertex of: two pits (labels 12 and 22, merged into their fruits 11 and 21 by the avocado
# pass), the plain blob 41, and a corner voxel of the 3 x 3 section of the thin process 51 (its centre line is y = 59, z = 41)
AVOCADO_TARGETS = {(21, 20, 22): 11, (2, 48, 24): 21, (50, 10, 6): 41, (47, 58, 40): 51}
AVOCADO_KEYS = [11, 21, 31, 41, 51]


def avocado_params(defaults):
    """the parameters of test_fix_avocados_matches_oracle"""
    params = dict(defaults)
    params.update(scale=1.5, const=20, soma_detection_threshold=10.0, soma_acceptance_threshold=1e9)
    return params


def vertex_set(skel):
    return set(map(tuple, np.asarray(skel.vertices).tolist()))


def holders(skels, pt, an):
    """the keys of the skeletons that have voxel `pt` (times the anisotropy) as a vertex"""
    phys = tuple(float(np.float32(p) * np.float32(a)) for p, a in zip(pt, an))
    return sorted(k for k, s in skels.items() if phys in vertex_set(s))


def island_volume():
    """label 5 with a closed cavity, label 6 an island inside the cavity: fill_holes swallows the island.  The target lies on 6."""
    lab = np.zeros((30, 26, 22), dtype=np.uint32, order="F")
    lab[3:27, 3:23, 3:19] = 5
    lab[8:22, 8:18, 7:15] = 0
    lab[11:19, 11:15, 9:13] = 6
    return lab, (12, 12, 10)


def spanning_block(wall):
    """a block of label 7 whose last row in the raster (y = 7, z = 6) begins with a run of label 9, and a graph that joins every
    pair of neighbours whatever their labels: ONE component whose first voxel says 7, whose last voxel says 7 and whose last run
    start says 9.  wall: the graph is cut between x = 11 and x = 12 -- two components, the 9-run in the first only."""
    from test_gpu_graph import cut_plane
    lab = np.zeros((24, 10, 8), dtype=np.uint32, order="F")
    lab[2:22, 2:8, 1:7] = 7
    lab[2:12, 7, 6] = 9
    g = np.full(lab.shape, 0x3FFFFFF, dtype=np.uint32, order="F")
    if wall:
        g = cut_plane(g, 0, 11)
    return lab, g


def graph_params(an):
    """the parameters of test_skeletonize_with_voxel_graph_matches_oracle"""
    return dict(scale=3.0, const=2.0 * an[0], pdrf_scale=5000, pdrf_exponent=4, soma_detection_threshold=1e9,
                soma_acceptance_threshold=1e9, soma_invalidation_scale=1.0, soma_invalidation_const=0.0)
