"""The inputs of tests/test_gpu_heap_flood.py (kh_heap_flood: one call of the flood of csrc/heap.h on Heap<1> or Heap<2>, plain or
profiled) and of tests/test_heap_flood_host.py, which asserts on the oracle alone that every input is in the regime it is named for.

The regimes are those of the batched leaf append on Heap<2> (TOP = 8 191 slots in LDS): a new leaf goes to LDS below slot 8 191 and
to memory from there on, and the key of its parent comes from LDS below leaf 16 383 and from memory from there on.  A flood whose
heap peaks below 8 191 nodes never leaves LDS, one that peaks between 8 191 and 16 383 appends to memory under parents in LDS, one
that peaks above 16 383 also reads parents from memory.  (For Heap<1>, TOP = 127, all but the first row are in the last regime.)

Blocks, sources, DBF and the random graph are those of tests/test_gpu_heap_mirror.py: a solid block, three sources, DBF = r."""
import ctypes as C
import functools
from types import SimpleNamespace

import numpy as np

import test_gpu_heap_mirror as HM

RADII = HM.RADII
TOP2 = 8191                    # Heap<2>: slots in LDS
PARENTS_LDS = 2 * TOP2 + 1     # the first leaf whose parent is slot TOP2, the first in memory
ONE_TRIP = HM.ONE_TRIP
LDS_ONLY, STRADDLE, PARENTS_HBM = (0, TOP2), (TOP2, PARENTS_LDS), (PARENTS_LDS, ONE_TRIP)

# (block, anisotropy, r, (peak above, peak below)).  The first two windows are narrower than "below 8 191": the small row has to
# outgrow the 64 nodes below which the append goes push by push and stays below Heap<1>'s mirror end (the existing row of
# test_gpu_heap_mirror.py); the second has to reach the last level of the LDS part (slots 4 095 .. 8 190).
ROWS = {
    "small":         ((6, 6, 4), (1, 1, 1), 3, (HM.LDS_TOP, HM.MIRROR_END)),
    "under_top":     ((24, 20, 12), (1, 1, 1), 14, (TOP2 // 2, TOP2)),
    "straddle":      ((30, 24, 16), (1, 1, 1), 18, STRADDLE),
    "straddle_anis": ((32, 28, 16), (16, 16, 40), 320, STRADDLE),
    "parents_hbm":      ((40, 32, 20), (1, 1, 1), 30, PARENTS_HBM),
    "parents_hbm_anis": ((40, 32, 20), (16, 16, 40), 500, PARENTS_HBM),
}
# the two isotropic rows above TOP with the asymmetric random graph of test_heap_mirror_voxel_graph (seed 77, 5 % of the bits
# cleared): pushes are sparser, so the peak is the graph's own and the window is asserted for it again
GRAPH_ROWS = {
    "straddle_graph":    ((30, 24, 16), (1, 1, 1), 18, STRADDLE),
    "parents_hbm_graph": ((40, 32, 20), (1, 1, 1), 30, PARENTS_HBM),
}
ALL_ROWS = {**ROWS, **GRAPH_ROWS}
assert all(HM.ROWS[m][:3] == ROWS[f][:3] for m, f in (("mirror_only", "small"), ("under_8191", "under_top"), ("one_trip", "parents_hbm"),
                                                      ("one_trip_anis", "parents_hbm_anis")))


@functools.lru_cache(maxsize=None)
def graph_of(shape):
    g = HM.random_graph(shape)
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def case(row, radii):
    """One flood, computed once and shared (the arrays are read-only): shape, an, path (three voxels), dbf, graph (or None), window,
    and the oracle's answer on a mask of ones: count, mask after, peak heap size, pushes."""
    shape, an, r, window = ALL_ROWS[row]
    path, dbf = HM.block_inputs(shape, r, radii)
    graph = graph_of(shape) if row in GRAPH_ROWS else None
    import oracle
    cnt, after, peak = HM.oracle_call(shape, an, path, dbf, graph=graph)
    # the pushes the oracle made (its heap_ops), from a second run of the same call
    cnt2, _, pushes = oracle.roll_invalidation_ball_inside_component(np.ones(shape, np.uint8, order="F"), dbf, 1.0, 0.0, an, path,
                                                                     return_stats=True, voxel_connectivity_graph=graph)
    assert cnt2 == cnt
    for a in (dbf, after):
        a.setflags(write=False)
    return SimpleNamespace(row=row, radii=radii, shape=shape, an=an, path=path, dbf=dbf, graph=graph, window=window, count=cnt,
                           after=after, peak=peak, pushes=int(pushes))


def in_window(c):
    above, below = c.window
    return above < c.peak < below


# ---- the same heap inside the path kernel: one volume, two labels -------------------------------------------------------------
BLOCK = (40, 32, 20)         # the large label: the block of the parents_hbm rows
PATH_AN = (1, 1, 1)
# scale / const of the path loop.  With the defaults' scale = 1.5 and const = 15 (and anything near them) the first path's balls cover
# the whole block: one flood per label, peak 16 976, and whatever order the heap pops in, the mask ends empty.  With 0.5 / 10 the
# first flood has the same peak (16 976: the front is the block's cross-section) but leaves 2 183 of the 25 600 voxels, and the eight
# floods and paths after it depend on WHICH voxels those are (149 vertices instead of 40).
PATH_SCALE, PATH_CONST = 0.5, 10.0


def path_volume():
    """a solid BLOCK as label 1 and, two voxels beside it, a bar of 6 x 2 x 2 voxels as label 2"""
    lab = np.zeros((BLOCK[0] + 8, BLOCK[1], BLOCK[2]), dtype=np.uint32, order="F")
    lab[:BLOCK[0]] = 1
    lab[BLOCK[0] + 2:, 4:6, 4:6] = 2
    return lab


@functools.lru_cache(maxsize=None)
def path_case():
    """The oracle's skeletons of path_volume() with PATH_SCALE / PATH_CONST and, for every call of the flood the oracle made on the
    way, (shape of the crop it ran on, voxels it invalidated, peak heap size, pushes)."""
    import oracle
    from oracle import pipeline as P
    lib = oracle.lib()
    lib.ko_get_last_heap_peak.restype = C.c_int64
    params = dict(P.DEFAULT_TEASAR_PARAMS)
    params["scale"], params["const"] = PATH_SCALE, PATH_CONST
    calls = []
    flood = oracle.roll_invalidation_ball_inside_component

    def recorded(labels, *args, **kwargs):
        out = flood(labels, *args, **kwargs)
        assert kwargs.get("return_stats"), "the path loop asks for the flood's pushes"
        calls.append((tuple(labels.shape), int(out[0]), int(lib.ko_get_last_heap_peak()), int(out[2])))
        return out

    oracle.roll_invalidation_ball_inside_component = recorded
    try:
        want = P.skeletonize(path_volume(), params, anisotropy=PATH_AN, dust_threshold=0, fix_borders=False)
    finally:
        oracle.roll_invalidation_ball_inside_component = flood
    return SimpleNamespace(params=params, an=PATH_AN, want=want, calls=calls)
