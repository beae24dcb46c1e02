"""The inputs of the search-regime tests: small, deterministic, each built for one part of sssp (csrc/sssp.h).
tests/test_search_ref_host.py proves search_ref == oracle on every one of them without a GPU; tests/test_gpu_search_regimes.py
runs them on the device.  Masks and fields are built on demand (`case["mask"]()`); points are (x, y, z)."""
import numpy as np

from voxel_graphs import random_graph

THREADS = (64, 128, 256, 512, 1024)       # threads per label of kh_edf_batch: H = 4 * threads slots, NQ = 2 * threads entries
LADDER = ((8, 8, 6), (12, 12, 8), (16, 16, 12), (24, 20, 12), (32, 32, 24), (40, 32, 20))
ANISOTROPIES = ((1, 1, 1), (16, 16, 40))


def solid(shape):
    return lambda: np.ones(shape, dtype=np.uint8, order="F")


def centre(shape):
    return tuple(s // 2 for s in shape)


def point_of(loc, shape):
    return (loc % shape[0], (loc // shape[0]) % shape[1], loc // (shape[0] * shape[1]))


def corners_and_centre(shape):
    pts = [(x, y, z) for z in (0, shape[2] - 1) for y in (0, shape[1] - 1) for x in (0, shape[0] - 1)]
    return pts + [centre(shape)]


def two_blocks():
    m = np.ones((13, 8, 6), dtype=np.uint8, order="F")
    m[6, :, :] = 0                            # an empty plane: x > 6 cannot be reached from x < 6
    return m


def l_shape():
    """two arms of width 3 along x and y that meet at the origin corner: the straight line between the arms' ends leaves the object"""
    m = np.zeros((16, 16, 4), dtype=np.uint8, order="F")
    m[:, :3, :] = 1
    m[:3, :, :] = 1
    return m


def asymmetric_graph(shape, seed):
    return lambda: random_graph(shape, np.random.default_rng(seed), 0.08, False)


def edf(name, shape, sources, an, mask=None, graph=None, fsr=0.0, threads=THREADS, expect=None):
    """expect: {counter: least value} every device run must report before its result counts (the regime the case is built for);
    runs / expect_once: the case is run that many times and the counter must reach the value in at least one of the runs"""
    return dict(name=name, shape=shape, sources=list(sources), an=an, mask=mask or solid(shape), graph=graph, fsr=fsr,
                threads=tuple(threads), expect=expect or {}, runs=1, expect_once={})


# ---- a. volume edges and the rows27 loads -------------------------------------------------------------------------------
TINY = [edf("tiny_%dx%dx%d" % s, s, [(0, 0, 0), tuple(v - 1 for v in s)], (2, 3, 5))
        for s in [(1, 1, 1), (2, 1, 1), (1, 2, 1), (1, 1, 2), (3, 1, 1), (2, 2, 1), (2, 2, 2), (4, 1, 1), (1, 1, 5)]]
# x steps forty times dearer than the others (and the other way round): a word taken from the wrapped row would lower a distance
EDGES = [edf("edge_%dx%dx%d_an%d_%d_%d" % (s + an), s, corners_and_centre(s), an)
         for s in [(2, 9, 7), (3, 5, 4), (2, 2, 40)] for an in [(40, 1, 1), (1, 40, 1), (1, 1, 1)]]
# frontier of one voxel, a far-list split per threshold raise: about 150 raises of two voxel steps each (delta floor = 2 * 16)
STICKS = [edf("stick_%dx%dx%d" % s, s, [(0, 0, 0)], (16, 16, 40), expect={"stat_search_splits": 50})
          for s in [(300, 1, 1), (1, 300, 1), (1, 1, 300)]]

# ---- b. near-list spill and combine-table retry.  Row = (threads, anisotropy) -> the ladder block ONE STEP ABOVE the smallest block
# at which the counter was seen nonzero on an MI355X (source at the centre).  The values seen at each row stand beside it.
#
# Spills are (almost) the same number in every run.  Retries are not: with more than one wave the order of the work lists depends
# on wave timing, a batch fills the table to about three quarters, and whether some offer then finds twelve occupied slots in a row
# is a matter of that order -- the counts are small random numbers (means 1.3 to 7 at the rows below) and zero in up to two of
# twenty runs.  A retry row above 64 threads is therefore run RETRY_RUNS times, every run's result is compared, and the counter
# must be nonzero in at least one of them (worst row: 0.1 ** 5 = 1e-5 that all five are zero); where the block one step above the
# smallest was zero more often than that, the row moved up to a block that, like the one under it, was nonzero in every run seen.
# At 64 threads (one wave, nothing to race) every run must show the retry.
ISO, ANISO = ANISOTROPIES
RETRY_RUNS = 5
SPILL_ROWS = {                   # twenty runs each
    (64, ISO): (12, 12, 8),      # 3 in every run            (smallest: (8, 8, 6), 1)
    (64, ANISO): (12, 12, 8),    # 4 in every run            (smallest: (8, 8, 6), 2)
    (128, ISO): (16, 16, 12),    # 4 in every run            (smallest: (12, 12, 8), 2)
    (128, ANISO): (16, 16, 12),  # 5 in every run            (smallest: (12, 12, 8), 1 - 2)
    (256, ISO): (24, 20, 12),    # 5 in every run            (smallest: (16, 16, 12), 3)
    (256, ANISO): (24, 20, 12),  # 5, once 6                 (smallest: (16, 16, 12), 2)
    (512, ISO): (32, 32, 24),    # 9 in every run            (smallest: (24, 20, 12), 1)
    (512, ANISO): (32, 32, 24),  # 10 - 12                   (smallest: (24, 20, 12), 1)
    (1024, ISO): (40, 32, 20),   # 4 - 7                     (smallest: (32, 32, 24), 6)
    (1024, ANISO): (40, 32, 20), # 5 in every run            (smallest: (32, 32, 24), 5 - 6)
}
RETRY_ROWS = {
    (64, ISO): (16, 16, 12),     # 2 in each of twenty runs  (smallest: (12, 12, 8), 4)
    (64, ANISO): (16, 16, 12),   # 1 in each of twenty runs  (smallest: (12, 12, 8), 3)
    (128, ISO): (32, 32, 24),    # 7 7 6                     ((12, 12, 8): 2 2 2, (16, 16, 12): zero in 4 of 20 runs, (24, 20, 12): 3 2 2)
    (128, ANISO): (32, 32, 24),  # 1 - 6 in twenty runs      ((12, 12, 8): 1 1 1, (16, 16, 12): 0 0 0, (24, 20, 12): 2 1 1)
    (256, ISO): (40, 32, 20),    # 1 - 4 in twenty runs, 0 once in five later ones   (smallest: (32, 32, 24), 2 4 2)
    (256, ANISO): (40, 32, 20),  # 0 - 7, zero once in 20    (smallest: (32, 32, 24), 0 3 0)
    (512, ISO): (40, 32, 20),    # 0 - 2, zero twice in 20   (smallest: (32, 32, 24), 1 5 1)
    (512, ANISO): (40, 32, 20),  # 1 - 4 in twenty runs      ((24, 20, 12): 1 1 1, (32, 32, 24): 0 1 0)
    # 1024 threads (H = 4096): 0 0 1 on (32, 32, 24) and 0 0 0 on (40, 32, 20) isotropic, 1 1 1 and 1 1 0 anisotropic -- the
    # largest block of the ladder does not fill that table: no row
}


def ladder_cases():
    out = []
    for (thr, an), s in sorted(SPILL_ROWS.items()):
        out.append(edf("spills_t%d_%dx%dx%d_an%d" % ((thr,) + s + (an[2],)), s, [centre(s)], an, threads=(thr,),
                       expect={"stat_search_spills": 1}))
    for (thr, an), s in sorted(RETRY_ROWS.items()):
        case = edf("retries_t%d_%dx%dx%d_an%d" % ((thr,) + s + (an[2],)), s, [centre(s)], an, threads=(thr,))
        if thr == 64:
            case["expect"] = {"stat_search_retries": 1}
        else:
            case.update(runs=RETRY_RUNS, expect_once={"stat_search_retries": 1})
        out.append(case)
    # the retry rows' blocks with a random asymmetric voxel graph, 8 % of the direction bits cleared (spills: 8 and 11 in every run)
    for thr in (64, 512):
        s = RETRY_ROWS[(thr, ANISO)]
        out.append(edf("graph_t%d_%dx%dx%d" % ((thr,) + s), s, [centre(s)], ANISO, graph=asymmetric_graph(s, 800 + thr),
                       threads=(thr,), expect={"stat_search_spills": 1}))
    return out


LADDER_CASES = ladder_cases()

# ---- c. ties, unreachable voxels, seeds ------------------------------------------------------------------------------------
TIES = [edf("tie_9x9x9", (9, 9, 9), [(4, 4, 4)], (1, 1, 1)),          # eight corners tie for farthest: index 0
        edf("tie_9x9x1", (9, 9, 1), [(4, 4, 0)], (1, 1, 1)),
        edf("two_blocks", (13, 8, 6), [(2, 3, 3), (12, 7, 5)], (1, 1, 1), mask=two_blocks)]
SEEDS = [edf("fsr%g_%s" % (r, nm), s, [src], (1, 1, 1), mask=mk, fsr=r)
         for nm, s, mk, src in [("block", (16, 16, 12), None, (8, 8, 6)), ("lshape", (16, 16, 4), l_shape, (15, 1, 2))]
         for r in (0.5, 3.0, 1000.0)]

EDF_CASES = TINY + EDGES + STICKS + LADDER_CASES + TIES + SEEDS
EDF_BY_NAME = {c["name"]: c for c in EDF_CASES}
assert len(EDF_BY_NAME) == len(EDF_CASES)


# ---- d. weighted searches (256 threads, delta floor 0) ----------------------------------------------------------------------
def flat_field():
    return np.ones((12, 12, 8), dtype=np.float32, order="F")


def wide_field(seed):
    def make():
        rng = np.random.default_rng(seed)
        return np.asfortranarray((10.0 ** rng.uniform(-3, 5, (16, 16, 12))).astype(np.float32))
    return make


def random_field():
    rng = np.random.default_rng(2412)
    return np.asfortranarray(rng.uniform(1.0, 9.0, (24, 20, 12)).astype(np.float32))


# name -> (field builder, source).  Every field is finite everywhere: the object is the whole block.
FIELD_CASES = {
    "flat": (flat_field, (6, 6, 4)),
    "wide_1": (wide_field(31), (8, 8, 6)),
    "wide_2": (wide_field(32), (0, 0, 0)),
    "wide_3": (wide_field(33), (15, 15, 11)),
    "random_24x20x12": (random_field, (12, 10, 6)),
}


def rail_adjacent():
    f = np.full((10, 8, 6), 3.0, dtype=np.float32, order="F")
    f[5, 4, 3] = 0.0
    return f


def rail_is_source():
    f = np.full((10, 8, 6), 3.0, dtype=np.float32, order="F")
    f[4, 4, 3] = 0.0
    f[9, 7, 5] = 0.0
    return f


def rail_equal_cost():
    f = np.full((11, 9, 5), 2.0, dtype=np.float32, order="F")
    f[1, 4, 2] = 0.0              # four steps to either side of the source: the same sum, the smaller index wins
    f[9, 4, 2] = 0.0
    return f


def rail_decoy():
    """a corridor along x (everything else is outside the object): on one side of the source three voxels of weight 4.0 and then
    rail A (12.0), on the other forty voxels of weight 0.25 and then rail B (10.0).  The search meets A first and must return B."""
    f = np.full((50, 3, 3), np.inf, dtype=np.float32, order="F")
    f[44, 1, 1] = 1.0             # the source
    f[45:48, 1, 1] = 4.0
    f[48, 1, 1] = 0.0             # A
    f[4:44, 1, 1] = 0.25
    f[3, 1, 1] = 0.0              # B
    return f


def rail_none():
    return np.full((8, 6, 4), 2.0, dtype=np.float32, order="F")


# name -> (field builder, source, the rail the path must end at or None when the call must fail)
RAIL_CASES = {
    "adjacent": (rail_adjacent, (4, 4, 3), (5, 4, 3)),
    "source_is_rail": (rail_is_source, (4, 4, 3), (4, 4, 3)),
    "equal_cost": (rail_equal_cost, (5, 4, 2), (1, 4, 2)),
    "decoy": (rail_decoy, (44, 1, 1), (3, 1, 1)),
    "no_rail": (rail_none, (3, 3, 2), None),
}

# reuse of one search object: railroad from a, from b, from a again (the block is larger than NQ = 512 at 256 threads, so the
# list of touched voxels runs past the LDS part of the near lists)
def reuse_field():
    rng = np.random.default_rng(99)
    f = np.asfortranarray(rng.uniform(1.0, 9.0, (24, 20, 12)).astype(np.float32))
    f[0, 0, 0] = 0.0              # the only rail, far from both sources: thousands of voxels are settled before it
    return f


REUSE = (reuse_field, (12, 10, 6), (20, 17, 9))
