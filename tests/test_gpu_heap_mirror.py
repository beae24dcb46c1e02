"""The heap emulation's key mirror (csrc/heap.h: heap levels 7-10 as LDS keys, one global round trip per pop for heaps
below 131 072 nodes) against the oracle's restatement of the reference's heap, at every heap size at which a pop takes
another way down: the LDS part alone (< 127 nodes), the mirror stage alone (< 2 047), one global chunk under a mirrored hole
(what used to be one chunk below 8 191 nodes and two above it).  sweep = False: every call is the heap emulation.

Inputs are solid blocks with three sources and a constant DBF = r (scale 1, const 0).  Each case first asserts, from the
oracle's own peak heap size, that it is in the regime it is meant for."""
import ctypes as C

import numpy as np
import pytest

from shapes import voronoi_labels

pytestmark = pytest.mark.gpu

LDS_TOP = 127            # heap slots in LDS as whole nodes
MIRROR_END = 2047        # ... and as keys (levels 7-10)
OLD_CHUNK = 8191         # below: one global chunk before the mirror, above: two
ONE_TRIP = 131071        # above: a second global chunk under the mirror (not reachable in a test of seconds)

# (block, anisotropy, r, (peak above, peak below))
ROWS = {
    "mirror_only":      ((6, 6, 4), (1, 1, 1), 3, (LDS_TOP, MIRROR_END)),
    "first_chunk":      ((12, 12, 8), (1, 1, 1), 6, (MIRROR_END, OLD_CHUNK)),
    "first_chunk_anis": ((12, 12, 8), (16, 16, 40), 150, (MIRROR_END, OLD_CHUNK)),
    "under_8191":       ((24, 20, 12), (1, 1, 1), 14, (OLD_CHUNK // 2, OLD_CHUNK)),
    "one_trip":         ((40, 32, 20), (1, 1, 1), 30, (2 * OLD_CHUNK + 1, ONE_TRIP)),
    "one_trip_anis":    ((40, 32, 20), (16, 16, 40), 500, (2 * OLD_CHUNK + 1, ONE_TRIP)),
}
# per-source factors of the radius: equal balls, and balls that differ so that the owner of a tied voxel decides its fate
RADII = {"equal": (1.0, 1.0, 1.0), "differ": (1.0, 0.85, 0.7)}


def sources(shape):
    sx, sy, sz = shape
    return [(sx // 4, sy // 4, sz // 4), (sx // 2, sy // 2, sz // 2), (3 * sx // 4, 3 * sy // 4, 3 * sz // 4)]


def block_inputs(shape, r, radii):
    """(sources, DBF) of a solid block: DBF = r everywhere, r times its factor at the three sources"""
    path = sources(shape)
    dbf = np.full(shape, r, np.float32, order="F")
    for (x, y, z), f in zip(path, RADII[radii]):
        dbf[x, y, z] = np.float32(r * f)
    return path, dbf


def block_case(row, radii):
    shape, an, r, regime = ROWS[row]
    path, dbf = block_inputs(shape, r, radii)
    return shape, an, path, dbf, regime


def random_graph(shape, seed=77, cleared=0.05):
    """a connectivity graph with every bit cleared independently (so asymmetrically: the reference reads only the word of the voxel
    it expands)"""
    rng = np.random.default_rng(seed)
    vcg = np.full(shape, (1 << 26) - 1, dtype=np.uint32, order="F")
    for b in range(26):
        vcg &= ~(np.asfortranarray(rng.random(shape) < cleared).astype(np.uint32) << np.uint32(b))
    return vcg


def oracle_call(shape, an, path, dbf, graph=None):
    """(count, mask after, peak heap size) of the oracle"""
    import oracle
    lib = oracle.lib()
    lib.ko_get_last_heap_peak.restype = C.c_int64
    m = np.ones(shape, np.uint8, order="F")
    cnt, _ = oracle.roll_invalidation_ball_inside_component(m, dbf, 1.0, 0.0, an, path, voxel_connectivity_graph=graph)
    return cnt, m, int(lib.ko_get_last_heap_peak())


@pytest.fixture(scope="module")
def heap_ops():
    """ops.* on an engine without the sweep: every invalidation is the heap emulation"""
    from kimimaro_amd import ops
    from kimimaro_amd.engine import Engine
    eng2 = Engine()
    eng2.sweep = False
    ops._engine = eng2
    try:
        yield ops
    finally:
        ops._engine = None


@pytest.mark.parametrize("radii", sorted(RADII))
@pytest.mark.parametrize("row", sorted(ROWS))
def test_heap_mirror_blocks(heap_ops, row, radii):
    shape, an, path, dbf, (above, below) = block_case(row, radii)
    want_cnt, want, peak = oracle_call(shape, an, path, dbf)
    print("%s/%s: oracle count %d, peak heap %d" % (row, radii, want_cnt, peak))
    assert above < peak < below, "the input left its regime: peak heap %d not in (%d, %d)" % (peak, above, below)
    m = np.ones(shape, np.uint8, order="F")
    cnt, out = heap_ops.roll_invalidation_ball_inside_component(m, dbf, 1.0, 0.0, an, path)
    assert cnt == want_cnt
    np.testing.assert_array_equal(out, want)


@pytest.mark.parametrize("radii", sorted(RADII))
def test_heap_mirror_voxel_graph(heap_ops, radii):
    """the (12, 12, 8) block with a random connectivity graph (bits cleared asymmetrically: the reference reads only the
    word of the voxel it expands): pushes are sparser, the heap still outgrows the mirror"""
    shape, an, path, dbf, _ = block_case("first_chunk", radii)
    vcg = random_graph(shape)
    want_cnt, want, peak = oracle_call(shape, an, path, dbf, graph=vcg)
    print("graph/%s: oracle count %d, peak heap %d" % (radii, want_cnt, peak))
    assert MIRROR_END < peak < OLD_CHUNK, "the input left its regime: peak heap %d" % peak
    m = np.ones(shape, np.uint8, order="F")
    cnt, out = heap_ops.roll_invalidation_ball_inside_component(m, dbf, 1.0, 0.0, an, path, voxel_connectivity_graph=vcg)
    assert cnt == want_cnt
    np.testing.assert_array_equal(out, want)


def test_heap_mirror_path_loop_lane_configuration():
    """the path loop as the lanes launch it -- one wave per label, a level window of 2 048 words, heap scratch from the pool --
    with the sweep off, on a volume whose heaps outgrow LDS part and mirror: the oracle's skeletons"""
    import kimimaro_amd
    from kimimaro_amd.engine import Engine
    from oracle import pipeline as P
    eng2 = Engine()
    eng2.trace_threads = 64
    eng2.window_cap = 2048
    eng2.window_cap_always = True
    eng2.sweep = False
    eng2.scratch_pool = True
    an = (16, 16, 40)
    lab = voronoi_labels((96, 96, 40), 7, seed=5, pts_per_label=3, step=12.0, anisotropy=an)
    params = dict(kimimaro_amd.DEFAULT_TEASAR_PARAMS)
    got = kimimaro_amd.skeletonize(lab, params, anisotropy=an, dust_threshold=100, fix_borders=True,
                                   progress=False, _engine=eng2)
    want = P.skeletonize(lab, params, anisotropy=an, dust_threshold=100, fix_borders=True)
    tk = eng2.last_tasks
    assert int(tk["stat_sweep_calls"].sum()) == 0
    assert int(tk["stat_heap_pushes"].max()) > 20000
    assert sorted(got.keys()) == sorted(want.keys()) and len(got) >= 4
    for k in got:
        np.testing.assert_array_equal(got[k].vertices, want[k].vertices)
        np.testing.assert_array_equal(got[k].edges, want[k].edges)
        np.testing.assert_allclose(got[k].radii, want[k].radii, rtol=1e-4)
