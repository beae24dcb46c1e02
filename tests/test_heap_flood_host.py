"""The inputs of tests/test_gpu_heap_flood.py are in the regimes they are named for -- asserted on the oracle alone (the peak heap
size of its restatement of the reference's flood, ko_get_last_heap_peak), without a GPU.  The heap emulation replays the oracle's
pushes and pops one for one, so the oracle's peak is the peak of Heap<1> and Heap<2> as well."""
import numpy as np
import pytest

import flood_cases as FC


@pytest.mark.parametrize("radii", sorted(FC.RADII))
@pytest.mark.parametrize("row", sorted(FC.ALL_ROWS))
def test_flood_rows_are_in_their_regime(row, radii):
    c = FC.case(row, radii)
    print("%s/%s: oracle count %d, peak heap %d, window %s" % (row, radii, c.count, c.peak, c.window))
    assert FC.in_window(c), "the input left its regime: peak heap %d not in (%d, %d)" % ((c.peak,) + c.window)
    assert 0 < c.count == c.after.size - int(np.count_nonzero(c.after))


def test_flood_rows_cover_every_regime():
    """the three windows tile (0, 131 071) at Heap<2>'s two boundaries and each has a row without and, above TOP, with a graph"""
    assert FC.LDS_ONLY[1] == FC.STRADDLE[0] == 8191 and FC.STRADDLE[1] == FC.PARENTS_HBM[0] == 16383
    plain = {w for _, _, _, w in FC.ROWS.values()}
    assert {FC.STRADDLE, FC.PARENTS_HBM} <= plain and any(FC.LDS_ONLY[0] <= a and b == FC.LDS_ONLY[1] for a, b in plain)
    assert {w for _, _, _, w in FC.GRAPH_ROWS.values()} == {FC.STRADDLE, FC.PARENTS_HBM}
    assert max(int(np.prod(s)) for s, _, _, _ in FC.ALL_ROWS.values()) == 25600


def test_graph_lowers_the_peak():
    """the graph rows are floods of their own: sparser pushes, a smaller peak than the same block without the graph"""
    for radii in sorted(FC.RADII):
        for g, plain in (("straddle_graph", "straddle"), ("parents_hbm_graph", "parents_hbm")):
            assert FC.case(g, radii).peak < FC.case(plain, radii).peak
            assert FC.case(g, radii).shape == FC.case(plain, radii).shape


def test_path_volume_reaches_parents_in_memory():
    """scale = 0.5, const = 10 on the (40, 32, 20) block (flood_cases.PATH_SCALE: why not the defaults): the largest flood of the path
    loop peaks at 16 976 nodes, above 16 383, on the block's crop, so the big label's Heap<2> reads parents from memory inside
    trace_paths_kernel<false, 2> too; it leaves voxels behind, so later floods and paths depend on its mask"""
    pc = FC.path_case()
    shape, count, peak, pushes = max(pc.calls, key=lambda c: c[2])
    block = [c for c in pc.calls if c[0] == FC.BLOCK]
    print("floods: %d, on the block %d; the largest on %s: %d voxels, peak heap %d, %d pushes" % (len(pc.calls), len(block), shape, count,
                                                                                                peak, pushes))
    assert (FC.PATH_SCALE, FC.PATH_CONST) == (0.5, 10.0)
    assert shape == FC.BLOCK and FC.PARENTS_HBM[0] < peak < FC.PARENTS_HBM[1] and peak == 16976
    assert block[0][2] == peak and 0 < block[0][1] < int(np.prod(FC.BLOCK)) and len(block) >= 5
    assert sum(c[1] for c in block) == int(np.prod(FC.BLOCK))
    assert sorted(pc.want.keys()) == [1, 2]
    assert all(len(s.vertices) >= 2 for s in pc.want.values())
    assert any(c[0] != FC.BLOCK for c in pc.calls), "the bar has a flood of its own"
