"""tests/search_ref.py (numpy Bellman fixpoint) against the oracle (heap Dijkstra in C) on every input of tests/search_cases.py,
word for word and without a GPU: the oracle gains a second witness, and the inputs of tests/test_gpu_search_regimes.py are proven
before a device sees them."""
import numpy as np
import pytest

import search_cases as SC
import search_ref as R


@pytest.mark.parametrize("name", [c["name"] for c in SC.EDF_CASES])
def test_edf_fixpoint_equals_oracle(name):
    import oracle
    case = SC.EDF_BY_NAME[name]
    mask = case["mask"]()
    graph = case["graph"]() if case["graph"] else None
    assert mask.shape == case["shape"]
    for src in case["sources"]:
        assert mask[src], "the source lies outside the mask"
        with oracle.voxel_graph(graph):
            want, wloc = oracle.euclidean_distance_field(mask, src, case["an"], free_space_radius=case["fsr"])
        got = R.edf_fixpoint(mask, src, case["an"], graph=graph, free_space_radius=case["fsr"])
        np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
        loc, val = R.farthest(got)
        assert R.point(loc, mask.shape) == tuple(wloc)
        assert val == want[tuple(wloc)]


def test_edf_case_properties():
    """what the cases claim about themselves"""
    d = R.edf_fixpoint(SC.EDF_BY_NAME["tie_9x9x9"]["mask"](), (4, 4, 4), (1, 1, 1))
    corners = [d[x, y, z] for x in (0, 8) for y in (0, 8) for z in (0, 8)]
    assert len(set(corners)) == 1 and corners[0] == d.max() and R.farthest(d)[0] == 0
    d = R.edf_fixpoint(SC.EDF_BY_NAME["tie_9x9x1"]["mask"](), (4, 4, 0), (1, 1, 1))
    assert d[0, 0, 0] == d[8, 0, 0] == d[0, 8, 0] == d[8, 8, 0] == d.max() and R.farthest(d)[0] == 0
    m = SC.two_blocks()
    d = R.edf_fixpoint(m, (2, 3, 3), (1, 1, 1))
    assert np.all(d[7:].view(np.uint32) == 0x7F800000) and np.all(np.isfinite(d[:6])) and R.farthest(d)[0] < m.size
    assert R.point(R.farthest(d)[0], m.shape)[0] < 6
    # the L shape: the straight line from the source to the far arm's end is shorter than any way inside the object
    m = SC.l_shape()
    src = (15, 1, 2)
    d = R.edf_fixpoint(m, src, (1, 1, 1))
    assert d[1, 15, 2] > np.float32(np.hypot(14, 14)) + 2
    seeded = R.edf_fixpoint(m, src, (1, 1, 1), free_space_radius=1000.0)
    assert seeded[1, 15, 2] == np.float32(np.sqrt(np.float32(14 * 14 + 14 * 14)))
    # free_space_radius = 0.5 seeds nothing, 3 seeds a ball, 1000 every voxel
    assert np.array_equal(R.edf_fixpoint(m, src, (1, 1, 1), free_space_radius=0.5), d)
    assert not np.array_equal(R.edf_fixpoint(m, src, (1, 1, 1), free_space_radius=3.0), d)


@pytest.mark.parametrize("name", sorted(SC.FIELD_CASES))
def test_field_fixpoint_equals_oracle(name):
    import oracle
    make, src = SC.FIELD_CASES[name]
    field = make()
    want = oracle.field_distances(field, src)
    got = R.field_fixpoint(field, src)
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("name", sorted(SC.RAIL_CASES))
def test_railroad_ends_at_the_fixpoint_rail(name):
    import oracle
    make, src, rail = SC.RAIL_CASES[name]
    field = make()
    d = R.field_fixpoint(field, src, rails_absorb=True)
    best = R.nearest_rail(field, d, src)
    if rail is None:
        assert best is None
        with pytest.raises(oracle.OracleError):
            oracle.railroad(field, src)
        return
    path = oracle.railroad(field, src)
    assert tuple(path[0]) == rail and tuple(path[-1]) == src
    if field[src] == 0:
        assert len(path) == 1                        # the source is a rail itself: no search
        return
    assert R.point(best[0], field.shape) == rail
    # the path's own cost (the weights of the voxels entered, summed from the source in float32) is the fixpoint's distance
    cost = np.float32(0)
    for p in path[::-1][1:]:
        cost = np.float32(cost + field[tuple(p)])
    assert cost == best[1]
    if name == "equal_cost":
        other = d[9, 4, 2]
        assert other == best[1] and R.lin((9, 4, 2), field.shape) > best[0]
    if name == "decoy":
        assert best[1] == np.float32(10.0) and d[48, 1, 1] == np.float32(12.0)


def test_reuse_inputs():
    import oracle
    make, a, b = SC.REUSE
    field = make()
    for src in (a, b):
        d = R.field_fixpoint(field, src, rails_absorb=True)
        best = R.nearest_rail(field, d, src)
        assert tuple(oracle.railroad(field, src)[0]) == R.point(best[0], field.shape)
