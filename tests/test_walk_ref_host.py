"""tests/walk_ref.py (the predecessor walk of csrc/backtrack.h restated from its header comment) against the oracle's ko_walk on
every input of tests/walk_cases.py, without a GPU: the oracle gains a witness that does not share its design, the distances the GPU
tests upload are proven, and every case shows -- on the reference alone -- that it is in the regime it is built for."""
import numpy as np
import pytest

import search_ref as R
import walk_cases as WC
import walk_ref as W

NAMES = [c["name"] for c in WC.ALL_CASES]


@pytest.mark.parametrize("name", NAMES)
def test_distances_equal_the_oracle(name):
    """the fixpoint the walks run on is the oracle's heap Dijkstra bit for bit (a railroad's search stops early: its distances are
    compared where the oracle settled them, through the rail it ends at and the path's own cost)"""
    import oracle
    case = WC.BY_NAME[name]
    for s in WC.solved(name):
        assert np.isfinite(s.field[s.source]) and s.dist[s.source] == 0
        if not case["rail"]:
            with oracle.voxel_graph(s.graph):
                want = oracle.field_distances(s.field, s.source)
            np.testing.assert_array_equal(s.dist.view(np.uint32), want.view(np.uint32))
            continue
        best = R.nearest_rail(s.field, s.dist, s.source)
        assert R.point(best[0], s.field.shape) == s.start
        cost = np.float32(0)
        for p in s.path[::-1][1:]:
            cost = np.float32(cost + s.field[p])
        assert cost == best[1]


@pytest.mark.parametrize("name", NAMES)
def test_walk_equals_the_oracle(name):
    import oracle
    case = WC.BY_NAME[name]
    for s in WC.solved(name):
        with oracle.voxel_graph(s.graph):
            if case["rail"]:
                want = oracle.railroad(s.field, s.source)                                   # rail end first, like the walk
            else:
                want = oracle.path_to_source(s.field, s.dist, s.source, s.start)[::-1]      # (source first: turned round)
        assert s.path[0] == s.start and s.path[-1] == s.stop
        np.testing.assert_array_equal(np.asarray(s.path), want)
        W.check_path(s.field, s.dist, s.path, s.graph, rails=case["rail"], stop=s.stop)


@pytest.mark.parametrize("name", NAMES)
def test_case_is_in_its_regime(name):
    """asserted on the reference alone: what the case is for happens in every one of its walks"""
    case = WC.BY_NAME[name]
    for s in WC.solved(name):
        st = s.stats
        print(name, s.source, "->", s.start, "path", len(s.path), st)
        if case["plateau"]:
            assert st["plateaus"] >= 1
        if case["wide"]:
            assert st["maxq"] > 64, "one pass of the 64-lane clean-up loop covers the queue"
            assert st["maxroute"] >= 2
        if case["plateaus"] is not None:
            assert st["plateaus"] == case["plateaus"]
    if name == "zero_source":
        # the plateau holds the source: no voxel at distance 0 has anything below it, and both targets reach it
        s = WC.solved(name)[0]
        assert int((s.dist == 0).sum()) == 32 and all(s.dist[t.path[-2]] == 0 for t in WC.solved(name))
    if name.startswith("rail_absorb"):
        s = WC.solved(name)[0]
        assert s.dist[s.path[1]] == s.dist[s.start], "the rail end does not start inside the plateau"


def test_check_path_rejects_wrong_paths():
    """the property check is no rubber stamp: a skipped voxel, a step against a one-way edge, a path that stops short"""
    s = WC.solved("absorb_graph_one_way")[0]
    W.check_path(s.field, s.dist, s.path, s.graph, stop=s.stop)
    with pytest.raises(AssertionError):
        W.check_path(s.field, s.dist, s.path[:3] + s.path[4:], s.graph, stop=s.stop)
    with pytest.raises(AssertionError):
        W.check_path(s.field, s.dist, s.path[:-1], s.graph, stop=s.stop)
    # a graph that forbids the second step of the path (the bit of the direction p2 -> p1 in p2's word)
    p1, p2 = s.path[1], s.path[2]
    k = W.DIRS.index(tuple(a - b for a, b in zip(p1, p2)))
    g = s.graph.copy()
    g[p2] &= np.uint32(~(1 << W.GRAPH_BIT[k]) & 0xFFFFFFFF)
    with pytest.raises(AssertionError):
        W.check_path(s.field, s.dist, s.path, g, stop=s.stop)
    z = WC.solved("zero_source")[1]
    with pytest.raises(AssertionError):
        W.check_path(z.field, z.dist, z.path[:-1], None, stop=z.stop)      # ends at distance 0, but not at the source


def test_walk_reports_a_dry_queue_and_a_missing_rail():
    f = np.ones((4, 4, 2), dtype=np.float32, order="F")
    d = R.field_fixpoint(f, (0, 0, 0))
    broken = d.copy()
    broken[1:, :, :] = 7.0                       # a plateau nothing leads out of
    with pytest.raises(W.WalkError, match="plateau"):
        W.walk(f, broken, (3, 3, 1), (0, 0, 0))
    f[3, 3, 1] = 0
    d[3, 3, 1] = 99.0                            # a rail end no neighbour achieves
    with pytest.raises(W.WalkError, match="no rail"):
        W.walk(f, d, (3, 3, 1), (0, 0, 0), rails=True)
