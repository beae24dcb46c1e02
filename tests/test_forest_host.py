"""DESIGN.md 3.22 without a GPU: kimimaro_amd.forest's pack / unpack_* and the *_many functions of kimimaro_amd.post written on them,
with the statement of the device calls (tests/forest_ref.py: a numpy union-find, the kernel's tick tables in Python) standing in for
the device -- against Skeleton.components(), post.remove_dust, post.remove_loops and post.remove_ticks."""
import ast

import numpy as np
import pytest

import forest_ref as R
from kimimaro_amd import forest, post
from kimimaro_amd.skeleton import Skeleton
from test_post import GOLD, N


def some_skeletons(seed=3, count=40):
    rng = np.random.default_rng(seed)
    out = [R.forest_of(rng, int(rng.integers(1, 7)), 40) for _ in range(count)]
    out[5] = Skeleton()                                                       # empty
    out[9] = Skeleton(np.zeros((3, 3)), None)                                 # vertices without an edge
    out[12] = R.random_tree(rng, 30)                                          # one component
    for k, s in enumerate(out):
        s.id = 100 + k
    return out


def packed(skeletons):
    return forest.pack([s.consolidate() for s in skeletons])


def test_pack_lays_the_skeletons_back_to_back():
    skels = some_skeletons()
    f = packed(skels)
    cons = [s.consolidate() for s in skels]
    assert f.nverts == sum(c.vertices.shape[0] for c in cons) and f.nedges == sum(c.edges.shape[0] for c in cons)
    assert f.vstart[5] == f.vstart[6] and f.vstart[9] == f.vstart[10] and f.estart[5] == f.estart[6]      # the empty ones occupy nothing
    assert f.edges.dtype == np.uint32 and f.xyz.dtype == np.float32
    for k, c in enumerate(cons):
        assert np.array_equal(f.xyz[f.vstart[k]:f.vstart[k + 1]], c.vertices.reshape(-1, 3)[:f.vstart[k + 1] - f.vstart[k]])
        assert np.array_equal(f.edges[f.estart[k]:f.estart[k + 1]].astype(np.int64) - f.vstart[k], c.edges.astype(np.int64))
    assert np.all(f.skeleton_of_vertex(f.edges[:, 1].astype(np.int64)) == np.repeat(np.arange(len(skels)), np.diff(f.estart)))


def test_component_lists_equal_components():
    skels = some_skeletons()
    f = packed(skels)
    got = forest.unpack_components(f, R.labels(f.edges, f.nverts))
    assert len(got) == len(skels) and got[5] == [] and got[9] == []
    for s, comps in zip(skels, got):
        want = s.components()
        assert len(comps) == len(want)
        assert all(R.same(a, b) and np.array_equal(a.vertex_types, b.vertex_types) for a, b in zip(comps, want))
    assert len(got[12]) == 1 and R.same(got[12][0], skels[12].consolidate())     # one component: the consolidated skeleton


def test_dust_unpack_orders_vertices_like_remove_dust():
    skels = some_skeletons()
    f = packed(skels)
    m = R.measure(f)
    g = forest.Groups(f, m.comp)
    for threshold in (40.0, 400.0, 1e9):
        keep = np.array([forest.component_cable(f, g, k) > threshold for k in range(g.root.size)])
        got = forest.unpack_dust(f, g, keep)
        for s, skel in zip(skels, got):
            want = post.remove_dust(s, threshold) if not s.empty() else Skeleton()
            assert R.same(skel, want), threshold
    assert all(R.same(s, Skeleton()) for s in got)                           # every skeleton vanished under the last threshold


def test_component_cable_is_cable_length():
    skels = some_skeletons()
    f = packed(skels)
    g = forest.Groups(f, R.labels(f.edges, f.nverts))
    want = [c.cable_length() for s in skels for c in s.components()]
    assert [forest.component_cable(f, g, k) for k in range(g.root.size)] == want


def test_malformed_inputs_are_rejected(monkeypatch):
    a, b = R.random_tree(np.random.default_rng(1), 10).consolidate(), R.random_tree(np.random.default_rng(2), 10).consolidate()
    crossing = a.clone()
    crossing.edges[-1, 1] = 12                                                # a vertex of the NEXT skeleton
    with pytest.raises(ValueError, match="cross"):
        forest.pack([crossing, b])
    unsorted = a.clone()
    unsorted.edges = unsorted.edges[::-1].copy()
    with pytest.raises(ValueError, match="sorted"):
        forest.pack([unsorted])
    swapped = a.clone()
    swapped.edges = swapped.edges[:, ::-1].copy()
    with pytest.raises(ValueError, match="lo < hi"):
        forest.pack([swapped])
    # 2^31 vertices, by a faked size: the same lists are fine below the limit, refused at it, and cut between skeletons by batches
    assert forest.LIMIT == 2 ** 31
    assert forest.pack([a, b]).nverts == 20
    monkeypatch.setattr(forest, "LIMIT", 20)
    with pytest.raises(ValueError, match="fewer than 20"):
        forest.pack([a, b])
    assert forest.batches([a, b, a]) == [slice(0, 1), slice(1, 2), slice(2, 3)]
    monkeypatch.setattr(forest, "LIMIT", 21)
    assert forest.batches([a, b, a]) == [slice(0, 2), slice(2, 3)]
    monkeypatch.setattr(forest, "LIMIT", 10)
    with pytest.raises(ValueError, match="skeleton 0"):
        forest.batches([a, b])


def test_adjacency_and_critical_lists():
    s = R.star([R.straight(0, 1, 1), R.straight(1, 1, 2), R.straight(2, 1, 3)]).consolidate()
    path = Skeleton.from_path(np.arange(12).reshape(4, 3) + 500.0).consolidate()
    f = forest.pack([s, path])
    row, nbr, upper = forest.adjacency(f.edges, f.nverts)
    assert row[-1] == 2 * f.nedges and np.array_equal(np.diff(row.astype(np.int64)), np.bincount(f.edges.reshape(-1), minlength=f.nverts))
    own = np.repeat(np.arange(f.nverts), np.diff(row.astype(np.int64)))
    assert np.array_equal(np.stack([own[upper], nbr[upper]], axis=1), f.edges)
    assert all(np.all(np.diff(nbr[row[v]:row[v + 1]].astype(np.int64)) > 0) for v in range(f.nverts))
    m = R.measure(f)
    crit, start = forest.critical_lists(m.comp, m.nv, m.ne, m.degree)
    assert start.tolist() == [0, 4]                                           # the path is not listed: one superedge
    assert sorted(crit.tolist()) == np.flatnonzero(m.degree[:7] != 2).tolist()


@pytest.mark.parametrize("name", sorted(R.tick_cases()))
def test_tick_statement_equals_remove_ticks(name):
    skel, thresholds = R.tick_cases()[name]
    with R.host_engine():
        for threshold in thresholds:
            assert R.same(post.remove_ticks_many([skel], threshold)[0], post.remove_ticks(skel, threshold)), threshold


def test_many_functions_equal_the_host_functions():
    skels = some_skeletons()
    before = [s.clone() for s in skels]
    with R.host_engine():
        for s, comps in zip(skels, post.components_many(skels)):
            want = s.components()
            assert len(comps) == len(want) and all(R.same(a, b) for a, b in zip(comps, want))
        for threshold in (0, 25.0, 90.0):
            stats = {}
            for s, got in zip(skels, post.remove_dust_many(skels, threshold, stats=stats)):
                assert R.same(got, post.remove_dust(s, threshold))
                assert (got is s) == (s.empty() or threshold == 0)
            assert (stats["components"] > 0) == (threshold != 0) and stats["dust_host_decided"] == 0
            for s, got in zip(skels, post.remove_ticks_many(skels, threshold)):
                assert R.same(got, post.remove_ticks(s, threshold))
                assert (got is s) == (s.empty() or threshold == 0)
        stats = {}
        for s, got in zip(skels, post.remove_loops_many(skels, stats=stats)):
            assert R.same(got, post.remove_loops(s))
        assert stats["loops_host"] == 0
    assert all(R.same(a, b) for a, b in zip(skels, before))                   # inputs unmodified


def test_dust_band_hands_the_decision_to_the_host():
    v = np.array([[0, 0, 0], [5, 0, 0], [5, 5, 0], [5, 5, 5]], dtype=np.float32)
    skel = Skeleton(v, [[0, 1], [1, 2], [2, 3]], segid=4)
    with R.host_engine():
        for threshold in (15.0, np.nextafter(15.0, 0.0), np.nextafter(15.0, np.inf)):
            stats = {}
            got = post.remove_dust_many([skel], threshold, stats=stats)[0]
            assert R.same(got, post.remove_dust(skel, threshold)) and got.empty() == (threshold >= 15.0)
            assert stats["dust_host_decided"] == 1


def test_cycles_take_the_host_paths():
    ring = Skeleton(np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [5, 5, 5], [6, 5, 5]], dtype=np.float32),
                    [[0, 1], [1, 2], [2, 3], [0, 3], [4, 5]], segid=2)
    tree = R.random_tree(np.random.default_rng(4), 20)
    with R.host_engine():
        stats = {}
        got = post.remove_loops_many([tree, ring], stats=stats)
        assert stats["loops_host"] == 1
        assert R.same(got[0], post.remove_loops(tree)) and R.same(got[1], post.remove_loops(ring))
        with pytest.raises(ValueError, match="distance_graph"):
            post.remove_ticks_many([tree, ring], 10.0)
        with pytest.raises(ValueError, match="distance_graph"):
            post.remove_ticks(ring, 10.0)


def test_goldens_through_the_statement():
    """the remove_dust, remove_loops and remove_ticks vectors of tests/golden/post.npz through the *_many functions"""
    count = {"remove_dust": 0, "remove_loops": 0, "remove_ticks": 0}
    with R.host_engine():
        for i in range(N):
            fn = str(GOLD["fn_%d" % i])
            if fn not in count:
                continue
            count[fn] += 1
            args = ast.literal_eval(str(GOLD["args_%d" % i]))
            skel = Skeleton(GOLD["vin_%d" % i].copy(), GOLD["ein_%d" % i].copy(), GOLD["rin_%d" % i].copy(), segid=7)
            skel = skel.consolidate(remove_disconnected_vertices=True)
            if fn == "remove_dust":
                assert R.same(post.remove_dust_many([skel], args[0])[0], post.remove_dust(skel, args[0])), i
            elif fn == "remove_loops":
                assert R.same(post.remove_loops_many([skel])[0], post.remove_loops(skel)), i
            else:
                assert R.same(post.remove_ticks_many([skel], args[0])[0], post.remove_ticks(skel, args[0])), i
    assert count == {"remove_dust": 36, "remove_loops": 36, "remove_ticks": 12}


def test_the_new_names_are_exported():
    import kimimaro_amd
    for name in ("components_many", "remove_dust_many", "remove_loops_many", "remove_ticks_many"):
        assert getattr(kimimaro_amd, name) is getattr(post, name)
    with pytest.raises(ValueError):
        post.postprocess_many([], stages="both")


def test_consolidated_skips_only_what_consolidate_would_copy():
    rng = np.random.default_rng(6)
    skel = R.forest_of(rng, 3, 30)
    done = skel.consolidate()
    assert forest.consolidated(done) is done
    got = forest.consolidated(skel)
    assert got is not skel and R.same(got, done)
    for spoil in ("vertex order", "edge order", "edge direction", "unused vertex", "repeated vertex", "repeated edge", "edge dtype"):
        bad = done.clone()
        if spoil == "vertex order":
            bad.vertices[[0, 1]] = bad.vertices[[1, 0]]
        elif spoil == "edge order":
            bad.edges[[0, 1]] = bad.edges[[1, 0]]
        elif spoil == "edge direction":
            bad.edges[0] = bad.edges[0, ::-1]
        elif spoil == "unused vertex":
            bad.vertices = np.concatenate([bad.vertices, [[9e6, 0, 0]]]).astype(np.float32)
            bad.radii, bad.vertex_types = np.append(bad.radii, np.float32(1)), np.append(bad.vertex_types, np.uint8(0))
        elif spoil == "repeated vertex":
            bad.vertices[1] = bad.vertices[0]
        elif spoil == "repeated edge":
            bad.edges = np.concatenate([bad.edges[:1], bad.edges])
        else:
            bad.edges = bad.edges.astype(np.int64)
        got = forest.consolidated(bad)
        assert got is not bad and R.same(got, bad.consolidate()), spoil
    assert forest.consolidated(Skeleton()).empty()


def test_forest_sits_below_ops_and_post():
    """kimimaro_amd.forest is a package of its own (tests/test_layering.py lists the package's .py files); its layer is stated here: it
    imports _abi and skeleton and nothing else of kimimaro_amd, at module level or inside a function"""
    import os
    tree = ast.parse(open(os.path.join(os.path.dirname(forest.__file__), "__init__.py")).read())
    found = set()
    for node in ast.walk(tree):
        if isinstance(node, ast.ImportFrom) and node.level >= 1:
            found.update([node.module.split(".")[0]] if node.module else [a.name for a in node.names])
        elif isinstance(node, (ast.Import, ast.ImportFrom)):
            names = [node.module] if isinstance(node, ast.ImportFrom) else [a.name for a in node.names]
            found.update(n.split(".")[1] for n in names if n and n.startswith("kimimaro_amd."))
    assert found == {"_abi", "skeleton"}
