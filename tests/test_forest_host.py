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


# ---- the model's tables and the exact cable (tests/test_gpu_forest_calls.py holds the device to them) ------------------------------------
FILL = 0xA5
WORD = int(R.filled(1, np.uint32, FILL)[0])
TABLE_CALLS = R.TABLE_CASES + ("tick_forest",)


def survival(f, threshold):
    """bool per edge row of the forest: the row is still an edge of post.remove_ticks(skeleton, threshold)"""
    out = np.ones(f.nedges, dtype=bool)
    for k, skel in enumerate(f.skeletons):
        a, b = int(f.estart[k]), int(f.estart[k + 1])
        if a == b or threshold == 0:                                          # (remove_ticks hands a skeleton back under a zero threshold)
            continue
        left = np.asarray(post.remove_ticks(skel, threshold).edges, dtype=np.int64).reshape(-1, 2)
        mine = f.edges[a:b].astype(np.int64) - int(f.vstart[k])
        out[a:b] = np.isin((mine[:, 0] << 32) | mine[:, 1], (left[:, 0] << 32) | left[:, 1])
    return out


@pytest.mark.parametrize("name", TABLE_CALLS)
def test_tick_tables_alive_is_remove_ticks_survival(name):
    f, m, thresholds = R.table_call(name)
    assert thresholds[0] == 0.0 and thresholds[-1] == np.inf and len(thresholds) >= 3
    removed = []
    for threshold in thresholds:
        T = R.tick_tables(f, m, threshold, fill=FILL)
        both = np.argsort(slot_keys(T), kind="stable").reshape(-1, 2)         # the two slots of every edge
        assert T.alive.dtype == np.uint8 and np.array_equal(T.alive[both[:, 0]], T.alive[both[:, 1]])
        got = T.alive[T.upper] != 0
        assert np.array_equal(got, survival(f, threshold)), threshold
        assert np.array_equal(got, R.ticks(f, m, threshold))
        removed.append(int(f.nedges - got.sum()))
    assert removed[0] == 0 and removed == sorted(removed) and removed[-1] > 0     # a larger threshold goes on where a smaller one stops


def slot_keys(T):
    row = T.row.astype(np.int64)
    own = np.repeat(np.arange(row.size - 1), np.diff(row))
    nbr = T.nbr.astype(np.int64)
    return (np.minimum(own, nbr) << 32) | np.maximum(own, nbr)


def chain(row, nbr, c, s):
    """the vertices from the critical vertex c through its slot s to the next critical vertex"""
    path = [int(c), int(nbr[s])]
    while row[path[-1] + 1] - row[path[-1]] == 2:
        n0, n1 = int(nbr[row[path[-1]]]), int(nbr[row[path[-1]] + 1])
        path.append(n1 if n0 == path[-2] else n0)
    return path


@pytest.mark.parametrize("name", TABLE_CALLS)
def test_threshold_zero_leaves_the_orientation(name):
    """the tables after a call with threshold 0, checked without the model's own loop: what an orientation of a contracted tree is"""
    f, m, _ = R.table_call(name)
    T = R.tick_tables(f, m, 0.0, fill=FILL)
    row, nbr = T.row.astype(np.int64), T.nbr.astype(np.int64)
    deg = np.diff(row)
    own = np.repeat(np.arange(f.nverts), deg)
    crit, start = T.crit.astype(np.int64), T.crit_start.astype(np.int64)
    assert T.alive.all() and np.array_equal(T.arity, np.where(deg >= 3, deg, 0)) and T.arity.dtype == np.int32
    assert [getattr(T, k).dtype for k in T.SLOT + T.RECORD] == [np.uint32, np.uint32, np.float32, np.uint32] + [np.uint32] * 5 + [np.float64, np.uint8]
    # slots: written for the listed critical vertices and for no other
    mine = np.zeros(f.nverts, dtype=bool)
    mine[crit] = True
    for table in T.SLOT:
        words = getattr(T, table).view(np.uint32)
        assert np.all(words[~mine[own]] == WORD) and (table == "len32" or np.all(words[mine[own]] != WORD)), table
    slots = np.flatnonzero(mine[own])
    twin, far = T.twin.astype(np.int64), T.far.astype(np.int64)
    assert np.array_equal(twin[twin[slots]], slots) and np.array_equal(far[twin[slots]], own[slots]) and np.array_equal(own[twin[slots]], far[slots])
    for s in slots.tolist():
        path = chain(row, nbr, own[s], s)
        assert path[-1] == far[s] and nbr[twin[s]] == path[-2]
        assert float(T.len32[s]) == R.directed_sums(f.xyz[path])[0], s
    assert start.size - 1 >= 1 and start[-1] == crit.size
    for c in range(start.size - 1):
        cs, ce = int(start[c]), int(start[c + 1])
        assert T.tail[c] == ce
        terminals = crit[cs:ce][deg[crit[cs:ce]] == 1]
        queue = T.queue[cs:ce].astype(np.int64)
        assert np.array_equal(np.sort(queue), crit[cs:ce]) and queue[0] == terminals.min()
        assert T.sb[cs] == R.NONE and T.flag[cs] == 0
        assert all(getattr(T, k)[cs:cs + 1].tobytes() == bytes([FILL]) * getattr(T, k).itemsize for k in ("ea", "eb", "sa", "len"))
        # records cs + 1 .. ce - 1: one per critical vertex but the start, each the superedge through which its vertex was reached
        i = np.arange(cs + 1, ce)
        assert i.size == (ce - cs) - 1 and np.all(np.isin(T.flag[i], (R.LIVE, R.LIVE | R.REMOVABLE)))
        ea, eb, sa, sb = (getattr(T, k)[i].astype(np.int64) for k in ("ea", "eb", "sa", "sb"))
        assert np.array_equal(eb, queue[1:]) and np.array_equal(own[sa], ea) and np.array_equal(own[sb], eb)
        assert np.array_equal(twin[sa], sb) and np.array_equal(T.rec[sa], i) and np.array_equal(T.rec[sb], i)
        assert np.array_equal(T.len[i].view(np.uint64), T.len32[sa].astype(np.float64).view(np.uint64))
        place = {int(v): k for k, v in enumerate(queue)}
        assert all(place[int(a)] < k + 1 for k, a in enumerate(ea))            # the parent was queued before its child
        assert np.array_equal(T.flag[i] == (R.LIVE | R.REMOVABLE), (deg[ea] == 1) | (deg[eb] == 1))


def chunked_queue(T, c):
    """the queue of listed component c as forest_ticks_kernel fills it: rounds of at most 64 entries, a lane per entry, every lane's
    children placed behind the queue's end at the exclusive prefix sum of the lanes' child counts -- the lanes taken LAST FIRST here,
    which must not matter"""
    row = T.row.astype(np.int64)
    cs, ce = int(T.crit_start[c]), int(T.crit_start[c + 1])
    terminals = [int(v) for v in T.crit[cs:ce] if row[v + 1] - row[v] == 1]
    queue, via = [min(terminals)], [R.NONE]
    head = 0
    while head < len(queue):
        n = min(64, len(queue) - head)
        cnt = np.array([row[queue[head + lane] + 1] - row[queue[head + lane]] - (via[head + lane] != R.NONE) for lane in range(n)])
        pos = len(queue) + np.cumsum(cnt) - cnt
        queue += [None] * int(cnt.sum())
        via += [None] * int(cnt.sum())
        for lane in reversed(range(n)):
            u, p = queue[head + lane], int(pos[lane])
            for s in range(row[u], row[u + 1]):
                if s != via[head + lane]:
                    queue[p], via[p] = int(T.far[s]), int(T.twin[s])
                    p += 1
        head += n
    return queue


def test_rounds_of_64_give_the_queue_of_the_fifo():
    f, m, _ = R.table_call("wide_round")
    T = R.tick_tables(f, m, 0.0, fill=FILL)
    assert f.nverts == 281 and T.crit_start.tolist() == [0, 211]              # 140 leaves, 70 forks and the hub
    queue = chunked_queue(T, 0)
    assert queue == T.queue.tolist()
    deg = np.diff(T.row.astype(np.int64))
    assert deg[queue[2]] == 70 or deg[queue[3]] == 70                         # the hub is in the third round
    assert [deg[v] for v in queue[4:73]] == [3] * 69                          # the fourth: 69 forks, lanes 0..63 and then 0..4


# ---- the measures ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.measure_shapes()) + ["all"])
def test_measure_shapes_have_an_exact_cable(name):
    """the CPU side of tests/test_gpu_forest_calls.py's bit-for-bit cable: its condition holds, and the model's sum in edge order is
    math.fsum's already"""
    f, m, exact = R.measure_call(name)
    by_root = R.lengths_by_root(f, m.comp)
    assert sorted(by_root) == np.flatnonzero(m.ne).tolist() == np.flatnonzero(m.nv).tolist()
    assert all(R.cable_is_exact(lengths) for lengths in by_root.values())
    assert np.array_equal(exact.view(np.uint64), m.cable.view(np.uint64))
    assert int(m.nv.sum()) == f.nverts and int(m.ne.sum()) == f.nedges and int(m.degree.sum()) == 2 * f.nedges


def test_measure_shapes_reach_their_regimes():
    for n in R.PATH_EDGES:
        f, m, _ = R.measure_call("path_%d" % n)
        assert f.nedges == n and m.nv[0] == n + 1 and m.ne[0] == n and not m.comp.any()
        d = np.abs(np.diff(f.xyz.astype(np.float64), axis=0))
        assert np.all((d > 0).sum(axis=0) >= n - 2)                           # all three axes move
        sq = d * d
        assert np.any(sq != sq.astype(np.float32))                            # and a square rounds in float32
    f, m, _ = R.measure_call("pairs_5000")
    assert f.nedges == 5000 == R.wave_runs(m.comp[f.edges[:, 0]]) == np.count_nonzero(m.nv) and np.all(m.nv[m.nv > 0] == 2)
    f, m, _ = R.measure_call("braid_3x700")
    assert f.nedges == 2097 == R.wave_runs(m.comp[f.edges[:, 0]]) and np.flatnonzero(m.nv).tolist() == [0, 1, 2]
    assert m.nv[:3].tolist() == [700] * 3 and m.ne[:3].tolist() == [699] * 3
    f, m, _ = R.measure_call("hub_5000")
    assert m.degree[2500] == 5000 and m.degree[0] == 1 and not m.comp.any() and m.ne[0] == 5000
    assert R.wave_runs(m.comp[f.edges[:, 0]]) == -(-5000 // 64)
    f, m, _ = R.measure_call("ring_and_tree")
    roots = np.flatnonzero(m.nv)
    assert m.nv[roots].tolist() == [64, 40] and m.ne[roots].tolist() == [64, 39]
    f, m, exact = R.measure_call("one_edge")
    assert f.nedges == 1 and exact[0] == float(R.edge_lengths(f.xyz, f.edges)[0]) and exact[1] == 0
    f, m, _ = R.measure_call("forests_300")
    assert (f.nverts, f.nedges) == (16562, 15515)


def test_cable_is_exact_is_a_condition_on_the_spread():
    assert R.cable_is_exact([]) and R.cable_is_exact([1.0]) and R.cable_is_exact([1.0, 2.0 ** 29])
    assert not R.cable_is_exact([1.0, 2.0 ** 30]) and not R.cable_is_exact([0.0, 1.0]) and not R.cable_is_exact([1.5, np.inf])
    assert R.cable_is_exact([1.75] * 1000) and not R.cable_is_exact([1.0 + 2.0 ** -23] * 2 ** 20 + [2.0 ** 30])
    # where it fails the order can matter: 2^30 + 1.5 + 1.5 from the left keeps both halves, from the right it does not
    terms = [2.0 ** 53, 1.0, 1.0]
    assert (terms[0] + terms[1]) + terms[2] != terms[0] + (terms[1] + terms[2])


@pytest.mark.parametrize("name", R.TREE_SHAPES)
def test_tree_shapes_take_no_host_path_in_the_statement(name):
    skels = R.measure_shapes()[name]
    f, m, _ = R.measure_call(name)
    threshold = R.dust_threshold(f, m)
    with R.host_engine():
        stats = {}
        got = post.remove_loops_many(skels, stats=stats)
        assert stats["loops_host"] == 0 and all(R.same(a, s.consolidate()) for a, s in zip(got, skels))
        got = post.remove_dust_many(skels, threshold, stats=stats)
        assert stats["dust_host_decided"] == 0 and stats["components"] == np.count_nonzero(m.nv)
