"""DESIGN.md 3.22 on the MI355X: kh_forest_components, kh_forest_measure and kh_forest_ticks through components_many, remove_dust_many,
remove_loops_many, remove_ticks_many and postprocess_many(stages="device"), against the host functions of kimimaro_amd.post (which
tests/golden/post.npz pins to the reference) -- array for array, plus id, space and transform."""
import ast
import os

import numpy as np
import pytest

import forest_ref as R
import join_ref as J
from kimimaro_amd.skeleton import Skeleton

pytestmark = pytest.mark.gpu

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "post.npz"))
N = int(GOLD["n"])
TIE_VECTORS_AT_MOST = 1          # postprocess vectors whose join a tree_tie decides (tests/test_join_host.py)


def canonical(vertices, edges, radii):
    """tests/test_post.py's: a skeleton as a graph on coordinates"""
    vertices = np.asarray(vertices, np.float32).reshape(-1, 3)
    edges = np.asarray(edges, np.int64).reshape(-1, 2)
    order = np.lexsort((vertices[:, 2], vertices[:, 1], vertices[:, 0]))
    rank = np.empty(len(order), np.int64)
    rank[order] = np.arange(len(order))
    e = np.sort(rank[edges], axis=1) if len(edges) else edges
    e = np.unique(e, axis=0) if len(e) else e
    return vertices[order], np.asarray(radii, np.float32)[order], e


def golden_input(i):
    return Skeleton(GOLD["vin_%d" % i].copy(), GOLD["ein_%d" % i].copy(), GOLD["rin_%d" % i].copy(), segid=7)


def golden_matches(i, got):
    gv, gr, ge = canonical(got.vertices, got.edges, got.radii)
    wv, wr, we = canonical(GOLD["vout_%d" % i], GOLD["eout_%d" % i], GOLD["rout_%d" % i])
    return gv.shape == wv.shape and np.array_equal(gv, wv) and np.array_equal(gr, wr) and ge.shape == we.shape and np.array_equal(ge, we)


def by_args(fn):
    """the vectors of one function grouped by their arguments: {args: [vector numbers]}"""
    groups = {}
    for i in range(N):
        if str(GOLD["fn_%d" % i]) == fn:
            groups.setdefault(str(GOLD["args_%d" % i]), []).append(i)
    return groups


def has_cycle(skel):
    """decided on the host: a component of Skeleton.components() that is no tree (ne != nv - 1)"""
    return any(c.edges.shape[0] != c.vertices.shape[0] - 1 for c in skel.components())


def in_batches(members, size):
    return [members] if size is None else [members[k:k + size] for k in range(0, len(members), size)]


# ---- 1. goldens ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [None, 7])
@pytest.mark.parametrize("fn,count", [("remove_dust", 36), ("remove_loops", 36), ("remove_ticks", 12)])
def test_stage_goldens(fn, count, size):
    from kimimaro_amd import post
    groups = by_args(fn)
    assert sum(len(m) for m in groups.values()) == count
    for args, members in groups.items():
        args = ast.literal_eval(args)
        for batch in in_batches(members, size):
            skels = [golden_input(i).consolidate(remove_disconnected_vertices=True) for i in batch]
            if fn == "remove_dust":
                got = post.remove_dust_many(skels, args[0])
            elif fn == "remove_loops":
                stats = {}
                got = post.remove_loops_many(skels, stats=stats)
                # only what the host finds cyclic may take the host path: a miscounted tree would come back equal, through it
                assert stats["loops_host"] == sum(has_cycle(s) for s in skels), (batch, stats)
            else:
                got = post.remove_ticks_many(skels, args[0])
            for i, skel, out in zip(batch, skels, got):
                assert golden_matches(i, out), (fn, i)
                assert R.same(out, getattr(post, fn)(skel, *args[:1] if fn != "remove_loops" else ())), (fn, i)


@pytest.mark.parametrize("size", [None, 7])
def test_postprocess_goldens(size):
    from kimimaro_amd import post
    from test_join_host import statement_postprocess
    groups = by_args("postprocess")
    assert sum(len(m) for m in groups.values()) == 46
    left_out = []
    for args, members in groups.items():
        dust, tick = ast.literal_eval(args)
        for batch in in_batches(members, size):
            got = post.postprocess_many([golden_input(i) for i in batch], dust_threshold=dust, tick_threshold=tick, stages="device")
            for i, skel in zip(batch, got):
                want, tied = statement_postprocess(i)
                assert skel.id == 7 and J.same(skel, want), i
                if tied:
                    left_out.append(i)
                    continue
                assert golden_matches(i, skel), i
    assert len(left_out) <= TIE_VECTORS_AT_MOST, left_out


# ---- 2. components ------------------------------------------------------------------------------------------------------------------
def test_labels_do_not_depend_on_edge_order():
    from kimimaro_amd import forest, ops
    rng = np.random.default_rng(7)
    n = 4097
    walk = rng.permutation(n)                                                 # the path visits the vertices in this order
    v = np.stack([np.arange(n), np.zeros(n), np.zeros(n)], axis=1).astype(np.float32)
    e = np.sort(np.stack([walk[:-1], walk[1:]], axis=1), axis=1)
    f = forest.pack([Skeleton(v, e[np.lexsort((e[:, 1], e[:, 0]))])])
    want = np.zeros(n, dtype=np.uint32)
    assert np.array_equal(forest.labels(ops.engine(), f), want)
    f.edges = np.ascontiguousarray(f.edges[rng.permutation(n - 1)])            # rows shuffled after the checks of pack
    f.edges[::3] = f.edges[::3, ::-1]
    assert np.array_equal(forest.labels(ops.engine(), f), want)


def test_five_thousand_two_vertex_components():
    from kimimaro_amd import post
    rng = np.random.default_rng(8)
    v = rng.permutation(20000)[:10000].reshape(-1, 1) * np.ones((1, 3))
    skel = Skeleton(v, np.arange(10000).reshape(5000, 2), segid=3)
    got = post.components_many([skel])[0]
    want = skel.components()
    assert len(got) == 5000 == len(want) and all(R.same(a, b) for a, b in zip(got, want))


def test_sizes_around_the_wave_and_the_block():
    from kimimaro_amd import ops, post
    rng = np.random.default_rng(9)
    skels = [R.random_tree(rng, n, segid=n) for n in (63, 64, 65, 255, 256, 257)]
    for s, comps in zip(skels, post.components_many(skels)):
        assert len(comps) == 1 and R.same(comps[0], s.consolidate())
    assert not ops.skeleton_component_labels(skels[3]).any()
    two = Skeleton.simple_merge([skels[0], skels[1]])
    two.vertices[63:] += 100
    lab = ops.skeleton_component_labels(two)
    assert lab.dtype == np.uint32 and sorted(np.unique(lab, return_counts=True)[1].tolist()) == [63, 64]


def test_three_hundred_random_forests():
    from kimimaro_amd import post
    rng = np.random.default_rng(10)
    skels = [R.forest_of(rng, int(rng.integers(1, 7)), 30) for _ in range(300)]
    for k, s in enumerate(skels):
        s.id, s.space = k, "physical"
    got = post.components_many(skels)
    for s, comps in zip(skels, got):
        want = s.components()
        assert len(comps) == len(want) and all(R.same(a, b) and np.array_equal(a.vertex_types, b.vertex_types) for a, b in zip(comps, want))


# ---- 3. dust ------------------------------------------------------------------------------------------------------------------------
def test_dust_at_the_threshold_is_the_hosts_decision():
    from kimimaro_amd import post
    v = np.array([[0, 0, 0], [5, 0, 0], [5, 5, 0], [5, 5, 5]], dtype=np.float32)
    skel = Skeleton(v, [[0, 1], [1, 2], [2, 3]], segid=4)
    for threshold in (15.0, np.nextafter(15.0, 0.0), np.nextafter(15.0, np.inf)):
        stats = {}
        got = post.remove_dust_many([skel], threshold, stats=stats)[0]
        assert R.same(got, post.remove_dust(skel, threshold)) and got.empty() == (threshold >= 15.0)      # equality drops it
        assert stats["dust_host_decided"] >= 1 and stats["components"] == 1


def test_dust_away_from_the_band_is_the_devices_decision():
    from kimimaro_amd import post
    rng = np.random.default_rng(12)
    skels = [R.forest_of(rng, int(rng.integers(1, 7)), 60) for _ in range(40)]
    comps = [c for s in skels for c in s.components()]
    cables = np.sort(np.array([c.cable_length() for c in comps]))
    gaps = np.flatnonzero((cables[1:] - cables[:-1]) > 1e-3 * cables[1:])
    k = int(gaps[gaps.size // 2])
    threshold = 0.5 * (cables[k] + cables[k + 1])
    # the host's own lengths: every component lies outside the band (twice over), so none may be handed to the host
    ne = np.array([c.edges.shape[0] for c in comps])
    cable = np.array([c.cable_length() for c in comps])
    assert np.all(np.abs(cable - threshold) > 2 * cable * ne * 2.0 ** -23)
    stats = {}
    got = post.remove_dust_many(skels, threshold, stats=stats)
    assert stats == {"components": len(comps), "dust_host_decided": 0}
    kept = 0
    for s, out in zip(skels, got):
        assert R.same(out, post.remove_dust(s, threshold))
        kept += out.vertices.shape[0]
    assert 0 < kept < sum(c.vertices.shape[0] for c in comps)


# ---- 4. ticks -----------------------------------------------------------------------------------------------------------------------
CASES = R.tick_cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_ticks(name):
    from kimimaro_amd import post
    skel, thresholds = CASES[name]
    for threshold in thresholds:
        want = post.remove_ticks(skel, threshold)
        got = post.remove_ticks_many([skel], threshold)[0]
        assert R.same(got, want), (name, threshold, got, want)


def test_ticks_of_two_hundred_random_trees():
    from kimimaro_amd import post
    rng = np.random.default_rng(13)
    skels = [R.random_tree(rng, int(rng.integers(2, 301)), extent=16, segid=k) for k in range(200)]
    removed = []
    for threshold in (4.0, 12.0, 40.0):
        got = post.remove_ticks_many(skels, threshold)
        for s, out in zip(skels, got):
            assert R.same(out, post.remove_ticks(s, threshold)), (s.id, threshold)
        removed.append(sum(s.edges.shape[0] - out.edges.shape[0] for s, out in zip(skels, got)))
    assert 0 < removed[0] < removed[1] < removed[2]


def test_a_cycle_raises_like_the_host():
    from kimimaro_amd import post
    ring = Skeleton(np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [5, 5, 5], [6, 5, 5]], dtype=np.float32),
                    [[0, 1], [1, 2], [2, 3], [0, 3], [4, 5]], segid=2)
    stats = {}
    assert R.same(post.remove_loops_many([ring], stats=stats)[0], post.remove_loops(ring)) and stats["loops_host"] == 1
    with pytest.raises(ValueError, match="distance_graph"):
        post.remove_ticks_many([ring], 10.0)


# ---- 5. integration -----------------------------------------------------------------------------------------------------------------
def test_device_stages_equal_host_stages():
    from kimimaro_amd import post
    skels = []
    for seed in range(20):
        skel = Skeleton.simple_merge(J.fragments(seed, denom=1024, nfrag=12, nvert=40, extent=24, rmax=4))
        skel.id = 50 + seed
        skels.append(skel)
    before = [s.clone() for s in skels]
    for dust, tick in ((0, 0), (10.0, 6.0), (30.0, 25.0)):
        stats = {}
        got = post.postprocess_many(skels, dust, tick, stages="device", stats=stats)
        want = post.postprocess_many(skels, dust, tick, stages="host")
        assert len(got) == len(want) == 20
        for a, b in zip(got, want):
            assert R.same(a, b), (dust, tick, a.id)
        assert (dust == 0) or stats["components"] > 0
    assert all(R.same(a, b) for a, b in zip(skels, before))
