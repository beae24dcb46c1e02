"""The path walk of DESIGN.md 3.23 without a GPU: with tests/walk_paths_ref.py's statement of csrc/walk.hip in the device's place, paths_many
is Skeleton.paths and utility._xs_occurrences_many is utility._xs_occurrences, job for job and bit for bit.  tests/test_gpu_walk_paths.py
holds the device to the same statement, table for table."""
import ast
import glob
import os

import numpy as np
import pytest

import walk_paths_ref as W
import kimimaro_amd
from kimimaro_amd import forest, ops, post, utility
from kimimaro_amd.skeleton import Skeleton

PATH_CASES = W.path_cases()
OCC_CASES = W.occurrence_cases()


@pytest.mark.parametrize("name", sorted(PATH_CASES))
def test_paths_many_is_skeleton_paths(name):
    skels = PATH_CASES[name]
    want = [s.paths(return_indices=True) for s in skels]
    with W.host_engine():
        stats = {}
        got = post.paths_many(skels, stats=stats)
        points = post.paths_many(skels, return_indices=False)
        single = [ops.skeleton_paths(s) for s in skels]
    assert len(got) == len(skels) and all(W.same_paths(g, w) for g, w in zip(got, want))
    assert all(W.same_paths(g, w) for g, w in zip(single, want))
    assert all(W.same_paths(g, s.paths()) for g, s in zip(points, skels))
    assert stats["walk_host"] == (0 if name in W.TREE_CASES else 1)
    device = [w for s, w in zip(skels, want) if name in W.TREE_CASES or s is not skels[1]]
    assert stats["paths"] == sum(len(w) for w in device) and stats["occurrences"] == sum(len(p) for w in device for p in w)
    assert stats["walk_s"] >= 0 and stats["pack_s"] >= 0


def test_the_cases_are_what_they_claim():
    paths = {k: [s.paths(return_indices=True) for s in v] for k, v in PATH_CASES.items()}
    assert [p.tolist() for p in paths["one_edge"][0]] == [[1, 0]]
    assert [p.tolist() for p in paths["middle_chain"][0]] == [[3, 1, 0, 2, 4]]             # both ends 2 hops away: the smaller one
    assert [len(p) for p in paths["chain_1000"][0]] == [1000] and len(paths["star_70"][0]) == 69
    comb = PATH_CASES["comb_130"][0]
    assert len(paths["comb_130"][0]) == 129 and len(comb.branches()) + len(comb.terminals()) > 128
    tree = PATH_CASES["order_tree"][0]
    assert [p.tolist() for p in paths["order_tree"][0]] == [[5, 9, 8, 7, 1, 0, 3, 4, 6], [5, 9, 8, 7, 1, 2]]    # the deeper arm first
    assert tree._neighbours()[1] == [0, 2, 7]                                               # ... and the parent is the largest neighbour
    for s in PATH_CASES["three_interleaved"]:
        labels = W.labels(forest.Walk([s]).edges, s.vertices.shape[0]).astype(np.int64)
        proper = np.flatnonzero(np.bincount(labels) >= 2)
        assert proper.size >= 3 and np.count_nonzero(np.bincount(labels) == 1) >= 1
        spans = [(np.flatnonzero(labels == r).min(), np.flatnonzero(labels == r).max()) for r in proper]
        assert any(a0 < b0 < a1 for a0, a1 in spans for b0, _ in spans)                     # numbers interleave between components
    raw = PATH_CASES["untidy"][0].edges.astype(np.int64)
    key = np.sort(raw, axis=1)
    assert np.any(raw[:, 0] == raw[:, 1]) and np.any(raw[:, 0] > raw[:, 1]) and np.unique(key, axis=0).shape[0] < key.shape[0]
    assert np.any(np.diff((key[:, 0] << 32) | key[:, 1]) < 0)


@pytest.mark.parametrize("name", sorted(PATH_CASES))
def test_orientation_tables_are_a_rooted_tree(name):
    """the statement's parent / depth checked without its own loop: what an orientation is"""
    w = forest.Walk(PATH_CASES[name])
    comp = W.labels(w.edges, w.nverts)
    T = forest.WalkTables(w, comp)
    R = W.orient_tables(w, comp, T, fill=0xA5)
    listed = np.zeros(w.nverts, dtype=bool)
    listed[T.root] = True
    listed = listed[comp.astype(np.int64)]
    parent, depth = R.parent.astype(np.int64), R.depth.astype(np.int64)
    roots = listed & (R.parent == W.NONE)
    assert np.all(R.parent[~listed] == W.NONE) and np.all(depth[~listed] == 0) and np.all(depth[roots] == 0)
    assert np.count_nonzero(roots) == T.root.size and np.all(w.degree[roots] == 1)
    inner = np.flatnonzero(listed & ~roots)
    assert np.array_equal(depth[inner], depth[parent[inner]] + 1) and np.array_equal(comp[parent[inner]], comp[inner])
    key = (np.minimum(inner, parent[inner]) << 32) | np.maximum(inner, parent[inner])
    assert np.all(np.isin(key, (w.edges[:, 0].astype(np.int64) << 32) | w.edges[:, 1]))    # every parent link is an edge
    leaves = R.path_leaf.astype(np.int64)
    assert np.all(w.degree[leaves] == 1) and not roots[leaves].any() and np.unique(leaves).size == leaves.size == T.npaths
    assert np.array_equal(R.path_len, depth[leaves] + 1)
    # what no kernel writes keeps the sentinel: the slots of vertices that are not critical
    mine = np.zeros(w.nverts, dtype=bool)
    mine[T.crit] = True
    own = np.repeat(np.arange(w.nverts), w.degree)
    word = int(W.filled(1, np.uint32, 0xA5)[0])
    for table in W.Tables.SLOT:
        assert np.all(getattr(R, table)[~mine[own]] == word), table


def occurrences(skel, an, offset, shape, window, step):
    vox, ov, on = utility._xs_occurrences(skel, an, offset, shape, window, step)
    mask = np.zeros(len(skel.vertices), dtype=bool)
    mask[skel.branches()] = True
    return vox, ov, on, mask


def assert_same_occurrences(got, want, note):
    for (gv, go, gn, gb), (wv, wo, wn, wb) in zip(got, want):
        assert gv.dtype == wv.dtype == np.int64 and np.array_equal(gv, wv), note
        assert go.dtype == wo.dtype == np.int64 and np.array_equal(go, wo), note
        assert gn.dtype == wn.dtype == np.float64 and gn.shape == wn.shape and np.array_equal(W.bits(gn), W.bits(wn)), note
        assert gb.dtype == bool and np.array_equal(gb, wb), note
    assert len(got) == len(want)


@pytest.mark.parametrize("name", sorted(OCC_CASES))
def test_occurrences_many_is_xs_occurrences(name):
    jobs, an, shape, windows, steps = OCC_CASES[name]
    for window in windows:
        for step in steps:
            want = [occurrences(s, an, offset, shape, window, step) for s, _, offset in jobs]
            with W.host_engine():
                stats = {}
                got = utility._xs_occurrences_many(ops.engine(), jobs, an, shape, window, step, stats)
            assert_same_occurrences(got, want, (window, step))
            assert stats["walk_host"] == (1 if name == "cyclic_between" else 0)
            assert stats["occurrences"] == sum(w[1].size for w in want)


def test_the_occurrence_cases_reach_their_regimes():
    one = np.ones(3, dtype=np.float32)
    nan_rows = lambda name, window, step=1: [np.isnan(utility._xs_occurrences(s, OCC_CASES[name][1], o, OCC_CASES[name][2], window, step)[2]).all(axis=1)
                                             for s, _, o in OCC_CASES[name][0]]
    assert nan_rows("twin_voxel", 1)[0].sum() == 1                          # two consecutive vertices in one voxel: one zero difference
    assert nan_rows("zigzag", 2)[0].sum() >= 5 and not nan_rows("zigzag", 1)[0].any()      # the smoothing cancels
    skel = OCC_CASES["shared_voxel"][0][0][0]
    vox, ov, _ = utility._xs_occurrences(skel, one, (0, 0, 0), W.SHAPE, 1, 1)
    assert np.array_equal(vox[2], vox[4]) and 2 not in ov and 4 in ov       # canon: the LAST vertex in the voxel
    skel = OCC_CASES["outside"][0][0][0]
    vox, ov, _ = utility._xs_occurrences(skel, one, (0, 0, 0), W.SHAPE, 1, 1)
    gone = ~np.all((vox >= 0) & (vox < np.array(W.SHAPE)), axis=1)
    assert gone.sum() == 7 and all((vox[gone, a] < 0).any() and (vox[gone, a] >= W.SHAPE[a]).any() for a in range(3))
    assert not np.isin(np.flatnonzero(gone), ov).any()
    for (s, _, o), L in zip(OCC_CASES["lengths"][0], (2, 3, 4, 6, 7)):
        for step in (1, 2, 3):
            ov = utility._xs_occurrences(s, one, o, W.SHAPE, 1, step)[1]
            assert ov[0] == L - 1 and ov[-1] == 0 and ov.size == len(set([0, L - 1] + list(range(step - 1, L, step))))
    jobs, an = OCC_CASES["physical"][0], OCC_CASES["physical"][1]
    assert jobs[0][0].space == "physical" and jobs[1][0].space == "voxel" and an.tolist() == [16, 16, 40] and jobs[0][2] != (0, 0, 0)


def test_the_second_pass_is_a_difference_of_running_sums_not_a_window_sum():
    """on this file's own input: with n = 3 the window-sum form of the second moving average differs from numpy's, the sequential form
    does not -- so the comparisons above are not blind to the summation order"""
    skel = OCC_CASES["random_walk_60"][0][0][0]
    path = skel.paths(return_indices=True)[0]
    vox = np.round(skel.vertices).astype(np.int64)
    d = W.differences(vox, path)
    for n, differs in ((2, False), (3, True), (5, True)):
        normals = utility.moving_average(d.astype(np.float32), n)
        want = utility.moving_average(normals[::-1], n)[::-1]
        first = W.first_pass(d, n)
        assert np.array_equal(first.view(np.uint64), np.asarray(normals).view(np.uint64))
        assert np.array_equal(W.second_pass(first, n).view(np.uint64), want.view(np.uint64))
        wrong = W.second_pass(first, n, window_sum=True)
        assert np.any(wrong.view(np.uint64) != want.view(np.uint64)) == differs, n
        assert np.allclose(wrong, want, rtol=0, atol=1e-12)


@pytest.mark.parametrize("length", (1, 2, 3, 5))
def test_reflect_is_numpys_symmetric_pad(length):
    a = np.arange(length)
    for n in (2, 3, 7, 11):
        assert np.pad(a, n, mode="symmetric").tolist() == [W.reflect(j, length) for j in range(-n, length + n)]


def test_a_long_call_is_cut_between_skeletons():
    """paths share their trunk, so a call's occurrences can pass the limit where its vertices and slots do not"""
    skels = [W.comb(5), W.comb(5), W.comb(5)]
    want = [s.paths(return_indices=True) for s in skels]
    assert [sum(len(p) for p in w) for w in want] == [22] * 3 and [len(w) for w in want] == [4] * 3
    with W.host_engine():
        calls = []
        emit = forest.walk_emit
        forest.walk_emit = lambda *a: calls.append(a[2:4]) or emit(*a)
        try:
            w = forest.walk(ops.engine(), skels, limit=60)                   # 30 vertices, 54 slots, 66 occurrences: two emit calls
            assert calls == [(0, 8), (8, 12)]
            assert all(W.same_paths(w.paths(k), want[k]) for k in range(3))
            with pytest.raises(ValueError, match="skeleton 0 has 22 vertices on its paths"):
                forest.walk(ops.engine(), skels[:1], limit=20)               # 10 vertices, 18 slots
        finally:
            forest.walk_emit = emit
    assert forest.walk_batches(skels, limit=25) == [slice(0, 1), slice(1, 2), slice(2, 3)]
    assert forest.walk_batches(skels, limit=40) == [slice(0, 2), slice(2, 3)]
    with pytest.raises(ValueError):
        forest.walk_batches(skels, limit=18)
    with pytest.raises(ValueError, match="outside its 2 vertices"):
        forest.Walk([W.skeleton([[0, 0, 0], [1, 0, 0]], [[0, 2]])])


def test_far_voxels_take_the_host_path():
    far = W.line(5)
    far.vertices = far.vertices + np.float32(forest.VOX_LIMIT)
    jobs = [(W.star(3), 1, (0, 0, 0)), (far, 2, (0, 0, 0))]
    one = np.ones(3, dtype=np.float32)
    want = [occurrences(s, one, o, W.SHAPE, 3, 1) for s, _, o in jobs]
    with W.host_engine():
        stats = {}
        got = utility._xs_occurrences_many(ops.engine(), jobs, one, W.SHAPE, 3, 1, stats)
    assert_same_occurrences(got, want, "far")
    assert stats["walk_host"] == 1


def test_walk_is_host_or_device():
    skel = W.line(4)
    vol = np.ones((8, 8, 8), dtype=np.uint8)
    for call in (lambda: kimimaro_amd.cross_sectional_area(vol, [skel], walk="bogus"),
                 lambda: kimimaro_amd.cross_sectional_area_filled(vol, [skel], walk="bogus"),
                 lambda: kimimaro_amd.cross_sectional_area_single(vol, skel, walk="bogus"),
                 lambda: kimimaro_amd.cross_sectional_area_chunked(vol, [skel], chunk_shape=(8, 8, 8), walk="bogus"),
                 lambda: kimimaro_amd.cross_sectional_area_filled_chunked(vol, [skel], chunk_shape=(8, 8, 8), walk="bogus"),
                 lambda: utility._xs_run(None, None, None, (8, 8, 8), np.ones(3, np.float32), [], 1, 1, False, False, None, walk="Device")):
        with pytest.raises(ValueError, match="walk must be"):
            call()


def test_the_new_names_are_exported():
    assert kimimaro_amd.paths_many is post.paths_many
    assert callable(ops.skeleton_paths) and callable(utility._xs_occurrences_many)


def test_no_fallback_without_a_device():
    try:
        kimimaro_amd._abi.require_gpu()
    except kimimaro_amd.HipUnavailableError:
        with pytest.raises(kimimaro_amd.HipUnavailableError):
            kimimaro_amd.paths_many([W.line(3)])
    else:
        assert W.same_paths(kimimaro_amd.paths_many([W.line(3)])[0], W.line(3).paths(return_indices=True))


def test_forest_package_keeps_its_layer():
    """every module of kimimaro_amd.forest imports _abi and skeleton and nothing else of kimimaro_amd"""
    found = set()
    for path in glob.glob(os.path.join(os.path.dirname(forest.__file__), "*.py")):
        for node in ast.walk(ast.parse(open(path).read())):
            if isinstance(node, ast.ImportFrom) and node.level >= 1:
                found.update([node.module.split(".")[0]] if node.module else [a.name for a in node.names])
            elif isinstance(node, (ast.Import, ast.ImportFrom)):
                names = [node.module] if isinstance(node, ast.ImportFrom) else [a.name for a in node.names]
                found.update(n.split(".")[1] for n in names if n and n.startswith("kimimaro_amd."))
    assert found == {"_abi", "skeleton"}
