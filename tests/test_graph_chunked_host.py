"""skeletonize_graph_chunked without a GPU: the whole driver run on the CPU oracle through its private hooks, against
the composition written out in tests/graph_chunked_ref.py, and its argument checks."""
import numpy as np
import pytest

import chunked_ref as R
import graph_chunked_ref as GR
import graph_ref as G
from kimimaro_amd import post, skeletonize_chunked, skeletonize_graph_chunked

CHUNKS = R.DATASETS[0][3]


def host_postprocess(skeletons, dust_threshold, tick_threshold):
    return [post.postprocess(s, dust_threshold, tick_threshold) for s in skeletons]


def oracle_run(labels, **kwargs):
    from oracle import pipeline as P
    return P.skeletonize(labels, **kwargs)


def on_oracle(lab, chunk_shape, driver=skeletonize_graph_chunked, **kwargs):
    kw = dict(teasar_params=R.TP, anisotropy=R.AN, dust_threshold=R.CHUNK_DUST, post_dust_threshold=R.POST_DUST, tick_threshold=R.TICK)
    if driver is skeletonize_graph_chunked:
        kw["_graph_of"] = G.graph_of
    kw.update(kwargs)
    return driver(lab, chunk_shape, _skeletonize=oracle_run, _postprocess=host_postprocess, **kw)


def supervoxels_of_the_wall():
    """(supervoxels, merges) whose graph is GR.walled_graph(): the walled label cut into two supervoxels at the wall, which no pair
    joins; another label cut in two and joined again by `merges`"""
    lab = R.dataset(0)
    g, label, axis, at = GR.walled_graph()
    assert axis == 0
    sv = lab.astype(np.uint32)
    sv[at + 1:][lab[at + 1:] == label] = label + 5000
    other = int(next(v for v in np.unique(lab) if v not in (0, label)))
    xs = np.flatnonzero((lab == other).any(axis=(1, 2)))
    mid = int(xs[len(xs) // 2])
    sv[mid:][lab[mid:] == other] = other + 5000
    return sv, [(other + 5000, other), (label, 0), (label, label)]


@pytest.fixture(scope="module")
def by_graph():
    return on_oracle(R.dataset(0), CHUNKS, voxel_graph=GR.walled_graph()[0])


def test_the_supervoxels_restate_the_walled_graph():
    lab = R.dataset(0)
    g, label, _, at = GR.walled_graph()
    sv, merges = supervoxels_of_the_wall()
    np.testing.assert_array_equal(G.graph_of(sv, 26, merges), g)
    plain = G.graph_of(lab)
    changed = np.argwhere(plain != g)
    assert changed.shape[0] > 50 and set(changed[:, 0].tolist()) == {at, at + 1} and (lab[tuple(changed.T)] == label).all()
    cuts = {b[3][0] - 1 for b in R.boxes(lab.shape, CHUNKS)} | {b[2][0] for b in R.boxes(lab.shape, CHUNKS)}
    assert all(abs(at - c) >= 3 for c in cuts)                                   # the wall stands away from the cuts


def test_driver_on_the_oracle_equals_the_composition(by_graph):
    lab = R.dataset(0)
    g = GR.walled_graph()[0]
    timings = {}
    frags = GR.fragments(lab, CHUNKS, oracle_run, graph=g)
    want = GR.compose(frags, post.postprocess)
    R.assert_same(by_graph, want)
    assert len(want) >= 8 and sum(len(f) > 1 for f in frags.values()) >= R.DATASETS[0][5]
    raw = on_oracle(lab, CHUNKS, voxel_graph=g, merge=False, timings=timings)
    assert list(raw) == list(frags) and timings["chunks"] == R.DATASETS[0][4]
    for label in frags:
        assert len(raw[label]) == len(frags[label]) and all(a == b for a, b in zip(raw[label], frags[label]))


def test_both_graph_routes_give_the_same_result(by_graph):
    sv, merges = supervoxels_of_the_wall()
    R.assert_same(on_oracle(R.dataset(0), CHUNKS, supervoxels=sv, merges=merges), by_graph)


def test_the_wall_changes_the_result(by_graph):
    label = GR.walled_graph()[1]
    plain = on_oracle(R.dataset(0), CHUNKS, driver=skeletonize_chunked)
    assert label in plain and label in by_graph
    a, b = plain[label], by_graph[label]
    assert a.vertices.shape != b.vertices.shape or not np.array_equal(a.vertices, b.vertices)
    # (the other labels may move as well: the transform with a graph measures to the wall between two voxels, half a pitch nearer
    # than the next voxel's centre -- tests/test_gpu_graph.py::test_edt_wall_is_half_a_pitch_away.)  Against the graph of the labels
    # WITHOUT the wall it is the walled label alone that changes:
    open_graph = on_oracle(R.dataset(0), CHUNKS, voxel_graph=G.graph_of(R.dataset(0)))
    c = open_graph[label]
    assert c.vertices.shape != b.vertices.shape or not np.array_equal(c.vertices, b.vertices)
    same = [k for k in open_graph if k != label]
    R.assert_same({k: by_graph[k] for k in same if k in by_graph}, {k: open_graph[k] for k in same})


def test_a_single_chunk_is_skeletonize_with_the_graph_then_postprocess():
    from oracle import pipeline as P
    lab = R.dataset(0)
    g = GR.walled_graph()[0]
    got = on_oracle(lab, (128, 128, 128), voxel_graph=g)
    whole = P.skeletonize(lab, teasar_params=R.TP, anisotropy=R.AN, dust_threshold=R.CHUNK_DUST, fix_borders=True, fix_branching=True,
                          voxel_graph=g)
    want = {k: post.postprocess(R.placed(s, (0, 0, 0), k), R.POST_DUST, R.TICK) for k, s in sorted(whole.items())}
    R.assert_same(got, {k: s for k, s in want.items() if not s.empty()})


def test_arguments():
    lab = np.ones((8, 8, 8), np.uint8)
    g = np.zeros((8, 8, 8), np.uint32)
    hooks = dict(_skeletonize=oracle_run, _postprocess=host_postprocess, _graph_of=G.graph_of)
    with pytest.raises(ValueError):
        skeletonize_graph_chunked(lab, (4, 4, 4), **hooks)
    with pytest.raises(ValueError):
        skeletonize_graph_chunked(lab, (4, 4, 4), voxel_graph=g, supervoxels=lab, **hooks)
    with pytest.raises(ValueError):
        skeletonize_graph_chunked(lab, (4, 4, 4), voxel_graph=g, merges=[(1, 2)], **hooks)
    with pytest.raises(NotImplementedError):
        skeletonize_graph_chunked(lab, (4, 4, 4), voxel_graph=g, fix_avocados=True, **hooks)
    with pytest.raises(NotImplementedError):
        skeletonize_graph_chunked(lab, (4, 4, 4), fix_avocados=True)            # before anything else is looked at
    for excluded in ("fill_holes_global", "filled_store", "region_store", "_fill"):
        with pytest.raises(TypeError):
            skeletonize_graph_chunked(lab, (4, 4, 4), voxel_graph=g, **{excluded: None}, **hooks)
    for other in (np.zeros((8, 8, 7), np.uint32), np.zeros((8, 8), np.uint32)):
        with pytest.raises(ValueError):
            skeletonize_graph_chunked(lab, (4, 4, 4), voxel_graph=other, **hooks)
        with pytest.raises(ValueError):
            skeletonize_graph_chunked(lab, (4, 4, 4), supervoxels=other, **hooks)
    assert skeletonize_graph_chunked(np.zeros((8, 8, 8), np.uint8), (4, 4, 4), voxel_graph=g, **hooks) == {}
    # the driver it wraps keeps refusing the keyword
    with pytest.raises(TypeError):
        skeletonize_chunked(lab, (4, 4, 4), voxel_graph=g)


def test_names_and_no_cpu_fallback_without_the_hooks():
    import torch
    import kimimaro_amd
    from kimimaro_amd import ops
    assert kimimaro_amd.skeletonize_graph_chunked is post.skeletonize_graph_chunked
    assert kimimaro_amd.voxel_connectivity_graph_chunked is post.voxel_connectivity_graph_chunked
    assert kimimaro_amd.voxel_connectivity_graph is ops.voxel_connectivity_graph
    assert kimimaro_amd.skeletonize_chunked is post.skeletonize_chunked
    for bad in (4, 8, 27):
        with pytest.raises(ValueError):
            kimimaro_amd.voxel_connectivity_graph(np.ones((4, 4, 4), np.uint8), connectivity=bad)
        with pytest.raises(ValueError):
            kimimaro_amd.voxel_connectivity_graph_chunked(np.ones((4, 4, 4), np.uint8), (2, 2, 2), connectivity=bad)
    if torch.cuda.is_available():
        return
    lab = np.ones((8, 8, 8), np.uint8)
    g = np.zeros((8, 8, 8), np.uint32)
    with pytest.raises(kimimaro_amd.HipUnavailableError):
        skeletonize_graph_chunked(lab, (4, 4, 4), voxel_graph=g)
    with pytest.raises(kimimaro_amd.HipUnavailableError):
        skeletonize_graph_chunked(lab, (4, 4, 4), supervoxels=lab)
    with pytest.raises(kimimaro_amd.HipUnavailableError):
        skeletonize_graph_chunked(lab, (4, 4, 4), supervoxels=lab, _skeletonize=oracle_run, _postprocess=host_postprocess)
    with pytest.raises(kimimaro_amd.HipUnavailableError):
        kimimaro_amd.voxel_connectivity_graph(lab)
    with pytest.raises(kimimaro_amd.HipUnavailableError):
        kimimaro_amd.voxel_connectivity_graph_chunked(lab, (4, 4, 4))
