"""GPU: kimimaro_amd.skeletonize_graph_chunked on dataset 0 of tests/chunked_ref.py with a wall across one label --
equal, array for array, to the composition it is defined as (tests/graph_chunked_ref.py: per box skeletonize with the clipped slice of
the graph, placement, simple_merge().consolidate(), host postprocess), to the same composition made by the CPU oracle, to itself
whatever the lane count and whichever way the graph arrives; and the case the option exists for: a label that touches itself."""
import numpy as np
import pytest

import chunked_ref as R
import graph_chunked_ref as GR
import graph_ref as G
import join_ref as J

pytestmark = pytest.mark.gpu

CHUNKS = R.DATASETS[0][3]


@pytest.fixture(scope="module")
def eng():
    from kimimaro_amd.engine import Engine
    return Engine()


@pytest.fixture(scope="module")
def hip_run(eng):
    import kimimaro_amd
    return lambda labels, **kwargs: kimimaro_amd.skeletonize(labels, _engine=eng, progress=False, **kwargs)


def oracle_run(labels, **kwargs):
    from oracle import pipeline as P
    return P.skeletonize(labels, **kwargs)


def chunked(**kwargs):
    import kimimaro_amd
    kw = dict(teasar_params=R.TP, anisotropy=R.AN, dust_threshold=R.CHUNK_DUST, post_dust_threshold=R.POST_DUST, tick_threshold=R.TICK,
              width=2)
    kw.update(kwargs)
    return kimimaro_amd.skeletonize_graph_chunked(R.dataset(0), CHUNKS, **kw)


def supervoxels_of_the_wall():
    """(supervoxels, merges) whose graph is GR.walled_graph(): the walled label in two supervoxels that no pair joins, another label
    in two that `merges` joins again"""
    lab = R.dataset(0)
    _, label, _, at = GR.walled_graph()
    sv = lab.astype(np.uint32)
    sv[at + 1:][lab[at + 1:] == label] = label + 5000
    other = int(next(v for v in np.unique(lab) if v not in (0, label)))
    xs = np.flatnonzero((lab == other).any(axis=(1, 2)))
    mid = int(xs[len(xs) // 2])
    sv[mid:][lab[mid:] == other] = other + 5000
    return sv, [(other + 5000, other)]


@pytest.fixture(scope="module")
def driver():
    return chunked(voxel_graph=GR.walled_graph()[0])


def test_equals_its_own_composition(driver, hip_run):
    """exact.  (postprocess_many and the host postprocess agree wherever no join is decided by a tree_tie, DESIGN.md 3.14, which the
    statement of tests/join_ref.py shows first for every label, as tests/test_gpu_chunked.py does.)"""
    from kimimaro_amd import post
    frags = GR.fragments(R.dataset(0), CHUNKS, hip_run, graph=GR.walled_graph()[0])
    for label, skel in R.fused(frags).items():
        cleaned = post.remove_loops(post.remove_dust(skel.consolidate(remove_disconnected_vertices=True), R.POST_DUST))
        assert not J.join(cleaned, restrict_by_radius=True)[1], "label %d: a tree_tie decides a join" % label
    R.assert_same(driver, GR.compose(frags, post.postprocess))
    assert sum(len(f) > 1 for f in frags.values()) >= R.DATASETS[0][5]
    raw = chunked(voxel_graph=GR.walled_graph()[0], merge=False)
    assert list(raw) == list(frags)
    for label in frags:
        assert len(raw[label]) == len(frags[label]) and all(a == b for a, b in zip(raw[label], frags[label]))


def test_equals_the_oracle_made_composition(driver):
    """vertices and edges exact, radii as tests/test_gpu_chunked.py compares the two"""
    from kimimaro_amd import post
    frags = GR.fragments(R.dataset(0), CHUNKS, oracle_run, graph=GR.walled_graph()[0])
    R.assert_same(driver, GR.compose(frags, post.postprocess), radii_rtol=1e-4)


def test_lane_count_does_not_matter(driver):
    timings = {}
    R.assert_same(chunked(voxel_graph=GR.walled_graph()[0], width=1, timings=timings), driver)
    assert timings["chunks"] == R.DATASETS[0][4]


def test_both_graph_routes_give_the_same_result(driver, eng):
    """supervoxels + merges, built per box on the device by the lane that takes it == the dataset's graph cut and clipped on the host
    == that graph made by voxel_connectivity_graph_chunked, also handed over as a tensor on the GPU"""
    import kimimaro_amd
    sv, merges = supervoxels_of_the_wall()
    R.assert_same(chunked(supervoxels=sv, merges=merges), driver)
    R.assert_same(chunked(supervoxels=sv, merges=merges, width=1), driver)
    g = kimimaro_amd.voxel_connectivity_graph_chunked(sv, (48, 48, 48), merges=merges)
    np.testing.assert_array_equal(g, GR.walled_graph()[0])
    tensor = eng.torch.from_numpy(np.ascontiguousarray(g).view(np.int32)).to(eng.device)
    R.assert_same(chunked(voxel_graph=tensor), driver)


def test_the_wall_changes_the_result(driver):
    import kimimaro_amd
    label = GR.walled_graph()[1]
    plain = kimimaro_amd.skeletonize_chunked(R.dataset(0), CHUNKS, teasar_params=R.TP, anisotropy=R.AN, dust_threshold=R.CHUNK_DUST,
                                             post_dust_threshold=R.POST_DUST, tick_threshold=R.TICK, width=2)
    a, b = plain[label], driver[label]
    assert a.vertices.shape != b.vertices.shape or not np.array_equal(a.vertices, b.vertices)


U_PARAMS = {"scale": 1.5, "const": 4, "pdrf_scale": 100000, "pdrf_exponent": 4, "soma_acceptance_threshold": 3500,
            "soma_detection_threshold": 1100, "soma_invalidation_const": 300, "soma_invalidation_scale": 2}


def edges_as_steps(fragments, supervoxels):
    """[(voxel u, voxel v)] of every edge of every fragment (unit anisotropy: a vertex is its voxel)"""
    out = []
    for f in fragments:
        vox = np.rint(f.vertices).astype(np.int64)
        out += [(tuple(vox[a]), tuple(vox[b])) for a, b in f.edges.tolist()]
    return out


def test_a_label_that_touches_itself_is_not_bridged():
    """GR.u_shape(): one label whose two arms touch along a stretch, in two chunks.  With the supervoxels of the arms and the bend, and
    the arms joined to the bend only, every edge of every fragment is a step the graph allows -- none joins arm A to arm B; without
    the graph the skeleton does take the short cut (the same holds on the CPU oracle: 0 and 1 such edges when this was written)."""
    import kimimaro_amd
    lab, sv, merges = GR.u_shape()
    g = G.graph_of(sv, 26, merges)
    kw = dict(teasar_params=U_PARAMS, dust_threshold=100, merge=False, width=2)
    got = kimimaro_amd.skeletonize_graph_chunked(lab, (24, 40, 24), supervoxels=sv, merges=merges, **kw)
    assert list(got) == [7] and len(got[7]) == 2
    steps = edges_as_steps(got[7], sv)
    assert len(steps) > 60
    for u, v in steps:
        assert G.allowed_step(g, u, v) and G.allowed_step(g, v, u), (u, v)
        assert {int(sv[u]), int(sv[v])} != {1, 2}, (u, v)
    plain = kimimaro_amd.skeletonize_chunked(lab, (24, 40, 24), **kw)
    across = [(u, v) for u, v in edges_as_steps(plain[7], sv) if {int(sv[u]), int(sv[v])} == {1, 2}]
    assert across                                        # the short cut the graph forbids
    by_graph = kimimaro_amd.skeletonize_graph_chunked(lab, (24, 40, 24), voxel_graph=g, **kw)
    assert len(by_graph[7]) == 2 and all(a == b for a, b in zip(by_graph[7], got[7]))
