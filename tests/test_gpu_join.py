"""GPU: kh_part_gaps and the public functions on it == the numpy statement of tests/join_ref.py, bit for bit:
ops.component_gaps on hand-built groups whose part sizes straddle the wave (64), the workgroup and the slab (256);
join_close_components_many on several groups at once, on the reference-made vectors of tests/golden/post.npz and against
post.join_close_components on tie-free inputs; postprocess_many on the postprocess vectors."""
import ast

import numpy as np
import pytest

import join_ref as J
from kimimaro_amd.skeleton import Skeleton
from test_join_host import (GOLD, LATTICES, MODES, TIE_FREE, TIE_VECTORS_AT_MOST, golden_input, golden_matches, golden_vectors, line,
                            statement_postprocess)

pytestmark = pytest.mark.gpu


def assert_tables(vertices, bound=np.inf):
    """ops.component_gaps == the statement's records: the bits of d2 and both indices of every cell; returns the statement's"""
    from kimimaro_amd import ops
    before = [v.copy() for v in vertices]
    d2, idx = ops.component_gaps(vertices, bound=bound)
    want_d2, want_idx, tie = J.records(vertices, float(bound) * float(bound))
    n = len(vertices)
    assert d2.dtype == np.float64 and d2.shape == (n, n) and idx.dtype == np.uint32 and idx.shape == (n, n, 2)
    np.testing.assert_array_equal(d2.view(np.uint64), want_d2.view(np.uint64))
    np.testing.assert_array_equal(idx, want_idx)
    for v, b in zip(vertices, before):
        assert np.array_equal(v, b)                       # inputs are not modified
    return want_d2, want_idx, tie


def cloud(rng, n, centre, spread):
    return (np.asarray(centre, dtype=np.float64) + rng.normal(0, spread, size=(n, 3))).astype(np.float32)


def test_sizes_across_wave_workgroup_and_slab():
    rng = np.random.default_rng(11)
    sizes = (2, 3, 63, 64, 65, 255, 256, 257, 513, 1025)
    verts = [cloud(rng, n, rng.uniform(0, 40, 3), 15.0) for n in sizes]
    d2, idx, _ = assert_tables(verts)
    assert np.isfinite(d2[~np.eye(len(sizes), dtype=bool)]).all()
    # the winners are spread over the parts: lanes of every wave and slab of the big ones hold a record
    assert len({int(k) // 256 for k in idx[9, :9, 0]}) >= 3 and len({int(k) // 64 for k in idx[:9, 9, 1]}) >= 5


def test_many_two_vertex_parts():
    rng = np.random.default_rng(12)
    assert_tables([cloud(rng, 2, rng.uniform(0, 30, 3), 2.0) for _ in range(33)])
    assert_tables([cloud(rng, 2, rng.uniform(0, 30, 3), 2.0) for _ in range(33)], bound=12.0)


def test_exact_ties_across_lanes_and_slabs():
    # two parallel straight lines of 600 vertices at distance 1: every vertex has its partner at d2 = 1, 600 equal minima that
    # span three slabs and ten waves -- the record is (1, 0, 0) in both orientations, whichever side the lanes go to
    a = np.zeros((600, 3), dtype=np.float32)
    a[:, 0] = np.arange(600)
    b = a.copy()
    b[:, 1] = 1
    c = a[:300].copy()                                    # shorter: the lanes go to the long lines, ties along the walked side
    c[:, 2] = 2
    d2, idx, tie = assert_tables([a, b, c, a[::-1].copy()])
    assert d2[0, 1] == 1 and idx[0, 1].tolist() == [0, 0] and idx[1, 0].tolist() == [0, 0]
    assert idx[3, 1].tolist() == [599, 0] and idx[1, 3].tolist() == [599, 0]      # reversed line: smallest query index first
    for k in range(2):
        frags = J.fragments(k, **LATTICES[0])
        _, _, tie = assert_tables([p.vertices for p in J.parts_of(frags)])
        assert tie.any()


def test_shared_vertex():
    rng = np.random.default_rng(13)
    a, b = cloud(rng, 300, (0, 0, 0), 5.0), cloud(rng, 70, (3, 0, 0), 5.0)
    b[41] = a[277]
    d2, idx, _ = assert_tables([a, b, cloud(rng, 5, (1, 1, 1), 1.0)])
    assert d2[0, 1] == 0 and idx[0, 1].tolist() == [277, 41] and idx[1, 0].tolist() == [41, 277]


def test_large_offset_and_anisotropy():
    for seed in range(2):
        frags = J.fragments(seed, **LATTICES[1])
        verts = [p.vertices + np.float32(2 ** 20) for p in J.parts_of(frags)]
        assert_tables(verts)
        assert_tables(verts, bound=100.0)
    rng = np.random.default_rng(14)
    assert_tables([cloud(rng, n, (2 ** 20, 2 ** 20, 2 ** 20), 30.0) for n in (70, 300, 9)])


def test_finite_bound_and_box_culling():
    rng = np.random.default_rng(15)
    k = np.arange(40, dtype=np.float32)
    diagonal = np.stack([k, k, 0 * k], axis=1)                           # from (0, 0, 0) to (39, 39, 0)
    corner = cloud(rng, 30, (36, 3, 0), 1.0)                              # inside the diagonal's box, about 23 from the diagonal itself
    distant = cloud(rng, 300, (200, 200, 200), 3.0)                       # culled by its box
    close = cloud(rng, 65, (5, 7, 1), 1.0)                                # within the bound of the diagonal
    bound = 6.0
    d2, idx, _ = assert_tables([diagonal, corner, distant, close], bound=bound)
    assert np.isinf(d2[0, 1]) and np.isinf(d2[1, 0]) and np.isinf(d2[0, 2]) and np.isfinite(d2[0, 3]) and np.isfinite(d2[3, 0])
    assert (idx[0, 1] == J.NONE).all() and (idx[2, 0] == J.NONE).all()
    # the bound is exclusive: a pair at exactly the bound is none, just above it is not
    a = np.array([[0, 0, 0], [1, 0, 0]], dtype=np.float32)
    b = np.array([[4, 0, 0], [9, 0, 0]], dtype=np.float32)
    d2, _, _ = assert_tables([a, b], bound=3.0)
    assert np.isinf(d2).all()
    d2, _, _ = assert_tables([a, b], bound=np.nextafter(3.0, 4.0))
    assert d2[0, 1] == 9 and d2[1, 0] == 9


def seven_groups():
    return [J.fragments(0, **TIE_FREE), [], [line(0, 5)], [line(0, 3), line(5, 2)], J.fragments(1, **LATTICES[0]),
            J.fragments(2, **TIE_FREE)[0], J.fragments(1, **LATTICES[1])]


@pytest.mark.parametrize("mode", range(len(MODES)))
def test_several_groups_in_one_call(mode):
    from kimimaro_amd import post
    radius, restrict = MODES[mode]
    groups = seven_groups()
    got = post.join_close_components_many(groups, radius=radius, restrict_by_radius=restrict)
    assert len(got) == len(groups)
    assert got[1].empty() and got[1].vertices.shape == (0, 3)
    for k, group in enumerate(groups):
        want, _, _ = J.join(group, radius=radius, restrict_by_radius=restrict)
        assert J.same(got[k], want), k
        alone = post.join_close_components_many([group], radius=radius, restrict_by_radius=restrict)[0]
        assert J.same(got[k], alone), k                   # no record crosses groups


def test_join_goldens_replayed_in_batches():
    """the 36 join vectors, one call per distinct (radius, restrict_by_radius) of the vectors"""
    from kimimaro_amd import post
    vectors = golden_vectors("join_close_components")
    assert len(vectors) == 36
    by_args = {}
    for i in vectors:
        by_args.setdefault(str(GOLD["args_%d" % i]), []).append(i)
    for args, members in by_args.items():
        radius, restrict = ast.literal_eval(args)
        got = post.join_close_components_many([golden_input(i) for i in members], radius=radius, restrict_by_radius=restrict)
        for i, skel in zip(members, got):
            assert golden_matches(i, skel), i


def test_postprocess_goldens_replayed_in_batches():
    """the 46 postprocess vectors, one call per distinct (dust_threshold, tick_threshold); a vector whose join a tree_tie decides is
    left out, as in the host test (at most one)"""
    from kimimaro_amd import post
    vectors = golden_vectors("postprocess")
    assert len(vectors) == 46
    by_args = {}
    for i in vectors:
        by_args.setdefault(str(GOLD["args_%d" % i]), []).append(i)
    left_out = []
    for args, members in by_args.items():
        dust, tick = ast.literal_eval(args)
        got = post.postprocess_many([golden_input(i) for i in members], dust_threshold=dust, tick_threshold=tick)
        for i, skel in zip(members, got):
            want, tied = statement_postprocess(i)
            assert skel.id == 7 and J.same(skel, want), i
            if tied:
                left_out.append(i)
                continue
            assert golden_matches(i, skel), i
    assert len(left_out) <= TIE_VECTORS_AT_MOST, left_out


def test_equals_the_host_function_on_tie_free_inputs():
    from kimimaro_amd import post
    groups = [J.fragments(seed, **TIE_FREE) for seed in range(20)]
    for radius, restrict in MODES:
        got = post.join_close_components_many(groups, radius=radius, restrict_by_radius=restrict)
        for seed, group in enumerate(groups):
            want = post.join_close_components(group, radius=radius, restrict_by_radius=restrict)
            assert J.same(got[seed], want), (seed, radius, restrict)


def test_inputs_are_not_modified():
    from kimimaro_amd import post
    groups = [J.fragments(3, **TIE_FREE), J.fragments(3, **LATTICES[0])]
    before = [[s.clone() for s in g] for g in groups]
    post.join_close_components_many(groups, restrict_by_radius=True)
    post.postprocess_many([Skeleton.simple_merge(g) for g in groups], dust_threshold=0, tick_threshold=0)
    for g, b in zip(groups, before):
        for s, c in zip(g, b):
            assert J.same(s, c) and s.id == c.id
