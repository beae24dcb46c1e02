"""GPU: kh_part_clusters == the numpy statement of tests/cluster_ref.py, exactly; join_close_components_many(split=True) == the dense
path (split=False); groups of more than 8 192 parts, which only the split can join."""
import numpy as np
import pytest

import cluster_ref as CR
import join_ref as J
from kimimaro_amd.skeleton import Skeleton

pytestmark = pytest.mark.gpu


def device_clusters(boxes, group_start, bound2, axis=None):
    from kimimaro_amd import ops, points
    before = np.array(boxes, copy=True)
    got = points.part_clusters(ops.engine(), boxes, group_start, bound2, axis=axis)
    assert got.dtype == np.uint32 and got.shape == (len(boxes),) and np.array_equal(boxes, before)
    return got


def random_boxes(rng, n, extent, size):
    """n boxes with integer low corners in [0, extent)^3 and integer edges in [0, size]"""
    low = rng.integers(0, extent, size=(n, 3))
    return np.concatenate([low, low + rng.integers(0, size + 1, size=(n, 3))], axis=1).astype(np.float32)


def several_groups():
    """-> (boxes, group_start, bound2): groups of 1, 2, 63, 63, 0, 64, 65, 257, 257 and 1 000 parts"""
    rng = np.random.default_rng(21)
    groups, bounds = [], []
    groups.append(random_boxes(rng, 1, 10, 2))                            # a part alone
    bounds.append(4.0)
    groups.append(np.array([[0, 0, 0, 1, 1, 1], [2, 2, 2, 3, 3, 3]], dtype=np.float32))          # low = 3 < 4
    bounds.append(4.0)
    shared = random_boxes(rng, 63, 24, 2)
    groups += [shared, shared.copy()]                                      # two groups in the same space: no cluster in common
    bounds += [9.0, 9.0]
    groups.append(np.zeros((0, 6), dtype=np.float32))                      # an empty group between the others
    bounds.append(1.0)
    groups.append(np.tile(np.array([[5, 6, 7, 8, 9, 10]], dtype=np.float32), (64, 1)))          # identical boxes: one cluster
    bounds.append(0.25)
    spanning = random_boxes(rng, 65, 60, 1)
    spanning[:, 1:3] = rng.integers(0, 12, size=(65, 2))
    spanning[:, 4:6] = spanning[:, 1:3] + 1
    spanning[40] = [-5, 3, 3, 70, 4, 4]                                    # one part whose box spans every axis' whole range
    groups.append(spanning)
    bounds.append(4.0)
    groups.append(random_boxes(rng, 257, 200, 3))                          # +inf: one cluster whatever the gaps
    bounds.append(np.inf)
    apart = 4.0 * np.stack(np.unravel_index(rng.permutation(343)[:257], (7, 7, 7)), axis=1)     # unit boxes on a grid of pitch 4
    groups.append(np.concatenate([apart, apart + 1], axis=1).astype(np.float32))
    bounds.append(9.0)                                                     # every gap is 3: a bound below (not above) every gap
    groups.append(random_boxes(rng, 1000, 40, 2))
    bounds.append(5.0)
    start = np.concatenate([[0], np.cumsum([len(g) for g in groups])])
    return np.concatenate(groups), start, np.array(bounds, dtype=np.float64)


def test_clusters_equal_the_statement_on_every_axis():
    boxes, start, bound2 = several_groups()
    assert np.diff(start).tolist() == [1, 2, 63, 63, 0, 64, 65, 257, 257, 1000]
    want = CR.clusters(boxes, start, bound2)
    piece = [want[start[g]:start[g + 1]] for g in range(len(bound2))]
    # what the cases are there for, on the statement
    assert piece[1].tolist() == [1, 1]
    assert np.array_equal(piece[2] - start[2], piece[3] - start[3]) and len(CR.sizes_of(piece[2])) > 1 and CR.sizes_of(piece[2])[0] > 1
    assert (piece[5] == start[5]).all()
    assert CR.sizes_of(piece[6])[0] > 10 and len(CR.sizes_of(piece[6])) > 1      # the spanning part gathers many, not all
    assert (piece[7] == start[7]).all()
    assert np.array_equal(piece[8], np.arange(start[8], start[9]))
    sizes = CR.sizes_of(piece[9])
    assert sizes[0] > 64 and np.count_nonzero(sizes == 1) > 10 and np.count_nonzero(sizes > 1) > 10
    for axis in (None, 0, 1, 2):
        np.testing.assert_array_equal(device_clusters(boxes, start, bound2, axis=axis), want, err_msg="axis %s" % axis)


def test_the_inequality_is_strict():
    boxes = np.array([[0, 0, 0, 1, 1, 1], [4, 0, 0, 5, 1, 1], [0, 4, 0, 1, 5, 1], [0, 0, 4, 1, 1, 5]], dtype=np.float32)    # exactly 3 apart
    for axis in (0, 1, 2):
        assert device_clusters(boxes, [0, 4], [9.0], axis=axis).tolist() == [0, 1, 2, 3]
        assert device_clusters(boxes, [0, 4], [np.nextafter(9.0, np.inf)], axis=axis).tolist() == [0, 0, 0, 0]
    assert CR.clusters(boxes, [0, 4], [9.0]).tolist() == [0, 1, 2, 3]
    assert CR.clusters(boxes, [0, 4], [np.nextafter(9.0, np.inf)]).tolist() == [0, 0, 0, 0]


def chain_boxes(n, seed, broken_every=None):
    """the boxes of n two-vertex parts in a row along x, each 2 from its successor and 5 from the one after; the part at position k
    of the row has index place[k], a random permutation.  broken_every: every link of that number is 12 long instead."""
    place = np.random.default_rng(seed).permutation(n)
    k = np.arange(n)
    x = 3 * k + (0 if broken_every is None else 10 * (k // broken_every))
    boxes = np.zeros((n, 6), dtype=np.float32)
    boxes[place, 0] = x
    boxes[place, 3] = x + 1
    return boxes, place


def test_a_shuffled_chain_is_one_cluster():
    boxes, place = chain_boxes(5000, 31)
    assert np.abs(np.diff(np.argsort(place))).max() > 1000                 # neighbours in the row lie far apart in the numbering
    for axis in (0, 1):                                                    # along the row, and across it (every box spans that axis)
        got = device_clusters(boxes, [0, 5000], [6.25], axis=axis)
        assert not got.any()


def test_a_chain_with_every_97th_link_broken():
    boxes, place = chain_boxes(5000, 32, broken_every=97)
    want = np.zeros(5000, dtype=np.uint32)
    for k0 in range(0, 5000, 97):
        want[place[k0:k0 + 97]] = place[k0:k0 + 97].min()
    assert np.unique(want).size == 52
    assert np.array_equal(CR.clusters(boxes, [0, 5000], [6.25]), want)
    for axis in (None, 0, 2):
        np.testing.assert_array_equal(device_clusters(boxes, [0, 5000], [6.25], axis=axis), want)


def test_component_clusters_mirror():
    from kimimaro_amd import ops
    frags = J.parts_of(J.fragments(4, **SCATTERED))
    want = CR.clusters(CR.boxes_of([p.vertices for p in frags]), [0, len(frags)], [6.25])
    assert np.array_equal(ops.component_clusters(frags, 2.5), want)
    assert np.array_equal(ops.component_clusters([p.vertices for p in frags], 2.5), want)
    assert ops.component_clusters([], 2.5).shape == (0,)


# fragments so far apart that a group falls into several sets under a bound of a few units, yet near enough that sets of two and
# more parts occur (checked on the CPU with cluster_ref: the assertion in the test)
SCATTERED = dict(denom=1024, nfrag=40, nvert=12, extent=28, rmax=2.0)


@pytest.mark.parametrize("radius,restrict", [(np.inf, True), (3.0, False)])
def test_split_equals_the_dense_path(radius, restrict):
    from kimimaro_amd import post
    groups = [J.fragments(seed, **SCATTERED) for seed in range(4)] + [[], [J.fragments(9, **SCATTERED)[0]]]
    several = 0
    for group in groups:
        parts = J.parts_of(group)
        r = J.final_radius(parts, radius, restrict)
        cluster = CR.clusters(CR.boxes_of([p.vertices for p in parts]), [0, len(parts)], [(r + 0.000001) * (r + 0.000001)])
        several += int(np.count_nonzero(CR.sizes_of(cluster) >= 2) >= 2) if len(parts) else 0
    assert several >= 1
    dense_t, split_t, auto_t = {}, {}, {}
    dense = post.join_close_components_many(groups, radius=radius, restrict_by_radius=restrict, split=False, timings=dense_t)
    split = post.join_close_components_many(groups, radius=radius, restrict_by_radius=restrict, split=True, timings=split_t)
    auto = post.join_close_components_many(groups, radius=radius, restrict_by_radius=restrict, timings=auto_t)
    assert len(dense) == len(split) == len(auto) == len(groups)
    added = 0
    for k in range(len(groups)):
        assert J.same(split[k], dense[k]), k
        assert J.same(auto[k], dense[k]), k
        added += dense[k].edges.shape[0] - sum(p.edges.shape[0] for p in J.parts_of(groups[k]))
    assert added > 0
    assert dense_t["clusters"] == 0 and dense_t["largest_cluster"] == 0 and dense_t["cluster_ms"] == 0.0
    assert auto_t["clusters"] == 0 and auto_t["largest_cluster"] == 0          # nothing here is beyond 8 192 parts
    assert split_t["clusters"] >= 2 * several and split_t["largest_cluster"] >= 2 and split_t["cluster_ms"] > 0.0


def test_split_true_leaves_an_infinite_bound_alone():
    from kimimaro_amd import post
    groups = [J.fragments(seed, **SCATTERED) for seed in range(2)]
    timings = {}
    split = post.join_close_components_many(groups, split=True, timings=timings)
    dense = post.join_close_components_many(groups, split=False)
    assert timings["clusters"] == 0 and all(J.same(a, b) for a, b in zip(split, dense))


def pair_rows(npairs, nvert, radius=1.5):
    """2 * npairs straight parts of nvert vertices along x: part m and part npairs + m face each other across a gap of 2, the pairs
    lie on a grid of pitch 10 + 2 * nvert, far beyond twice the radius from each other.  Returns (vertices f32 [2 * npairs, nvert, 3],
    the edges u32 [npairs, 2] that join the pairs in the numbering of the concatenated parts)."""
    pitch = 10 + 2 * nvert
    m = np.arange(npairs)
    v = np.zeros((2 * npairs, nvert, 3), dtype=np.float32)
    v[:, :, 0] = np.arange(nvert)[None, :]
    v[:npairs, :, 0] += (pitch * (m % 64))[:, None]
    v[npairs:, :, 0] += (pitch * (m % 64) + nvert + 1)[:, None]
    v[:npairs, :, 1] = (pitch * (m // 64))[:, None]
    v[npairs:, :, 1] = (pitch * (m // 64))[:, None]
    # the earlier part is the tree: its last vertex to the first vertex of its partner
    joins = np.stack([nvert * m + nvert - 1, nvert * (npairs + m)], axis=1).astype(np.uint32)
    return v, joins


def paired_group():
    """8 200 two-vertex parts in 4 100 isolated near pairs, as ONE Skeleton (its components are the parts), and the joined result"""
    v, joins = pair_rows(4100, 2)
    inner = 2 * np.arange(8200, dtype=np.uint32)[:, None] + np.array([[0, 1]], dtype=np.uint32)
    radii = np.full(16400, 1.5, np.float32)
    return (Skeleton(v.reshape(-1, 3), inner, radii, segid=1),
            Skeleton(v.reshape(-1, 3), np.concatenate([inner, joins]), radii, segid=1).consolidate())


def test_a_group_of_8200_parts_in_isolated_pairs():
    """fails without the split: the group is beyond the 8 192 parts of one table"""
    from kimimaro_amd import post
    group, want = paired_group()
    timings = {}
    got = post.join_close_components_many([group], restrict_by_radius=True, timings=timings)[0]
    assert timings["largest_cluster"] == 2 and timings["clusters"] == 4100 and timings["cluster_ms"] > 0.0
    assert got.edges.shape[0] == 8200 + 4100 and J.same(got, want)        # the added edges are the 4 100 known ones
    pieces = got.components()
    assert len(pieces) == 4100 and all(p.vertices.shape[0] == 4 and p.edges.shape[0] == 3 for p in pieces)


def test_a_group_of_8200_parts_that_is_not_split_stays_an_error():
    from kimimaro_amd import post
    group, _ = paired_group()
    with pytest.raises(ValueError, match="8200 parts"):
        post.join_close_components_many([group], restrict_by_radius=True, split=False)
    with pytest.raises(ValueError, match="8200 parts"):
        post.join_close_components_many([group], split=True)           # an infinite bound: nothing to split by


def test_an_unbroken_chain_of_8193_parts_is_an_error():
    from kimimaro_amd import post
    k = np.arange(8193)
    v = np.zeros((8193, 2, 3), dtype=np.float32)          # a row of two-vertex parts, each 2 from its successor
    v[:, 0, 0] = 3 * k
    v[:, 1, 0] = 3 * k + 1
    inner = 2 * k.astype(np.uint32)[:, None] + np.array([[0, 1]], dtype=np.uint32)
    chain = Skeleton(v.reshape(-1, 3), inner, np.ones(2 * 8193, np.float32), segid=1)
    pair = Skeleton(v[:2].reshape(-1, 3), inner[:2], np.ones(4, np.float32), segid=2)
    with pytest.raises(ValueError, match=r"group 1: a cluster of 8193 parts .* bound 2\.5"):
        post.join_close_components_many([pair, chain], radius=2.5)


def test_postprocess_many_on_8200_components():
    from kimimaro_amd import post
    v, joins = pair_rows(4100, 3)
    inner = (3 * np.arange(8200, dtype=np.uint32)[:, None, None] + np.array([[0, 1], [1, 2]], dtype=np.uint32)[None]).reshape(-1, 2)
    skeleton = Skeleton(v.reshape(-1, 3), inner, np.full(24600, 1.5, np.float32), segid=77)
    got = post.postprocess_many([skeleton], dust_threshold=1.0, tick_threshold=0)        # cable length 2 each; ticks stay
    assert len(got) == 1 and got[0].id == 77
    want = Skeleton(v.reshape(-1, 3), np.concatenate([inner, joins]), np.full(24600, 1.5, np.float32), segid=77).consolidate()
    assert J.same(got[0], want)
    pieces = got[0].components()
    assert len(pieces) == 4100 and all(p.vertices.shape[0] == 6 and p.edges.shape[0] == 5 for p in pieces)
