"""DESIGN.md 3.14, the split of a group into independent clusters, without a GPU: the theorem (the edges the plan adds to a group
are the union of the edges it adds to each set of parts connected through near boxes) on the numpy statements of tests/join_ref.py
and tests/cluster_ref.py and on kh_host_join_plan; the two pure functions of post.py that regroup; the argument checks of
join_close_components_many(split=...)."""
import numpy as np
import pytest

import cluster_ref as CR
import join_ref as J
from kimimaro_amd import post
from test_join_host import c_plan, lib, line  # noqa: F401  (lib: the fixture that builds and loads the library)

CASES = 120


def lattice_case(k):
    """case k -> (parts, radius, restrict_by_radius): 4..21 random-walk fragments on the integer lattice, scattered so that they fall
    into several connected sets; even cases under restrict_by_radius, odd ones with a finite radius"""
    nparts = 4 + k % 18
    frags = J.fragments(1000 + k, nfrag=nparts + 4, nvert=6, extent=5 + nparts // 2, rmax=1.5, denom=1)
    restrict = k % 2 == 0
    parts = J.parts_of(frags)[:nparts]                    # (a walk that steps on the spot can consolidate to nothing: four spare)
    assert len(parts) == nparts
    return parts, (np.inf if restrict else 2.0), restrict


def edge_set(edges):
    return {(int(a), int(b)) for a, b in np.asarray(edges).reshape(-1, 2)}


def split_plan(parts, cluster, bound2, r, restrict, plan):
    """the edges of the per-cluster plans, through post.split_by_cluster and post.lift_edges, in the group's numbering"""
    sizes = [p.vertices.shape[0] for p in parts]
    lifted, count = set(), 0
    for members, sub in post.split_by_cluster(parts, cluster):
        d2, idx, _ = J.records([p.vertices for p in sub], bound2)
        edges = plan([p.vertices.shape[0] for p in sub], d2, idx, np.concatenate([p.radii for p in sub]), r, restrict)
        got = edge_set(post.lift_edges(edges, members, sizes))
        assert len(got) == len(edges) and not (got & lifted)
        lifted |= got
        count += len(edges)
    assert count == len(lifted)
    return lifted


def test_the_plan_of_a_group_is_the_union_of_its_clusters_plans(lib):
    several = equal_keys = merged = 0
    seen_restrict = set()
    for k in range(CASES):
        parts, radius, restrict = lattice_case(k)
        assert 4 <= len(parts) <= 21
        sizes, d2, idx, _, radii, r = J.tables_of(parts, radius, restrict)
        bound2 = (r + 0.000001) * (r + 0.000001)
        cluster = CR.clusters(CR.boxes_of([p.vertices for p in parts]), [0, len(parts)], [bound2])
        # a pair with a record is near: no record crosses two clusters
        t, q = np.nonzero(np.isfinite(d2))
        assert np.array_equal(cluster[t], cluster[q])
        whole = J.plan(sizes, d2, idx, radii, r, restrict)
        assert edge_set(c_plan(lib, sizes, d2, idx, radii, r, restrict)) == edge_set(whole)
        for plan in (J.plan, lambda *a: c_plan(lib, *a)):
            assert split_plan(parts, cluster, bound2, r, restrict, plan) == edge_set(whole), k
        several += int(np.count_nonzero(CR.sizes_of(cluster) >= 2) >= 2)
        upper = d2[np.triu_indices(len(parts), 1)]
        keys = np.sqrt(upper[np.isfinite(upper)]).astype(np.float32)
        equal_keys += int(np.unique(keys).size < keys.size)
        merged += len(whole)
        seen_restrict.add(restrict)
    print("cases with >= 2 clusters of >= 2 parts: %d, with two equal float32 keys: %d, edges: %d" % (several, equal_keys, merged))
    assert 3 * several >= CASES                           # not vacuous: the split does something in a third of the cases,
    assert 2 * equal_keys >= CASES                        # the plan has to break ties in half of them,
    assert seen_restrict == {False, True} and merged > CASES


def part(n):
    return line(0, n)


def test_split_by_cluster_hand_cases():
    parts = [part(2), part(3), part(4), part(5), part(6), part(7)]
    # ids in no ascending order of discovery (kh_part_clusters gives the smallest member, the function does not rely on it);
    # part 3 is alone
    got = post.split_by_cluster(parts, [9, 4, 9, 7, 4, 4])
    assert [m.tolist() for m, _ in got] == [[0, 2], [1, 4, 5]]
    assert all(m.dtype == np.int64 for m, _ in got)
    assert [[p.vertices.shape[0] for p in sub] for _, sub in got] == [[2, 4], [3, 6, 7]]
    assert got[0][1][1] is parts[2]
    # the ids of a later group of a call: large, and the first cluster's id is not the smallest
    got = post.split_by_cluster(parts, np.array([4000000001, 4000000000, 4000000001, 4000000000, 7, 7], dtype=np.uint32))
    assert [m.tolist() for m, _ in got] == [[0, 2], [1, 3], [4, 5]]
    # singletons only; one cluster; nothing
    assert post.split_by_cluster(parts, np.arange(6, dtype=np.uint32)) == []
    got = post.split_by_cluster(parts, np.zeros(6, dtype=np.uint32))
    assert len(got) == 1 and got[0][0].tolist() == [0, 1, 2, 3, 4, 5] and got[0][1] == parts
    assert post.split_by_cluster([], np.zeros(0, dtype=np.uint32)) == []
    with pytest.raises(ValueError):
        post.split_by_cluster(parts, [0, 0])


def test_lift_edges_hand_cases():
    sizes = [2, 3, 4, 5, 6, 7]                            # the parts start at 0, 2, 5, 9, 14, 20
    # the sub-group (1, 4, 5) numbers its vertices 0..2 | 3..8 | 9..15
    got = post.lift_edges([[0, 3], [2, 9], [8, 15], [4, 1]], [1, 4, 5], sizes)
    assert got.dtype == np.uint32 and got.tolist() == [[2, 14], [4, 20], [19, 26], [15, 3]]
    # a group that is one cluster: the identity
    edges = np.array([[0, 26], [13, 14], [1, 2]], dtype=np.uint32)
    assert np.array_equal(post.lift_edges(edges, np.arange(6), sizes), edges)
    # no edges; an empty group
    assert post.lift_edges(np.zeros((0, 2), np.uint32), [0, 2], sizes).shape == (0, 2)
    assert post.lift_edges(np.zeros((0, 2), np.uint32), [], []).shape == (0, 2)
    with pytest.raises(ValueError):
        post.lift_edges([[0, 6]], [0, 2], sizes)          # the sub-group (0, 2) has 6 vertices


def test_lift_edges_inverts_the_concatenation():
    rng = np.random.default_rng(3)
    sizes = rng.integers(1, 9, size=40)
    first = np.concatenate([[0], np.cumsum(sizes)])
    members = np.sort(rng.choice(40, size=11, replace=False))
    vertex = np.concatenate([np.arange(first[m], first[m + 1]) for m in members])     # sub-group numbering -> group numbering
    edges = rng.integers(0, vertex.size, size=(200, 2))
    assert np.array_equal(post.lift_edges(edges, members, sizes), vertex[edges])


def test_cluster_statement_hand_cases():
    unit = np.array([[0, 0, 0], [1, 1, 1]], dtype=np.float32)
    verts = [unit, unit + np.float32(4), unit + np.float32(20), unit + [np.float32(23), 20, 20]]
    boxes = CR.boxes_of(verts)
    assert boxes[1].tolist() == [4, 4, 4, 5, 5, 5]
    assert CR.low(boxes[:1], boxes[1:2])[0, 0] == 27.0 and CR.low(boxes[2:3], boxes[3:4])[0, 0] == 4.0
    assert CR.clusters(boxes, [0, 4], [4.0]).tolist() == [0, 1, 2, 3]               # strict: a pair at the bound is not near
    assert CR.clusters(boxes, [0, 4], [np.nextafter(4.0, 5.0)]).tolist() == [0, 1, 2, 2]
    assert CR.clusters(boxes, [0, 4], [28.0]).tolist() == [0, 0, 2, 2]
    assert CR.clusters(boxes, [0, 4], [np.inf]).tolist() == [0, 0, 0, 0]
    assert CR.clusters(boxes, [0, 2, 4], [np.inf, np.inf]).tolist() == [0, 0, 2, 2]  # groups are never connected
    assert CR.clusters(boxes, [0, 0, 4, 4], [1.0, np.inf, 1.0]).tolist() == [0, 0, 0, 0]


@pytest.mark.parametrize("split", [None, True, False])
def test_split_checks_the_radius_first_and_fails_without_a_gpu(split):
    import torch
    import kimimaro_amd
    for radius in (0, -1.0):
        with pytest.raises(ValueError):
            post.join_close_components_many([[line(0, 3), line(5, 2)]], radius=radius, split=split)   # (before the device is asked for)
    if torch.cuda.is_available():
        return
    with pytest.raises(kimimaro_amd.HipUnavailableError):
        post.join_close_components_many([[line(0, 3), line(5, 2)]], radius=4.0, split=split)
    with pytest.raises(kimimaro_amd.HipUnavailableError):
        kimimaro_amd.ops.component_clusters([line(0, 3), line(5, 2)], 4.0)
