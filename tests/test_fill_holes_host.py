"""fill_all_holes in one pass, the part that needs no GPU: the two restatements of tests/fill_ref.py agree, the host
resolver kh_host_resolve_holes agrees with them on region graphs built by numpy and on hand-made graphs, and the public function
has the reference's signature."""
import inspect
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fill_ref  # noqa: E402

SEEDS = range(240)


@pytest.fixture(scope="module")
def cases():
    """(volume, sequential's result) per seed, computed once"""
    out = []
    for seed in SEEDS:
        cc = fill_ref.random_volume(seed)
        out.append((cc, fill_ref.sequential(cc)))
    return out


def test_inputs_fill_and_swallow(cases):
    """conditions on the INPUTS, on the sequential restatement alone: enough volumes fill something, some swallow a label"""
    fills = sum(1 for _, (_, count, _) in cases if count > 0)
    swallows = sum(1 for _, (_, _, state) in cases if any(bits & fill_ref.KILLED for bits in state.values()))
    extent1 = sum(1 for cc, _ in cases if 1 in cc.shape)
    print("fills %d, swallows %d, extent-1 volumes %d of %d" % (fills, swallows, extent1, len(cases)))
    assert len(cases) >= 200
    assert 3 * fills >= len(cases)
    assert swallows >= 5
    assert extent1 >= 3


def test_static_form_equals_sequential_loop(cases):
    for seed, (cc, (want, count, state)) in zip(SEEDS, cases):
        got, got_count, got_state = fill_ref.static(cc)
        assert np.array_equal(got, want), seed
        assert got_count == count, seed
        assert got_state == state, seed


def _resolve(cc):
    from kimimaro_amd import intake
    value, count, face, pairs, region = fill_ref.region_graph(cc)
    owner, label_value, label_state, filled = intake.resolve_holes(value, count, face, pairs)
    return fill_ref.owner_volume(cc, owner, region), filled, {int(v): int(s) for v, s in zip(label_value, label_state)}


def test_host_resolver_on_numpy_region_graphs(cases):
    for seed, (cc, (want, count, state)) in zip(SEEDS, cases):
        got, got_count, got_state = _resolve(cc)
        assert np.array_equal(got, want), seed
        assert got_count == count, seed
        assert got_state == state, seed


def _graph(nodes, edges):
    """nodes: [(value, count, face)] for regions 1..; edges: pairs of region ids"""
    value = np.array([0] + [n[0] for n in nodes], dtype=np.uint64)
    count = np.array([0] + [n[1] for n in nodes], dtype=np.uint32)
    face = np.array([0] + [n[2] for n in nodes], dtype=np.uint8)
    pairs = np.array([(min(a, b) << 32) | max(a, b) for a, b in edges], dtype=np.uint64)
    return value, count, face, pairs


def _run(nodes, edges):
    from kimimaro_amd import intake
    owner, label_value, label_state, filled = intake.resolve_holes(*_graph(nodes, edges))
    return owner[1:].tolist(), filled, dict(zip(label_value.tolist(), label_state.tolist()))


P, F, K = fill_ref.PROCESSED, fill_ref.FILLED, fill_ref.KILLED


def test_chain_in_both_id_orders():
    """A contains B contains C (regions: outside 0, A, B, C of 100 / 50 / 20 / 5 voxels)"""
    edges = [(1, 2), (2, 3), (3, 4)]
    # ids ascending outwards-in: A fills B and C (25), both are dead when their turn comes
    owner, filled, state = _run([(0, 100, 1), (1, 50, 0), (2, 20, 0), (3, 5, 0)], edges)
    assert owner == [0, 0, 1, 1] and filled == 25
    assert state == {1: P | F, 2: K, 3: K}
    # ids ascending inwards-out: B fills C (5) first, then A fills B and C (25): C's voxels count twice
    owner, filled, state = _run([(0, 100, 1), (3, 50, 0), (2, 20, 0), (1, 5, 0)], edges)
    assert owner == [0, 0, 3, 3] and filled == 30
    assert state == {1: P | K, 2: P | F | K, 3: P | F}


def test_hole_with_two_adjacent_labels_and_background():
    """a shell (label 5) around a pocket that holds labels 2 and 3 and background, all three mutually adjacent: no region of the
    pocket has a single neighbour label, the pocket is closed all the same"""
    nodes = [(0, 100, 1), (5, 40, 0), (2, 4, 0), (3, 6, 0), (0, 2, 0)]
    edges = [(1, 2), (2, 3), (2, 4), (2, 5), (3, 4), (3, 5), (4, 5)]
    owner, filled, state = _run(nodes, edges)
    assert owner == [0, 0, 5, 5, 5] and filled == 12
    assert state == {2: P | K, 3: P | K, 5: P | F}        # 2 and 3 had their turn (no holes of their own) before 5 swallowed them


def test_label_with_a_region_inside_and_one_outside():
    """label 7 has a region inside label 3's hole and one outside, which has a hole of its own (background, 9 voxels): 7 is killed
    whole, the outside region keeps its id and its hole stays open"""
    nodes = [(0, 100, 1), (3, 40, 0), (7, 5, 0), (7, 30, 1), (0, 9, 0)]
    edges = [(1, 2), (2, 3), (1, 4), (4, 5)]
    owner, filled, state = _run(nodes, edges)
    assert owner == [0, 0, 3, 0, 0] and filled == 5
    assert state == {3: P | F, 7: K}
    # with the ids swapped, 3 (the two-region label) goes first and fills its own hole; 7 then swallows its inner region
    nodes = [(0, 100, 1), (7, 40, 0), (3, 5, 0), (3, 30, 1), (0, 9, 0)]
    owner, filled, state = _run(nodes, edges)
    assert owner == [0, 0, 7, 0, 3] and filled == 14
    assert state == {3: P | F | K, 7: P | F}


def test_resolver_refuses_bad_pairs():
    from kimimaro_amd import intake
    value, count, face, _ = _graph([(0, 1, 1), (1, 1, 0)], [])
    with pytest.raises(ValueError):
        intake.resolve_holes(value, count, face, np.array([(1 << 32) | 3], dtype=np.uint64))
    with pytest.raises(ValueError):
        intake.resolve_holes(value, count, face, np.array([(2 << 32) | 2], dtype=np.uint64))


def test_fill_all_holes_has_the_reference_signature():
    import torch
    import kimimaro_amd
    from kimimaro_amd import intake
    sig = inspect.signature(intake.fill_all_holes)
    assert [(p.name, p.default) for p in sig.parameters.values()] == [
        ("cc_labels", inspect.Parameter.empty), ("progress", False), ("return_fill_count", False)]
    if not torch.cuda.is_available():
        with pytest.raises(kimimaro_amd.HipUnavailableError):
            intake.fill_all_holes(np.ones((4, 4, 4), np.uint32))
