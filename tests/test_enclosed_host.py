"""kh_host_enclosed_regions, which needs no GPU: hole(L) of every wanted label as lists of regions, against
tests/section_filled_ref.filled_mask on region graphs built by numpy and on hand-made graphs; the capacity protocol, the argument
checks, and that kh_host_resolve_holes, which shares the search, answers as before."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import scipy.ndimage as ndi

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fill_ref  # noqa: E402
from section_filled_ref import filled_mask  # noqa: E402

SEEDS = range(240)               # tests/test_fill_holes_host.py's


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def test_random_volumes():
    from kimimaro_amd import intake
    with_holes, shared = 0, 0
    for seed in SEEDS:
        cc = fill_ref.random_volume(seed)
        value, _, face, pairs, region = fill_ref.region_graph(cc)
        present = np.unique(cc).tolist()
        absent = max(present) + 7
        wanted = present + [absent, present[-1]]
        offsets, regions = intake.enclosed_regions(value, face, pairs, wanted)
        assert offsets.dtype == np.uint64 and regions.dtype == np.uint32
        assert offsets.shape == (len(wanted) + 1,) and offsets[0] == 0 and offsets[-1] == regions.size
        lists = [regions[int(offsets[k]):int(offsets[k + 1])] for k in range(len(wanted))]
        listed_by = {}
        for L, mine in zip(wanted, lists):
            assert np.all(mine[1:] > mine[:-1]), (seed, L)
            assert np.array_equal(np.isin(region, mine), filled_mask(cc, L) & (cc != L)), (seed, L)
            for r in mine.tolist():
                listed_by.setdefault(r, set()).add(L)
            if 1 not in cc.shape and L != absent:
                assert np.array_equal(filled_mask(cc, L), ndi.binary_fill_holes(cc == L)), (seed, L)
        assert lists[-2].size == 0                                   # the label that does not occur
        assert np.array_equal(lists[-1], lists[len(present) - 1])    # the duplicate
        with_holes += int(regions.size > 0)
        shared += int(any(len(owners) >= 2 for owners in listed_by.values()))
    print("volumes with a hole %d of %d, with a region in the holes of two labels %d" % (with_holes, len(SEEDS), shared))
    assert 3 * with_holes >= len(SEEDS)
    assert shared >= 1


def _graph(nodes, edges):
    """nodes: [(value, face)] for regions 1..; edges: pairs of region ids"""
    value = np.array([0] + [n[0] for n in nodes], dtype=np.uint64)
    face = np.array([0] + [n[1] for n in nodes], dtype=np.uint8)
    pairs = np.array([(min(a, b) << 32) | max(a, b) for a, b in edges], dtype=np.uint64)
    return value, face, pairs


def _run(nodes, edges, wanted):
    from kimimaro_amd import intake
    offsets, regions = intake.enclosed_regions(*_graph(nodes, edges), wanted)
    return [regions[int(offsets[k]):int(offsets[k + 1])].tolist() for k in range(len(wanted))]


def test_chain_in_both_id_orders():
    """outside - A - B - core: A gets {B, core}, B gets {core}, whatever the order of the ids (no dead set, no ascending rule)"""
    edges = [(1, 2), (2, 3), (3, 4)]
    assert _run([(0, 1), (1, 0), (2, 0), (3, 0)], edges, [1, 2, 3, 0]) == [[3, 4], [4], [], [2, 3, 4]]
    assert _run([(0, 1), (3, 0), (2, 0), (1, 0)], edges, [3, 2, 1]) == [[3, 4], [4], []]


def test_label_with_a_region_inside_and_one_outside():
    """label 7 has a region (3) inside label 3's hole and one outside (4, on a face) with a hole of its own (5): it is listed for
    the encloser, and its own holes are still answered"""
    nodes = [(0, 1), (3, 0), (7, 0), (7, 1), (0, 0)]
    edges = [(1, 2), (2, 3), (1, 4), (4, 5)]
    assert _run(nodes, edges, [3, 7]) == [[3], [5]]


def test_hole_bordering_two_labels_and_background():
    """a shell (label 5) around a pocket that holds labels 2 and 3 and background, mutually adjacent: all of it is 5's hole; the
    pocket's own labels enclose nothing"""
    nodes = [(0, 1), (5, 0), (2, 0), (3, 0), (0, 0)]
    edges = [(1, 2), (2, 3), (2, 4), (2, 5), (3, 4), (3, 5), (4, 5)]
    assert _run(nodes, edges, [5, 2, 3]) == [[3, 4, 5], [], []]


def test_capacity_protocol():
    from kimimaro_amd import _abi
    lib = _abi.lib()
    value, face, pairs = _graph([(0, 1), (1, 0), (2, 0), (3, 0)], [(1, 2), (2, 3), (3, 4)])
    wanted = np.array([1, 2], dtype=np.uint64)
    offsets = np.full(3, 99, dtype=np.uint64)
    call = lambda regions, cap: lib.kh_host_enclosed_regions(4, _ptr(value), _ptr(face), pairs.size, _ptr(pairs), 2, _ptr(wanted),
                                                             _ptr(offsets), regions, cap)
    assert call(None, 0) == 3                              # capacity 0: the total, the offsets
    assert offsets.tolist() == [0, 2, 3]
    regions = np.full(4, 77, dtype=np.uint32)
    assert call(_ptr(regions), 2) == 3                     # too small: nothing is written
    assert regions.tolist() == [77] * 4
    assert call(_ptr(regions), 3) == 3                     # exact: filled
    assert regions.tolist() == [3, 4, 4, 77]


def test_bad_arguments():
    from kimimaro_amd import _abi, intake
    lib = _abi.lib()
    value, face, _ = _graph([(0, 1), (1, 0)], [])
    for bad in ((1 << 32) | 3, (2 << 32) | 2, 1):
        with pytest.raises(ValueError):
            intake.enclosed_regions(value, face, np.array([bad], dtype=np.uint64), [1])
    pairs = np.array([(1 << 32) | 2], dtype=np.uint64)
    wanted = np.array([1], dtype=np.uint64)
    offsets = np.zeros(2, dtype=np.uint64)
    regions = np.zeros(4, dtype=np.uint32)
    good = [2, _ptr(value), _ptr(face), 1, _ptr(pairs), 1, _ptr(wanted), _ptr(offsets), _ptr(regions), 4]
    assert lib.kh_host_enclosed_regions(*good) == 0
    for at in (1, 2, 4, 6, 7, 8):                          # each pointer in turn
        args = list(good)
        args[at] = None
        assert lib.kh_host_enclosed_regions(*args) == -2, at
    for at in (0, 3, 5, 9):                                # each size in turn
        args = list(good)
        args[at] = -1
        assert lib.kh_host_enclosed_regions(*args) == -2, at


def test_resolver_answers_as_before():
    """the two functions share the search: a call of the new one between two calls of kh_host_resolve_holes changes nothing"""
    from kimimaro_amd import intake
    for seed in (0, 1, 2, 3, 5, 8, 13, 21, 34, 55):
        cc = fill_ref.random_volume(seed)
        value, count, face, pairs, _ = fill_ref.region_graph(cc)
        before = intake.resolve_holes(value, count, face, pairs)
        intake.enclosed_regions(value, face, pairs, np.unique(cc))
        after = intake.resolve_holes(value, count, face, pairs)
        for a, b in zip(before, after):
            assert np.array_equal(a, b), seed
