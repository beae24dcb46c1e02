"""DESIGN.md 3.14 without a GPU: the numpy statement (tests/join_ref.py) against the reference-made vectors of
tests/golden/post.npz and against post.join_close_components; kh_host_join_plan against the statement's plan; argument checks and
errors of the public functions."""
import ast
import ctypes as C
import os

import numpy as np
import pytest

import join_ref as J
from kimimaro_amd import _abi, build, post
from kimimaro_amd.skeleton import Skeleton
from test_post import GOLD, N, canonical

MODES = ((np.inf, False), (9.0, False), (np.inf, True))                # radius=inf, radius=9.0, restrict_by_radius=True
TIE_FREE = dict(denom=1024, nfrag=12, nvert=40, extent=24, rmax=4)
LATTICES = (dict(denom=1, nfrag=10, nvert=30, extent=12, rmax=3),
            dict(denom=1, anisotropy=(16, 16, 40), nfrag=12, nvert=40, extent=24, rmax=60))
TIE_VECTORS_AT_MOST = 1          # postprocess vectors whose join is decided by a tree_tie (vector 164 on the CPU this was written on)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_abi.LIB_PATH):
        build.build()
    return _abi.lib()


def golden_input(i):
    return Skeleton(GOLD["vin_%d" % i].copy(), GOLD["ein_%d" % i].copy(), GOLD["rin_%d" % i].copy(), segid=7)


def golden_matches(i, got):
    gv, gr, ge = canonical(got.vertices, got.edges, got.radii)
    wv, wr, we = canonical(GOLD["vout_%d" % i], GOLD["eout_%d" % i], GOLD["rout_%d" % i])
    return (gv.shape == wv.shape and np.array_equal(gv, wv) and np.array_equal(gr, wr) and ge.shape == we.shape
            and np.array_equal(ge, we))


def golden_vectors(fn):
    return [i for i in range(N) if str(GOLD["fn_%d" % i]) == fn]


def statement_postprocess(i):
    """postprocess with the statement's join -> (Skeleton, a tree_tie decided a merge)"""
    args = ast.literal_eval(str(GOLD["args_%d" % i]))
    skeleton = golden_input(i)
    skel = skeleton.consolidate(remove_disconnected_vertices=True)
    skel = post.remove_loops(post.remove_dust(skel, args[0]))
    skel, tied, _ = J.join(skel, restrict_by_radius=True)
    skel = post.remove_ticks(skel, args[1])
    skel.id = skeleton.id
    return skel.consolidate(remove_disconnected_vertices=True), tied


def test_statement_reproduces_the_join_goldens():
    vectors = golden_vectors("join_close_components")
    assert len(vectors) == 36
    for i in vectors:
        args = ast.literal_eval(str(GOLD["args_%d" % i]))
        got, _, _ = J.join(golden_input(i), radius=args[0], restrict_by_radius=args[1])
        assert golden_matches(i, got), i


def test_statement_reproduces_the_postprocess_goldens():
    vectors = golden_vectors("postprocess")
    assert len(vectors) == 46
    left_out = []
    for i in vectors:
        got, tied = statement_postprocess(i)
        if tied:
            left_out.append(i)
            continue
        assert golden_matches(i, got), i
    print("postprocess vectors left out for a tree_tie:", left_out)
    assert len(left_out) <= TIE_VECTORS_AT_MOST, left_out


@pytest.mark.parametrize("seed", range(20))
def test_statement_equals_the_host_function(seed):
    frags = J.fragments(seed, **TIE_FREE)
    for radius, restrict in MODES:
        got, _, ties = J.join(frags, radius=radius, restrict_by_radius=restrict)
        assert ties == 0, "seed %d carries a tree_tie: take another seed" % seed
        want = post.join_close_components(frags, radius=radius, restrict_by_radius=restrict)
        assert J.same(got, want), (seed, radius, restrict)


def c_plan(lib, sizes, d2, idx, radii, radius, restrict):
    sizes = np.ascontiguousarray(sizes, dtype=np.uint32)
    d2 = np.ascontiguousarray(d2, dtype=np.float64)
    idx = np.ascontiguousarray(idx, dtype=np.uint32)
    radii = np.ascontiguousarray(radii, dtype=np.float32)
    edges = np.full((max(len(sizes) - 1, 1), 2), 0xDEADBEEF, dtype=np.uint32)
    p = _abi.np_ptr
    m = lib.kh_host_join_plan(len(sizes), p(sizes), p(d2), p(idx), p(radii), float(radius), int(restrict), p(edges))
    assert m >= 0, m
    return edges[:m]


def check_plan(lib, skeletons, radius, restrict):
    parts = J.parts_of(skeletons)
    sizes, d2, idx, _, radii, r = J.tables_of(parts, radius, restrict)
    want = J.plan(sizes, d2, idx, radii, r, restrict)
    got = c_plan(lib, sizes, d2, idx, radii, r, restrict)
    assert got.shape == want.shape and np.array_equal(got, want)
    assert np.array_equal(post.join_plan(sizes, d2, idx, radii, r, restrict), want)
    return want


def test_c_plan_on_the_golden_inputs(lib):
    for i in golden_vectors("join_close_components"):
        args = ast.literal_eval(str(GOLD["args_%d" % i]))
        check_plan(lib, golden_input(i), np.inf if args[0] is None else args[0], args[1])
    for i in golden_vectors("postprocess"):
        args = ast.literal_eval(str(GOLD["args_%d" % i]))
        skel = post.remove_loops(post.remove_dust(golden_input(i).consolidate(remove_disconnected_vertices=True), args[0]))
        check_plan(lib, skel, np.inf, True)


@pytest.mark.parametrize("seed", range(20))
def test_c_plan_on_the_tie_free_inputs(lib, seed):
    frags = J.fragments(seed, **TIE_FREE)
    for radius, restrict in MODES:
        check_plan(lib, frags, radius, restrict)


@pytest.mark.parametrize("lattice", range(len(LATTICES)))
@pytest.mark.parametrize("seed", range(4))
def test_c_plan_on_integer_lattices_with_ties(lib, lattice, seed):
    frags = J.fragments(seed, **LATTICES[lattice])
    merged = 0
    for radius, restrict in MODES + ((3.0 * max(LATTICES[lattice].get("anisotropy", (1,))), False),):
        merged += len(check_plan(lib, frags, radius, restrict))
    assert merged > 0
    if lattice == 0:
        assert J.join(frags)[2] > 0                      # the unit lattice does carry tree ties (the stretched one: equal keys)


def line(x0, n, y=0.0, r=1.0):
    v = np.zeros((n, 3), dtype=np.float32)
    v[:, 0] = x0 + np.arange(n)
    v[:, 1] = y
    return Skeleton(v, np.stack([np.arange(n - 1), np.arange(1, n)], axis=1), np.full(n, r, np.float32), segid=1)


def test_c_plan_hand_cases(lib):
    # two parts
    assert np.array_equal(check_plan(lib, [line(0, 3), line(5, 2)], np.inf, False), [[2, 3]])
    # every record none: the bound is below every distance
    assert len(check_plan(lib, [line(0, 3), line(10, 3), line(20, 3)], 2.0, False)) == 0
    # two clusters that are not the fused one merge first (parts 2 and 3), then a later merge has a fused cluster of two members
    # on the query side: (0, 1) fuse at gap 2, (2, 3) at gap 1 first; then {2, 3} is the tree and {0, 1}, further back, the query
    skels = [line(0, 3), line(4, 3), line(20, 3, y=0), line(23, 3, y=0), line(40, 2)]
    edges = check_plan(lib, skels, np.inf, False)
    assert edges.tolist()[:2] == [[8, 9], [2, 3]] and len(edges) == 4
    # restrict_by_radius rejects the nearest pair (gap 2 between thin ends) and takes none; with fat radii it joins
    thin = [line(0, 3, r=0.5), line(4, 3, r=0.5)]
    thin[0].radii[0] = 3.0                               # makes the search radius 6 without fattening the facing ends
    assert len(check_plan(lib, thin, np.inf, True)) == 0
    assert np.array_equal(check_plan(lib, [line(0, 3, r=1.5), line(4, 3, r=1.5)], np.inf, True), [[2, 3]])
    # ... and rejecting the nearest pair does not fall back on a farther one of the same two parts
    far = [line(0, 3, r=0.5), line(4, 3, r=0.5)]
    far[0].radii[1] = 3.0
    far[1].radii[1] = 3.0                                # the pair (1, 1) at distance 4 would pass the test: it is not asked
    assert len(check_plan(lib, far, np.inf, True)) == 0


def test_c_plan_rejects_bad_arguments(lib):
    sizes = np.array([3, 2], dtype=np.uint32)
    d2 = np.array([[np.inf, 4.0], [4.0, np.inf]])
    idx = np.array([[[J.NONE, J.NONE], [2, 0]], [[0, 2], [J.NONE, J.NONE]]], dtype=np.uint32)
    radii = np.ones(5, dtype=np.float32)
    edges = np.zeros((1, 2), dtype=np.uint32)
    p = _abi.np_ptr
    call = lib.kh_host_join_plan
    assert call(2, p(sizes), p(d2), p(idx), p(radii), np.inf, 0, p(edges)) == 1 and edges.tolist() == [[2, 3]]
    assert call(-1, p(sizes), p(d2), p(idx), p(radii), np.inf, 0, p(edges)) < 0
    null = C.c_void_p(0)
    for k in range(5):
        args = [p(sizes), p(d2), p(idx), p(radii), p(edges)]
        args[k] = null
        assert call(2, args[0], args[1], args[2], args[3], np.inf, 0, args[4]) < 0, k
    for cell, col in (((0, 1), 0), ((0, 1), 1), ((1, 0), 0), ((1, 0), 1)):
        bad = idx.copy()
        bad[cell][col] = 3 if (cell == (0, 1)) == (col == 0) else 2       # one past its part: tree of (0, 1) is part 0 (3 vertices)
        assert call(2, p(sizes), p(d2), p(bad), p(radii), np.inf, 0, p(edges)) < 0, (cell, col)
    none = idx.copy()
    none[1, 0] = 7                                        # an index outside its part in a record that IS none does not matter
    d2n = d2.copy()
    d2n[1, 0] = np.inf
    assert call(2, p(sizes), p(d2n), p(none), p(radii), np.inf, 0, p(edges)) == 1 and edges.tolist() == [[2, 3]]


def test_public_functions_fail_without_a_gpu_and_check_the_radius_first():
    import torch
    import kimimaro_amd
    assert kimimaro_amd.join_close_components_many is post.join_close_components_many
    assert kimimaro_amd.postprocess_many is post.postprocess_many
    for radius in (0, -1.0):
        with pytest.raises(ValueError):
            post.join_close_components_many([[line(0, 3), line(5, 2)]], radius=radius)        # (before the device is asked for)
    if torch.cuda.is_available():
        return
    with pytest.raises(kimimaro_amd.HipUnavailableError):
        post.join_close_components_many([[line(0, 3), line(5, 2)]])
    with pytest.raises(kimimaro_amd.HipUnavailableError):
        post.postprocess_many([line(0, 3)])
    with pytest.raises(kimimaro_amd.HipUnavailableError):
        kimimaro_amd.ops.component_gaps([line(0, 3), line(5, 2)])
