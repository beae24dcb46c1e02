"""The inputs of the predecessor-walk tests (csrc/backtrack.h): small, deterministic, each the smallest found that reaches one
regime of the walk.  tests/test_walk_ref_host.py proves walk_ref == oracle on every one of them without a GPU and asserts, on the
reference alone, that the case is in its regime; tests/test_gpu_walk.py runs them on the device.

Fields are (x, y, z), float32, Fortran order, built on demand; +inf = outside the object; points are (x, y, z).  A weight of 2**26
next to weights of 1 makes float-absorption plateaus: fl32(k * 2**26 + 1) == k * 2**26."""
import functools

import numpy as np

import search_cases as SC
import search_ref as R
import walk_ref as W
from voxel_graphs import random_graph

BIG = np.float32(2.0 ** 26)


def absorb():
    """ones behind a wall of 2**26: everything behind the wall lies at one distance, a plateau in three dimensions that touches
    every face of the volume but x = 0"""
    f = np.ones((12, 12, 8), dtype=np.float32, order="F")
    f[:4] = BIG
    return f


def ring():
    """a square ring of ones, one voxel thick in z, entered through a corridor of 2**26: the plateau is a closed loop, so the
    breadth-first search meets its own marks from both sides"""
    f = np.full((20, 20, 3), np.inf, dtype=np.float32, order="F")
    f[2:18, 2:18, 1] = 1
    f[5:15, 5:15, 1] = np.inf
    f[0:3, 9, 1] = BIG
    return f


def two():
    """a bar with two walls (2**26, then 2**30): two plateaus in one walk, the marks of the first must be gone before the second"""
    f = np.full((40, 5, 5), np.inf, dtype=np.float32, order="F")
    f[:, 1:4, 1:4] = 1
    f[0:3, 1:4, 1:4] = BIG
    f[20:22, 1:4, 1:4] = np.float32(2.0 ** 30)
    return f


def zslab():
    """a slab of zero weights away from the source: an exact plateau, no rounding involved"""
    f = np.ones((14, 12, 9), dtype=np.float32, order="F")
    f[7, 1:11, 1:8] = 0
    return f


def zero_source():
    """a block of zero weights around the source: the plateau at distance 0 contains the source itself, and no voxel of it has a
    strictly smaller predecessor"""
    f = np.ones((8, 8, 4), dtype=np.float32, order="F")
    f[2:6, 2:6, 1:3] = 0
    return f


def absorb_graph(symmetric):
    return lambda: random_graph((12, 12, 8), np.random.default_rng(5), 0.3, symmetric)


def rail_absorb(second):
    def make():
        f = absorb()
        f[10, 6, 4] = 0
        if second:
            f[9, 2, 2] = 0
        return f
    return make


def case(name, field, pairs, graph=None, rail=False, plateau=True, wide=False, plateaus=None):
    """pairs: (source, target) of each walk (target None: a railroad from the source).  plateau: every walk crosses one.  wide: every
    walk has a queue of more than 64 entries (a second pass of the kernel's 64-lane clean-up loop) and a route of two voxels or
    more.  plateaus: that many in every walk, exactly."""
    return dict(name=name, field=field, pairs=list(pairs), graph=graph, rail=rail, plateau=plateau, wide=wide, plateaus=plateaus)


PLATEAU_CASES = [
    case("absorb", absorb, [((0, 5, 3), (11, 11, 7)), ((0, 0, 0), (11, 0, 7))], wide=True),
    case("ring", ring, [((0, 9, 1), (17, 10, 1))], wide=True),
    case("two", two, [((0, 2, 2), (39, 3, 3))], wide=True, plateaus=2),
    case("zslab", zslab, [((0, 0, 0), (13, 11, 8))]),
    case("zero_source", zero_source, [((3, 3, 1), (7, 7, 3)), ((3, 3, 1), (5, 5, 2))]),
    case("absorb_graph_symmetric", absorb, [((0, 5, 3), (11, 11, 7))], graph=absorb_graph(True), wide=True),
    case("absorb_graph_one_way", absorb, [((0, 5, 3), (11, 11, 7))], graph=absorb_graph(False), wide=True),
]
RAIL_CASES = [
    case("rail_absorb", rail_absorb(False), [((0, 5, 3), None)], rail=True, wide=True),
    case("rail_absorb_two", rail_absorb(True), [((0, 5, 3), None)], rail=True, wide=True),
    case("rail_absorb_two_graph", rail_absorb(True), [((0, 5, 3), None)], rail=True, wide=True,
         graph=lambda: random_graph((12, 12, 8), np.random.default_rng(8), 0.3, False)),
]


def field_case(name):
    """a FIELD_CASES entry of search_cases with the two targets test_gpu_search_regimes walks to: the voxel farthest from the source
    and the last voxel (solved() turns the two words into points)"""
    make, src = SC.FIELD_CASES[name]
    return case("field_" + name, make, [(src, "farthest"), (src, "last")], plateau=False, plateaus=0)


NO_PLATEAU_CASES = [field_case(name) for name in sorted(SC.FIELD_CASES)]

WALK_CASES = PLATEAU_CASES + NO_PLATEAU_CASES          # walks to a target: kh_path_search mode 2, ops.dijkstra
ALL_CASES = WALK_CASES + RAIL_CASES
BY_NAME = {c["name"]: c for c in ALL_CASES}
assert len(BY_NAME) == len(ALL_CASES)


class Solved:
    """one walk of a case with its reference: field, graph (or None), source, dist (search_ref's fixpoint from the source), start
    and stop of the walk (start = the target, or the nearest rail; stop = the source), path (walk_ref's, start first) and stats"""

    def __init__(self, **kw):
        self.__dict__.update(kw)


@functools.lru_cache(maxsize=None)
def solved(name):
    """the walks of case `name`, computed once per process and shared (the arrays are read-only)"""
    c = BY_NAME[name]
    field = c["field"]()
    graph = c["graph"]() if c["graph"] else None
    out = []
    for src, tgt in c["pairs"]:
        dist = R.field_fixpoint(field, src, graph=graph, rails_absorb=c["rail"])
        if c["rail"]:
            start = R.point(R.nearest_rail(field, dist, src)[0], field.shape)
        elif tgt == "farthest":
            start = R.point(R.farthest(dist)[0], field.shape)
        elif tgt == "last":
            start = tuple(v - 1 for v in field.shape)
        else:
            start = tgt
        path, stats = W.walk(field, dist, start, src, rails=c["rail"], graph=graph)
        for a in (field, dist) + (() if graph is None else (graph,)):
            a.setflags(write=False)
        out.append(Solved(field=field, graph=graph, source=src, dist=dist, start=start, stop=src, path=path, stats=stats,
                          rail=c["rail"]))
    return out
