"""Which component a target, a label and a skeleton id belong to (kimimaro/intake.py:162-193, utility.py:58-83), on the HIP path.

skeletonize does two pieces of bookkeeping between the kernels and the result: every component id gets an original label, every
extra target the component it lies on.  fill_holes, fix_avocados and voxel_graph edit or redefine the components first.  These tests
use an option TOGETHER with extra targets and build graph components that span two labels, and they assert literal skeleton ids
next to GPU == oracle: product and oracle are written side by side, a rule both get wrong passes a comparison.

The two rules:
  * a target belongs to the component that holds its voxel when tracing starts -- after fill_holes (the reference's order) AND
    after the avocado pass (NOT the reference's order, which drops targets inside a pit);
  * a component is named by the label at its last run start in the x-fastest raster (skeletontricks.get_mapping).
"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


@pytest.fixture(scope="module")
def eng():
    from kimimaro_amd.engine import Engine
    return Engine()


def _both(eng, lab, **kw):
    """(product, oracle) skeletons of one call, every skeleton compared: vertices and edges bit exact, radii to 1e-4 relative"""
    import kimimaro_amd
    from oracle import pipeline as P
    from test_gpu_configs import _same
    want = P.skeletonize(lab, **kw)
    got = kimimaro_amd.skeletonize(lab, progress=False, _engine=eng, **kw)
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k].id == want[k].id == k
        _same(got[k], want[k], k)
    return got, want


@pytest.mark.parametrize("fix_borders", [False, True])
@pytest.mark.parametrize("side", ["extra_targets_before", "extra_targets_after"])
def test_avocados_with_extra_targets(eng, side, fix_borders):
    """a target inside a pit belongs to the fruit the pass merged the pit into: the points are mapped on the components the pass
    LEFT.  (Mapped before it, as the reference does, the two pit targets are vertices of no skeleton.)"""
    import kimimaro_amd
    import bookkeeping_cases as B
    from shapes import avocado_volume
    lab = avocado_volume()
    assert [int(lab[pt]) for pt in B.AVOCADO_TARGETS] == [12, 22, 41, 51]
    assert (lab[30:66, 58:61, 40:43] == 51).all() and (lab == 51).sum() == 36 * 9
    an = B.AVOCADO_AN
    kw = dict(teasar_params=B.avocado_params(kimimaro_amd.DEFAULT_TEASAR_PARAMS), anisotropy=an, dust_threshold=50,
              fix_borders=fix_borders, fix_avocados=True)
    plain, _ = _both(eng, lab, **kw)
    assert sorted(plain) == B.AVOCADO_KEYS
    assert B.holders(plain, (47, 58, 40), an) == []          # the process's corner voxel is a vertex only when it is a target
    got, want = _both(eng, lab, **kw, **{side: list(B.AVOCADO_TARGETS)})
    assert sorted(got) == sorted(want) == [11, 21, 31, 41, 51]
    for pt, key in B.AVOCADO_TARGETS.items():
        assert B.holders(got, pt, an) == [key], (pt, key)
        assert B.holders(want, pt, an) == [key], (pt, key)


@pytest.mark.parametrize("side", ["extra_targets_before", "extra_targets_after"])
def test_fill_holes_with_extra_targets(eng, side):
    """kimimaro/intake.py:168-172: the points are mapped after the fill -- a target on an island the fill swallowed belongs to the
    label around it"""
    import kimimaro_amd
    import bookkeeping_cases as B
    lab, pt = B.island_volume()
    an = B.AVOCADO_AN
    kw = dict(teasar_params=B.avocado_params(kimimaro_amd.DEFAULT_TEASAR_PARAMS), anisotropy=an, dust_threshold=50, fix_borders=True)
    got, _ = _both(eng, lab, **kw, **{side: [pt]})
    assert sorted(got) == [5, 6] and B.holders(got, pt, an) == [6]
    got, _ = _both(eng, lab, fill_holes=True, **kw)
    assert sorted(got) == [5] and B.holders(got, pt, an) == []
    got, want = _both(eng, lab, fill_holes=True, **kw, **{side: [pt]})
    assert sorted(got) == sorted(want) == [5]
    assert B.holders(got, pt, an) == [5] and B.holders(want, pt, an) == [5]


def test_fill_holes_and_avocados_with_extra_targets(eng):
    """both options: the fill runs first, then the pass, then the points are mapped"""
    import kimimaro_amd
    import bookkeeping_cases as B
    from shapes import avocado_volume
    an = B.AVOCADO_AN
    pits = {(21, 20, 22): 11, (2, 48, 24): 21}
    got, want = _both(eng, avocado_volume(), teasar_params=B.avocado_params(kimimaro_amd.DEFAULT_TEASAR_PARAMS), anisotropy=an,
                      dust_threshold=50, fix_borders=False, fill_holes=True, fix_avocados=True, extra_targets_after=list(pits))
    assert sorted(got) == sorted(want) == [11, 21, 31, 41, 51]
    for pt, key in pits.items():
        assert B.holders(got, pt, an) == [key] and B.holders(want, pt, an) == [key]


@pytest.mark.parametrize("an,fix_borders", [((1, 1, 1), True), ((16, 16, 40), False)])
def test_graph_component_that_spans_two_labels(eng, an, fix_borders):
    """one component of labels 7 and 9: its first voxel says 7, its last voxel says 7, its last run start says 9 -- and get_mapping
    (skeletontricks.pyx:490-525) reads the last run start.  With a wall: two components, one id each."""
    from kimimaro_amd import intake
    import bookkeeping_cases as B
    lab, g = B.spanning_block(wall=False)
    fg = np.flatnonzero(lab.reshape(-1, order="F"))
    assert lab.reshape(-1, order="F")[fg[0]] == 7 and lab.reshape(-1, order="F")[fg[-1]] == 7
    _, n, remap = intake.compute_cc_labels_device(eng, lab, eng.graph_to_device(g, lab.shape))
    assert n == 1 and remap == {1: 9}
    kw = dict(teasar_params=B.graph_params(an), anisotropy=an, dust_threshold=20, fix_borders=fix_borders)
    got, want = _both(eng, lab, voxel_graph=g, **kw)
    assert list(got) == list(want) == [9] and got[9].vertices.shape[0] >= 10
    lab, g = B.spanning_block(wall=True)
    _, n, remap = intake.compute_cc_labels_device(eng, lab, eng.graph_to_device(g, lab.shape))
    assert n == 2 and remap == {1: 9, 2: 7}
    got, want = _both(eng, lab, voxel_graph=g, **kw)
    assert sorted(got) == sorted(want) == [7, 9]
    assert got[9].vertices[:, 0].max() <= 11 * an[0] < 12 * an[0] <= got[7].vertices[:, 0].min()     # one id per half




# the five parametrisations of test_gpu_graph.test_ccl_graph_matches_oracle
RANDOM_CASES = [((40, 33, 21), np.uint32, 0, 0.3), ((70, 9, 5), np.uint16, 1, 0.6), ((33, 40, 1), np.uint8, 2, 0.5),
                ((300, 1, 1), np.uint32, 3, 0.4), ((24, 24, 24), np.uint64, 4, 0.9)]
_CASES = {}


def _random_case(shape, dtype, seed, drop):
    """(labels, graph, the oracle's components, their number, get_mapping's names for them): computed once per case"""
    if seed not in _CASES:
        import oracle as K
        from oracle import pipeline as P
        from voxel_graphs import random_graph
        rng = np.random.default_rng(seed)
        lab = np.asfortranarray(rng.integers(0, 3, size=shape).astype(dtype))
        g = random_graph(shape, rng, drop, symmetric=(seed % 2 == 0))
        cc, n = K.color_connectivity_graph(lab, g)
        want = {k: v for k, v in P.get_mapping(lab, cc).items() if k >= 1}
        assert sorted(want) == list(range(1, n + 1))
        _CASES[seed] = (lab, g, cc, n, want)
    return _CASES[seed]


@pytest.mark.parametrize("shape,dtype,seed,drop", RANDOM_CASES)
def test_graph_component_names_match_get_mapping(eng, shape, dtype, seed, drop):
    """random labels 0..2 under random graphs: the product's remapping equals get_mapping's on the oracle's components, entry by
    entry"""
    from kimimaro_amd import intake
    lab, g, _, n_want, want = _random_case(shape, dtype, seed, drop)
    _, n, remap = intake.compute_cc_labels_device(eng, lab, eng.graph_to_device(g, shape))
    assert n == n_want and sorted(remap) == sorted(want)
    wrong = {k: (remap[k], want[k]) for k in want if remap[k] != want[k]}
    assert not wrong, "%d of %d components misnamed (got, want), e.g. %s" % (len(wrong), n, sorted(wrong.items())[:5])


def test_random_graph_cases_tell_the_naming_rules_apart():
    """from the oracle alone: over the five cases at least 300 components whose FIRST voxel and at least 50 whose LAST voxel carry
    another label than the one get_mapping names them by -- a product on either of those rules fails above"""
    by_first = by_last = 0
    for case in RANDOM_CASES:
        lab, _, cc, n, want = _random_case(*case)
        flat_cc, flat_lab = cc.reshape(-1, order="F"), lab.reshape(-1, order="F")
        where = np.arange(flat_cc.size)
        first = np.full(n + 1, flat_cc.size, dtype=np.int64)
        last = np.full(n + 1, -1, dtype=np.int64)
        np.minimum.at(first, flat_cc, where)
        np.maximum.at(last, flat_cc, where)
        names = np.array([want[k] for k in range(1, n + 1)], dtype=np.int64)
        by_first += int((flat_lab[first[1:]].astype(np.int64) != names).sum())
        by_last += int((flat_lab[last[1:]].astype(np.int64) != names).sum())
    print("components named otherwise by their first voxel: %d, by their last voxel: %d" % (by_first, by_last))
    assert by_first >= 300 and by_last >= 50
