"""The parts of cross_sectional_area that need no GPU: moving_average, the skeleton traversals, the arguments, the
per-voxel geometry the kernel shares with the host -- and self-checks of the CPU statement the GPU tests compare against."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import section_ref  # noqa: E402


# ---- moving_average: the vectors of the reference's test (automated_test.py:530-560) ------------------------------------------

def test_moving_average_identity():
    from kimimaro_amd.utility import moving_average
    data = np.array([])
    assert moving_average(data, 1) is data
    assert moving_average(data, 2) is data
    for data in (np.ones(11, dtype=int), np.ones(12, dtype=int), np.array([1, 1, 1, 1, 1, 10, 1, 1, 1, 1, 1])):
        assert moving_average(data, 1) is data
    assert np.all(moving_average(np.ones(11, dtype=int), 2) == np.ones(11))


def test_moving_average_windows():
    from kimimaro_amd.utility import moving_average
    data = np.array([0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0])
    assert np.all(moving_average(data, 2) == np.array([0, 0.5, 1, 1, 1, 1, 1, 1, 1, 1, 0.5]))
    res = moving_average(data, 3)
    assert np.all(res == np.array([1 / 3, 1 / 3, 2 / 3, 1, 1, 1, 1, 1, 1, 1, 2 / 3]))
    assert len(res) == len(data) and res.dtype == np.float64


def test_moving_average_rejects_window_zero():
    from kimimaro_amd.utility import moving_average
    with pytest.raises(ValueError):
        moving_average(np.ones(5), 0)
    with pytest.raises(ValueError):
        moving_average(np.ones(5), -2)


def test_moving_average_two_dimensional():
    from kimimaro_amd.utility import moving_average
    rng = np.random.default_rng(3)
    data = rng.normal(size=(17, 3)).astype(np.float32)
    got = moving_average(data, 4)
    assert got.shape == data.shape and got.dtype == np.float64
    for c in range(3):
        assert np.array_equal(got[:, c], moving_average(data[:, c], 4))
    assert np.array_equal(got, section_ref.moving_average(data, 4))
    # trailing window over the symmetric extension
    ext = np.concatenate([data[:4][::-1], data]).astype(np.float64)
    want = np.stack([ext[i + 1:i + 5].mean(axis=0) for i in range(17)])
    assert np.allclose(got, want, rtol=0, atol=1e-12)


# ---- paths / branches / terminals ----------------------------------------------------------------------------------------------

def _random_tree(n, seed):
    rng = np.random.default_rng(seed)
    return np.array([[int(rng.integers(0, v)), v] for v in range(1, n)])


GRAPHS = {
    "line": (6, [[0, 1], [1, 2], [2, 3], [3, 4], [4, 5]]),
    "y": (7, [[0, 1], [1, 2], [2, 3], [3, 4], [2, 5], [5, 6]]),
    # centre 0, arms of 1, 2, 3 and 3 vertices: the two longest arms end equally far from vertex 0 -- the smaller end is the root
    "cross": (10, [[0, 1], [0, 2], [2, 3], [0, 4], [4, 5], [5, 6], [0, 7], [7, 8], [8, 9]]),
    "two components and a loner": (9, [[5, 6], [6, 7], [1, 0], [1, 2], [1, 3], [7, 8]]),
    "cycle with a tail": (6, [[0, 1], [1, 2], [2, 3], [3, 0], [2, 4], [4, 5]]),
    "random tree": (200, _random_tree(200, 11)),
}


@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_traversal_matches_statement(name):
    from kimimaro_amd import Skeleton
    n, edges = GRAPHS[name]
    edges = np.asarray(edges)
    rng = np.random.default_rng(1)
    verts = rng.integers(0, 50, size=(n, 3)).astype(np.float32)
    skel = Skeleton(verts, edges)
    assert skel.branches().tolist() == section_ref.branches(n, edges)
    assert skel.terminals().tolist() == section_ref.terminals(n, edges)
    want = section_ref.paths(n, edges)
    got = skel.paths(return_indices=True)
    assert [p.tolist() for p in got] == want
    coords = skel.paths()
    assert len(coords) == len(want)
    for c, p in zip(coords, want):
        assert np.array_equal(c, verts[p])
    # every path starts at its component's root; on a tree the paths cover every edge
    nb = section_ref.neighbours(n, edges)
    covered = set()
    for p in want:
        assert len(p) >= 2
        for a, b in zip(p, p[1:]):
            assert b in nb[a]
            covered.add((min(a, b), max(a, b)))
    roots = {}
    for p in want:
        comp = min(_component(nb, p[0]))
        assert roots.setdefault(comp, p[0]) == p[0]
    all_edges = {(min(a, b), max(a, b)) for a, b in edges.tolist()}
    if name != "cycle with a tail":
        assert covered == all_edges
    else:
        assert len(all_edges - covered) == 1          # the cycle is cut where the walk closes it


def _component(nb, start):
    seen, todo = {start}, [start]
    while todo:
        for q in nb[todo.pop()]:
            if q not in seen:
                seen.add(q)
                todo.append(q)
    return seen


def test_traversal_known_answers():
    from kimimaro_amd import Skeleton
    n, edges = GRAPHS["cross"]
    skel = Skeleton(np.zeros((n, 3)), edges)
    # hops from vertex 0: 6 and 9 are both 3 away -> root 6; the walk from 6 reaches 0 and takes 1, 2, 7 in turn
    assert [p.tolist() for p in skel.paths(return_indices=True)] == [[6, 5, 4, 0, 1], [6, 5, 4, 0, 2, 3], [6, 5, 4, 0, 7, 8, 9]]
    assert skel.branches().tolist() == [0] and skel.terminals().tolist() == [1, 3, 6, 9]
    n, edges = GRAPHS["two components and a loner"]
    skel = Skeleton(np.zeros((n, 3)), edges)
    assert [p.tolist() for p in skel.paths(return_indices=True)] == [[2, 1, 0], [2, 1, 3], [8, 7, 6, 5]]
    n, edges = GRAPHS["cycle with a tail"]
    skel = Skeleton(np.zeros((n, 3)), edges)
    assert [p.tolist() for p in skel.paths(return_indices=True)] == [[5, 4, 2, 1, 0, 3]]


# ---- the statement checks itself -----------------------------------------------------------------------------------------------

def _plane_in_box_area(normal, extent):
    """area of the plane through the origin inside the box [-extent/2, extent/2]: ONE clip of the whole box"""
    return float(section_ref.voxel_areas(normal, extent, np.zeros(1))[0])


def test_statement_union_property():
    rng = np.random.default_rng(7)
    labels = np.ones((21, 21, 21), dtype=np.uint8)
    for _ in range(50):
        n = rng.normal(size=3)
        n /= np.sqrt(n @ n)
        vox, area, contact = section_ref.section(labels, (10, 10, 10), n, (1, 1, 1), 1)
        want = _plane_in_box_area(n, (21, 21, 21))
        assert abs(area - want) <= 1e-9 * want
        assert contact != 0 and len(vox) >= 21 * 21


def test_statement_hexagon():
    labels = np.ones((21, 21, 21), dtype=np.uint8)
    n = np.ones(3) / np.sqrt(3.0)
    _, area, contact = section_ref.section(labels, (10, 10, 10), n, (1, 1, 1), 1)
    want = 3 * np.sqrt(3.0) / 4 * 21 ** 2
    assert abs(area - want) <= 1e-9 * want
    assert contact == 63


def test_kernel_geometry_on_the_host():
    """kh_host_section_voxel runs the inline functions the kernel runs: membership bit for bit, the closed-form area against the
    statement's clipped polygon (absolute error below 1e-12 of the largest face)"""
    from kimimaro_amd import _abi, build
    if not os.path.exists(_abi.LIB_PATH):
        build.build()
    L = _abi.lib()
    rng = np.random.default_rng(5)
    normals = [v / np.sqrt(v @ v) for v in rng.normal(size=(40, 3))]
    normals += [np.array(v, dtype=np.float64) for v in
                [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, -1), (0, 1, 1), (1, 1, 1), (1, -1, 1), (1, 1e-9, 0), (0, 1e-9, 1),
                 (3, 0, 0), (0.5, 0.5, 1e-7)]]
    d, h, area = C.c_double(), C.c_double(), C.c_double()
    for a in [(1, 1, 1), (4, 4, 40), (40, 4, 4), (1, 7, 3)]:
        an = np.array(a, dtype=np.float64)
        for n in normals:
            n = np.ascontiguousarray(n)
            deltas = rng.integers(-3, 4, size=(24, 3))
            want_d = section_ref.offsets(n, an, deltas)
            want_h = section_ref.half_width(n, an)
            want_area = section_ref.voxel_areas(n, an, want_d)
            for k, delta in enumerate(deltas.tolist()):
                cut = L.kh_host_section_voxel(n.ctypes.data, an.ctypes.data, delta[0], delta[1], delta[2], C.byref(d), C.byref(h),
                                              C.byref(area))
                assert d.value == want_d[k] and h.value == want_h
                assert cut == int(abs(want_d[k]) < want_h)
                if cut:
                    assert abs(area.value - want_area[k]) <= 1e-12 * max(a) ** 2


# ---- import and arguments -------------------------------------------------------------------------------------------------------

def _line_skeleton():
    from kimimaro_amd import Skeleton
    verts = np.array([[x, 1, 1] for x in range(10)])
    edges = np.array([[x, x + 1] for x in range(9)])
    return Skeleton(verts, edges, segid=1)


def test_public_names():
    import kimimaro_amd
    from kimimaro_amd import utility
    assert callable(kimimaro_amd.cross_sectional_area) and callable(kimimaro_amd.cross_sectional_area_single)
    assert utility.XS_PROP == {"id": "cross_sectional_area", "data_type": "float32", "num_components": 1}
    assert utility.XS_CONTACT_PROP == {"id": "cross_sectional_area_contacts", "data_type": "uint8", "num_components": 1}


def test_arguments_are_checked_before_the_device():
    import kimimaro_amd
    labels = np.ones((10, 3, 3), dtype=bool, order="F")
    with pytest.raises(AssertionError):
        kimimaro_amd.cross_sectional_area(labels, _line_skeleton(), step=-1)
    with pytest.raises(AssertionError):
        kimimaro_amd.cross_sectional_area(labels, _line_skeleton(), smoothing_window=0)
    with pytest.raises(AssertionError):
        kimimaro_amd.cross_sectional_area_single(labels, _line_skeleton(), step=0)
    with pytest.raises(NotImplementedError):
        kimimaro_amd.cross_sectional_area(labels, _line_skeleton(), fill_holes=True)
    with pytest.raises(NotImplementedError):
        kimimaro_amd.cross_sectional_area(labels, _line_skeleton(), visualize_section_planes=True)
    with pytest.raises(NotImplementedError):
        kimimaro_amd.cross_sectional_area_single(labels, _line_skeleton(), visualize_section_planes=True)


def test_fails_loudly_without_gpu():
    import torch
    import kimimaro_amd
    from kimimaro_amd import ops
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    labels = np.ones((10, 3, 3), dtype=bool, order="F")
    with pytest.raises(kimimaro_amd.HipUnavailableError):
        kimimaro_amd.cross_sectional_area(labels, _line_skeleton())
    with pytest.raises(kimimaro_amd.HipUnavailableError):
        kimimaro_amd.cross_sectional_area_single(labels, _line_skeleton())
    with pytest.raises(kimimaro_amd.HipUnavailableError):
        ops.cross_sectional_area(labels, (5, 1, 1), (1, 0, 0))
