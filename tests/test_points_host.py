"""Host tier of the point queries: the CPU statements of tests/points_ref.py against the reference's compiled
extract_edges_from_binary_image (oracle/_ref, or the goldens it made: tests/golden/binary_edges.npz) and against exact arithmetic;
the public signatures; the exits that need no GPU.

    python tests/test_points_host.py      regenerates tests/golden/binary_edges.npz from oracle/_ref
"""
import inspect
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

import points_ref as R
from shapes import voronoi_labels

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "binary_edges.npz")
CONNECTIVITIES = (6, 18, 26)
GOLDEN_CASES = ("cube3", "corner", "random_7x5x4_d50")


def random_image(shape, density, seed):
    return np.asfortranarray((np.random.default_rng(seed).random(shape) < density).astype(np.uint8))


def edge_cases():
    """name -> uint8 image: the cases of the edge contract shared by the host and the GPU tier"""
    cases = {"cube3": np.ones((3, 3, 3), dtype=np.uint8)}
    corner = np.zeros((6, 5, 4), dtype=np.uint8)
    corner[2, 2, 1] = 1                         # an isolated voxel: foreground, but no vertex
    corner[5, 4, 3] = corner[4, 3, 2] = 1       # a pair across a corner, in the last corner of the volume
    cases["corner"] = corner
    for axis in range(3):
        shape = [6, 5, 4]
        shape[axis] = 1
        cases["flat_axis%d" % axis] = random_image(tuple(shape), 0.5, 40 + axis)
    for shape in ((7, 5, 4), (70, 9, 5)):
        for density in (0.05, 0.5):
            cases["random_%dx%dx%d_d%02d" % (shape + (round(100 * density),))] = random_image(shape, density, sum(shape) + round(100 * density))
    return {k: np.asfortranarray(v) for k, v in cases.items()}


def reference_pairs(refmod, image, connectivity):
    """(coordinate pairs, vertex set) of the reference's answer: its numbering is arbitrary, the sets are not"""
    verts, edges = refmod.extract_edges_from_binary_image(np.asfortranarray(image, dtype=np.uint8), connectivity)
    verts = np.asarray(verts, dtype=np.uint32).reshape(-1, 3)
    edges = np.asarray(edges, dtype=np.uint32).reshape(-1, 2)
    assert len(np.unique(verts, axis=0)) == len(verts)
    return R.coordinate_pairs(verts, edges), set(map(tuple, verts.tolist()))


def check_against(image, connectivity, want_pairs, want_vertices=None):
    verts, edges = R.extract_edges(image, connectivity)
    assert verts.dtype == np.uint32 and edges.dtype == np.uint32 and verts.shape[1:] == (3,) and edges.shape[1:] == (2,)
    np.testing.assert_array_equal(R.coordinate_pairs(verts, edges), want_pairs)
    got_vertices = set(map(tuple, verts.tolist()))
    assert len(got_vertices) == len(verts)
    if want_vertices is None:           # (the goldens hold the pairs: the vertex set is the set of their ends)
        want_vertices = set(map(tuple, want_pairs.reshape(-1, 3).tolist()))
    assert got_vertices == want_vertices
    # the canonical order: vertices by ascending Fortran index, edges (a, b), a < b, sorted by a, then b
    shape = (tuple(image.shape) + (1, 1, 1))[:3]
    lin = verts[:, 0].astype(np.int64) + shape[0] * (verts[:, 1].astype(np.int64) + shape[1] * verts[:, 2].astype(np.int64))
    assert np.all(np.diff(lin) > 0)
    assert np.all(edges[:, 0] < edges[:, 1])
    key = edges[:, 0].astype(np.int64) * (len(verts) + 1) + edges[:, 1]
    assert np.all(np.diff(key) > 0)
    return verts, edges


@pytest.mark.ref
@pytest.mark.parametrize("connectivity", CONNECTIVITIES)
@pytest.mark.parametrize("name", sorted(edge_cases()))
def test_extract_edges_matches_compiled_reference(refmod, name, connectivity):
    image = edge_cases()[name]
    pairs, vertices = reference_pairs(refmod, image, connectivity)
    check_against(image, connectivity, pairs, vertices)


@pytest.mark.parametrize("connectivity", CONNECTIVITIES)
@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_extract_edges_matches_goldens(name, connectivity):
    """the same comparison where oracle/_ref is absent: three cases the reference answered when the goldens were made"""
    with np.load(GOLDEN) as z:
        image, pairs = z[name + "_image"], z["%s_pairs%d" % (name, connectivity)]
    np.testing.assert_array_equal(image, edge_cases()[name])
    check_against(image, connectivity, pairs)


def test_extract_edges_counts():
    verts, edges = R.extract_edges(edge_cases()["cube3"], 26)
    assert (len(verts), len(edges)) == (27, 158)
    assert len(R.extract_edges(edge_cases()["cube3"], 18)[1]) == 158 - 4 * 8        # without the 4 corner offsets x 2^3 pairs each
    assert len(R.extract_edges(edge_cases()["cube3"], 6)[1]) == 3 * 18
    verts, edges = R.extract_edges(edge_cases()["corner"], 26)
    np.testing.assert_array_equal(verts, [[4, 3, 2], [5, 4, 3]])
    np.testing.assert_array_equal(edges, [[0, 1]])
    for connectivity in (6, 18):                  # a corner pair is no pair there: nothing is left
        verts, edges = R.extract_edges(edge_cases()["corner"], connectivity)
        assert verts.shape == (0, 3) and edges.shape == (0, 2)
    verts, edges = R.extract_edges(np.zeros((4, 3), dtype=bool))
    assert verts.shape == (0, 3) and edges.shape == (0, 2)


def dyadic_synapses(labels, seed, per_label=6):
    """{label: [(centroid, swc_label), ...]} with centroids on the 1/8 grid, some of them outside the volume: every squared distance
    is then exact in float64 whatever the order of the sum, and every tie a true geometric tie"""
    rng = np.random.default_rng(seed)
    shape = np.array(labels.shape)
    synapses = {}
    for label in np.unique(labels).tolist():
        eighths = rng.integers(-3 * 8, (shape + 3) * 8, size=(per_label, 3))
        synapses[label] = [(tuple((e / 8.0).tolist()), int(rng.integers(0, 3))) for e in eighths]
    return synapses


def test_synapses_to_targets_reference_properties():
    """every key carries its label, and exact rational arithmetic finds no voxel of that label strictly nearer to a centroid than
    the voxel the centroid chose (which is the first of the nearest ones in C order)"""
    labels = voronoi_labels((13, 11, 9), 4, seed=3, pts_per_label=2, step=3.0, dtype=np.uint16)
    synapses = dyadic_synapses(labels, 11)
    targets = R.synapses_to_targets(labels, synapses)
    assert targets and all(type(v) is int for key in targets for v in key)
    swc_of = {label: {swc for _, swc in pairs} for label, pairs in synapses.items()}
    for key, swc in targets.items():
        assert swc in swc_of[int(labels[key])]
    for label, pairs in synapses.items():
        cloud = np.argwhere(labels == label)
        for centroid, swc in pairs:
            (chosen, got_swc), = R.synapses_to_targets(labels, {label: [(centroid, swc)]}).items()
            assert got_swc == swc and int(labels[chosen]) == label and chosen in targets
            c = [Fraction(v) for v in centroid]
            d2 = [sum((Fraction(int(p[k])) - c[k]) ** 2 for k in range(3)) for p in cloud]
            best = min(d2)
            assert sum((Fraction(chosen[k]) - c[k]) ** 2 for k in range(3)) == best
            assert tuple(int(v) for v in cloud[d2.index(best)]) == chosen        # argwhere lists in C order


REFERENCE_SIGNATURES = {
    # kimimaro/intake.py:706, :268-275 and kimimaro/utility.py:54 -- (name, default) in order
    "synapses_to_targets": [("labels", inspect.Parameter.empty), ("synapses", inspect.Parameter.empty), ("progress", False)],
    "connect_points": [("labels", inspect.Parameter.empty), ("start", inspect.Parameter.empty), ("end", inspect.Parameter.empty),
                       ("anisotropy", (1, 1, 1)), ("fill_holes", False), ("in_place", False), ("pdrf_scale", 100000),
                       ("pdrf_exponent", 4)],
    "extract_skeleton_from_binary_image": [("image", inspect.Parameter.empty)],
}


@pytest.mark.parametrize("name", sorted(REFERENCE_SIGNATURES))
def test_public_signatures(name):
    import kimimaro_amd
    params = inspect.signature(getattr(kimimaro_amd, name)).parameters.values()
    assert [(p.name, p.default) for p in params] == REFERENCE_SIGNATURES[name]
    assert all(p.kind == inspect.Parameter.POSITIONAL_OR_KEYWORD for p in params)


def test_early_exits_need_no_gpu(monkeypatch):
    import kimimaro_amd
    from kimimaro_amd import ops

    def no_engine():
        raise AssertionError("the GPU was asked for")
    monkeypatch.setattr(ops, "engine", no_engine)
    volume = np.ones((4, 3, 2), dtype=np.uint32)
    assert kimimaro_amd.synapses_to_targets(volume, {}) == {}
    assert kimimaro_amd.synapses_to_targets(np.ones((4, 3), dtype=np.uint32), {}) == {}
    four = np.ones((4, 3, 2, 2), dtype=np.uint8)
    with pytest.raises(kimimaro_amd.DimensionError):
        kimimaro_amd.connect_points(four, (0, 0, 0), (1, 1, 1))
    with pytest.raises(kimimaro_amd.DimensionError):
        kimimaro_amd.extract_skeleton_from_binary_image(four)
    with pytest.raises(kimimaro_amd.DimensionError):
        ops.extract_edges_from_binary_image(four)
    with pytest.raises(kimimaro_amd.DimensionError):          # not 3-D once the trailing axes are dropped
        kimimaro_amd.synapses_to_targets(np.ones((4, 3), dtype=np.uint32), {1: [((0.0, 0.0, 0.0), 1)]})
    with pytest.raises(TypeError):
        kimimaro_amd.extract_skeleton_from_binary_image(np.ones((4, 3, 2), dtype=np.float32))


def test_connectivity_follows_the_reference_comparisons():
    """skeletontricks.hpp:422-439 tests `connectivity > 6` and `connectivity > 18`"""
    from kimimaro_amd import points
    assert [points.connectivity_directions(c) for c in (6, 18, 26)] == [0x3F, 0x3FFFF, 0x3FFFFFF]
    assert points.connectivity_directions(7) == 0x3FFFF and points.connectivity_directions(19) == 0x3FFFFFF


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from oracle import build_ref
    mod = build_ref.load()
    assert mod is not None, "oracle/_ref is not available"
    out = {}
    for case in GOLDEN_CASES:
        out[case + "_image"] = edge_cases()[case]
        for conn in CONNECTIVITIES:
            out["%s_pairs%d" % (case, conn)] = reference_pairs(mod, edge_cases()[case], conn)[0].astype(np.int16)
    np.savez_compressed(GOLDEN, **out)
    print(GOLDEN, os.path.getsize(GOLDEN), "bytes")
