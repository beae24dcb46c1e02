"""GPU: the point queries of csrc/points.hip and their public callers == the CPU statements of tests/points_ref.py, exactly
(DESIGN.md 3.11): ops.extract_edges_from_binary_image array for array in the canonical order, synapses_to_targets item for item in
insertion order, connect_points against the oracle composition of test_point_to_point_and_dijkstra_match_oracle."""
import functools

import numpy as np
import pytest

import points_ref as R
from shapes import random_walk_tube, voronoi_labels
from test_points_host import dyadic_synapses, edge_cases, random_image

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------------------- edges
def gpu_edge_cases():
    cases = dict(edge_cases())
    # rows that straddle the 64-lane boundary, more voxels than one block of 256
    cases["random_130x3x3_d30"] = random_image((130, 3, 3), 0.3, 1303)
    cases["random_65x67x3_d30"] = random_image((65, 67, 3), 0.3, 6567)
    cases["zeros"] = np.zeros((5, 4, 3), dtype=np.uint8, order="F")
    cases["ones_5x4x3"] = np.ones((5, 4, 3), dtype=np.uint8, order="F")
    return cases


def biggest_component(mask):
    import oracle
    cc, n = oracle.connected_components(mask)
    big = np.argmax(np.bincount(cc.ravel())[1:]) + 1
    return np.asfortranarray((cc == big).astype(np.uint8))


def assert_edges_equal(image, connectivity, reference_image=None):
    from kimimaro_amd import ops
    got_v, got_e = ops.extract_edges_from_binary_image(image, connectivity)
    want_v, want_e = R.extract_edges(image if reference_image is None else reference_image, connectivity)
    assert got_v.dtype == np.uint32 and got_e.dtype == np.uint32
    assert got_v.shape == want_v.shape and got_e.shape == want_e.shape
    np.testing.assert_array_equal(got_v, want_v)
    np.testing.assert_array_equal(got_e, want_e)
    return got_v, got_e


@pytest.mark.parametrize("connectivity", (6, 18, 26))
@pytest.mark.parametrize("name", sorted(gpu_edge_cases()))
def test_edges_equal_statement(name, connectivity):
    verts, edges = assert_edges_equal(gpu_edge_cases()[name], connectivity)
    if name == "cube3" and connectivity == 26:
        assert (len(verts), len(edges)) == (27, 158)
    if name == "corner" and connectivity == 26:
        assert (len(verts), len(edges)) == (2, 1)
    if name == "zeros":
        assert verts.shape == (0, 3) and edges.shape == (0, 2)


def test_edges_dtypes_tensor_and_2d():
    import torch
    base = random_image((33, 9, 5), 0.3, 77)
    assert_edges_equal(base.astype(bool), 26)
    assert_edges_equal(base, 26)
    signed = base.astype(np.int32) * np.random.default_rng(5).choice(np.array([-3, 7, 1 << 20], dtype=np.int32), size=base.shape)
    assert_edges_equal(signed, 26)
    assert_edges_equal(np.ascontiguousarray(signed), 18)                      # C-ordered input
    for t in (torch.from_numpy(np.ascontiguousarray(signed)).cuda(), torch.from_numpy(np.ascontiguousarray(base)).cuda().bool()):
        assert_edges_equal(t, 26, reference_image=t.cpu().numpy())
    flat = random_image((41, 23), 0.4, 78)
    verts, _ = assert_edges_equal(flat, 26)
    assert len(verts) and np.all(verts[:, 2] == 0)
    assert_edges_equal(torch.from_numpy(np.ascontiguousarray(flat)).cuda(), 26, reference_image=flat)


def thinned_walk(shape, seed, steps):
    """a random walk thinned to a path without 26-shortcuts: from every kept voxel jump to the LAST voxel of the walk that is within
    one step of it, so no two kept voxels other than consecutive ones are 26-neighbours"""
    rng = np.random.default_rng(seed)
    walk = np.clip(np.array(shape) // 2 + np.cumsum(rng.integers(-1, 2, size=(steps, 3)), axis=0), 0, np.array(shape) - 1)
    kept, i = [0], 0
    while True:
        near = np.flatnonzero(np.abs(walk[i + 1:] - walk[i]).max(axis=1) <= 1)
        if near.size == 0:
            break
        i = i + 1 + int(near[-1])
        if np.array_equal(walk[i], walk[kept[-1]]):
            break
        kept.append(i)
    return walk[kept]


def test_extract_skeleton_from_thinned_path():
    import kimimaro_amd
    path = thinned_walk((40, 30, 20), 9, 400)
    assert len(path) > 20
    image = np.zeros((40, 30, 20), dtype=bool)
    image[tuple(path.T)] = True
    assert int(image.sum()) == len(path)
    skel = kimimaro_amd.extract_skeleton_from_binary_image(image)
    assert isinstance(skel, kimimaro_amd.Skeleton)
    assert skel.vertices.shape == (len(path), 3) and skel.edges.shape == (len(path) - 1, 2)
    assert len(skel.components()) == 1
    assert set(map(tuple, skel.vertices.astype(np.int64).tolist())) == set(map(tuple, path.tolist()))


# ---------------------------------------------------------------------------------------------------------------- nearest voxel
@functools.lru_cache(maxsize=None)
def _tessellation():
    lab = voronoi_labels((37, 29, 23), 6, seed=21, pts_per_label=3, step=7.0)
    lab[0, 0, 0] = 7                                   # a label with one voxel
    return lab


def tessellation():
    """computed once; every test gets a copy of its own"""
    return _tessellation().copy(order="F")


def tie_blocks(lab):
    """-> (corner of a 2 x 2 x 2 block of one label, corner of a block whose first voxel carries ANOTHER label while (x+1, y, z) and
    (x, y, z+1) carry one: there the first voxel in C order is (x, y, z+1), the first in Fortran order (x+1, y, z))"""
    full = split = None
    for x, y, z in np.ndindex(*(np.array(lab.shape) - 1)):
        block = lab[x:x + 2, y:y + 2, z:z + 2]
        if full is None and x > 3 and np.all(block == block[0, 0, 0]):
            full = (x, y, z)
        if split is None and block[0, 0, 0] != block[1, 0, 0] and block[1, 0, 0] == block[0, 0, 1]:
            split = (x, y, z)
        if full and split:
            return full, split
    raise AssertionError("the volume has no such blocks")


def required_synapses(lab):
    """the cases the contract names, on top of centroids of the 1/8 grid (some outside the volume) for every label"""
    synapses = dyadic_synapses(lab, 31, per_label=5)
    assert 7 in synapses and int((lab == 7).sum()) == 1
    full, split = tie_blocks(lab)
    label_full, label_split = int(lab[full]), int(lab[split[0] + 1, split[1], split[2]])
    # eight-way tie at the centre of a block of one label; a tie that a Fortran tie-break gets wrong (swc labels of their own)
    synapses[label_full].append((tuple(v + 0.5 for v in full), 10))
    synapses[label_split].append((tuple(v + 0.5 for v in split), 11))
    # two centroids of one swc label that pick one voxel; two swc labels of one label that pick one voxel: the later one stays
    x, y, z = (int(v) for v in np.argwhere(lab == label_full)[17])
    synapses[label_full] += [((x + 0.125, y, z), 12), ((x, y - 0.125, z), 12), ((x, y, z + 0.25), 13), ((x - 0.125, y, z), 14)]
    synapses[5] = [((1.0, 2.0, 3.0), 1)]               # a label that does not occur
    synapses[10 ** 12] = [((1.0, 2.0, 3.0), 1)]        # ... and one that only the widest dtype can hold
    return synapses, full, split, (x, y, z)


def assert_targets_equal(volume, synapses, reference_volume=None):
    import kimimaro_amd
    got = kimimaro_amd.synapses_to_targets(volume, synapses)
    want = R.synapses_to_targets(volume if reference_volume is None else reference_volume, synapses)
    assert all(type(v) is int for key in got for v in key)
    assert list(got.items()) == list(want.items())
    return got


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.uint32, np.uint64])
def test_synapses_to_targets_equals_statement(dtype):
    base = tessellation()
    lab = np.asfortranarray(base.astype(dtype))
    assert len(np.unique(lab)) == len(np.unique(base))
    synapses, full, split, shared = required_synapses(base)
    # (labels are asked for as the dtype holds them)
    synapses = {(int(np.array(k).astype(dtype)) if k < 10 ** 6 and k != 5 else k): v for k, v in synapses.items()}
    got = assert_targets_equal(lab, synapses)
    assert got[full] == 10                                                   # the first voxel of the block in C order
    assert got[(split[0], split[1], split[2] + 1)] == 11 and (split[0] + 1, split[1], split[2]) not in got
    assert got[shared] == 14                                                 # 12 (twice), 13, then 14 claimed it
    assert list(got).count(shared) == 1 and got[(0, 0, 0)] in (0, 1, 2)
    if dtype == np.uint32:
        assert_targets_equal(np.ascontiguousarray(lab), synapses)            # C-ordered input, same answer
        assert_targets_equal(lab[..., np.newaxis], synapses)                 # a trailing axis is dropped


def test_synapses_to_targets_tensor_and_signed():
    import torch
    base = tessellation()
    synapses, _, _, _ = required_synapses(base)
    t = torch.from_numpy(np.ascontiguousarray(base.astype(np.int32))).cuda()
    assert_targets_equal(t, synapses, reference_volume=base)
    signed = np.asfortranarray(base.astype(np.int64) - 1003)                 # negative labels, 8 bytes
    moved = {k - 1003 if k < 10 ** 6 else k: v for k, v in synapses.items()}
    assert_targets_equal(signed, moved)


def test_synapses_to_targets_labels_alternate_inside_a_wave():
    lab = np.zeros((70, 3, 3), dtype=np.uint16, order="F")
    lab[0::2], lab[1::2] = 40, 41
    rng = np.random.default_rng(8)
    # centroids of the 1/8 grid along the whole row and beyond its ends; the later label of the volume is asked for first
    synapses = {k: [(tuple((rng.integers(-16, [80 * 8, 5 * 8, 5 * 8]) / 8.0).tolist()), swc) for swc in (0, 1, 0, 2, 1, 0)]
                for k in (41, 40)}
    got = assert_targets_equal(lab, synapses)
    assert all(int(lab[key]) in (40, 41) for key in got)


def test_synapses_to_targets_random_float_centroids():
    """200 float64 centroids over 6 labels: the best and the second-best distance of every query differ by more than 1e-9 relative
    (asserted here, on the CPU), so a last-bit difference between two correct summations cannot change a winner"""
    from scipy.spatial.distance import cdist
    lab = tessellation()
    labels = [int(v) for v in np.unique(lab) if v != 7]
    assert len(labels) == 6
    rng = np.random.default_rng(2024)
    cens = rng.uniform(-4.0, np.array(lab.shape) + 4.0, size=(200, 3))
    synapses = {}
    for k, c in enumerate(cens):
        label = labels[k % 6]
        synapses.setdefault(label, []).append((tuple(c.tolist()), k % 4))
        d = np.sort(cdist(np.argwhere(lab == label), c[None])[:, 0])
        assert d[1] - d[0] > 1e-9 * d[1]
    assert_targets_equal(lab, synapses)


def test_synapses_to_targets_composes_with_skeletonize():
    import kimimaro_amd
    from scipy import ndimage
    an = (16, 16, 40)
    lab = voronoi_labels((64, 64, 48), 10, seed=5, pts_per_label=5, step=10.0, anisotropy=an)
    rng = np.random.default_rng(4)
    synapses = {}
    for label in np.unique(lab).tolist():
        comp, n = ndimage.label(lab == label, structure=np.ones((3, 3, 3)))
        sizes = np.bincount(comp.ravel())[1:]
        if sizes.max() <= 200:
            continue
        inside = np.argwhere(comp == 1 + int(np.argmax(sizes)))               # voxels of the component skeletonize() traces
        picks = inside[rng.choice(len(inside), size=3, replace=False)]
        synapses[label] = [(tuple((p + rng.integers(-3, 4, size=3) / 8.0).tolist()), 3) for p in picks]
    targets = assert_targets_equal(lab, synapses)
    assert len(targets) == 3 * len(synapses) and len(synapses) >= 5
    params = dict(kimimaro_amd.DEFAULT_TEASAR_PARAMS)
    params["const"] = 64
    skels = kimimaro_amd.skeletonize(lab, params, anisotropy=an, dust_threshold=200, fix_borders=True, progress=False,
                                     extra_targets_after=list(targets.keys()))
    for target in targets:
        voxels = np.round(skels[int(lab[target])].vertices / np.array(an, dtype=np.float32)).astype(np.int64)
        assert np.any(np.all(voxels == np.array(target), axis=1)), target


# ---------------------------------------------------------------------------------------------------------------- connect_points
@pytest.mark.parametrize("case,an", list(enumerate([(1, 1, 1), (16, 16, 40), (2, 3, 5)])))
def test_connect_points_matches_oracle_composition(case, an):
    import oracle
    import kimimaro_amd
    m = biggest_component(random_walk_tube((40, 36, 30), 8800 + case, steps=45, step=3.0, radius=(1.3, 4.0)))
    idx = np.flatnonzero(m.ravel(order="F"))
    start, end = (tuple(int(v) for v in p) for p in oracle.locs_to_pts(idx[[5, idx.size - 7]], m.shape))
    got = kimimaro_amd.connect_points(m, start, end, anisotropy=an)
    dbf = oracle.edt(m, an, black_border=True)
    dbf_max = np.max(dbf)
    dbf = oracle.zero2inf(dbf)
    daf, tgt = oracle.euclidean_distance_field(m, start, an)
    daf = oracle.inf2zero(daf)
    pdrf = oracle.compute_pdrf(dbf_max, 100000, 4, dbf, daf, daf[tgt])
    want = oracle.path_to_source(pdrf, oracle.field_distances(pdrf, end), end, start)
    np.testing.assert_array_equal(got.vertices, np.asarray(want, dtype=np.float32) * np.array(an, dtype=np.float32))
    assert got.space == "physical" and got.edges.shape[0] == len(want) - 1
    w = np.asarray(want, dtype=np.int64)
    np.testing.assert_array_equal(got.radii, dbf[w[:, 0], w[:, 1], w[:, 2]])


def test_connect_points_refuses_disconnected_and_takes_2d():
    import torch
    import kimimaro_amd
    two = np.zeros((24, 12, 10), dtype=np.uint8, order="F")
    two[2:22, 2:5, 3:6] = 1
    two[2:22, 8:11, 3:6] = 1
    message = "Cannot extract centerline from disconnected components."
    with pytest.raises(ValueError, match=message):
        kimimaro_amd.connect_points(two, (3, 3, 4), (20, 9, 4))
    with pytest.raises(ValueError, match=message):
        kimimaro_amd.connect_points(two, (0, 0, 0), (20, 9, 4))              # start is background
    inside = kimimaro_amd.connect_points(two, (3, 3, 4), (20, 3, 4), anisotropy=(2, 2, 5))
    assert inside.space == "physical" and len(inside.vertices) >= 18
    ends = {tuple(inside.vertices[0].tolist()), tuple(inside.vertices[-1].tolist())}
    assert ends == {(6.0, 6.0, 20.0), (40.0, 6.0, 20.0)}
    on_gpu = kimimaro_amd.connect_points(torch.from_numpy(np.ascontiguousarray(two)).cuda(), (3, 3, 4), (20, 3, 4), anisotropy=(2, 2, 5))
    np.testing.assert_array_equal(on_gpu.vertices, inside.vertices)

    bend = np.zeros((30, 20), dtype=bool)
    bend[2:27, 3:7] = True
    bend[23:27, 3:18] = True
    flat = kimimaro_amd.connect_points(bend, (3, 5), (25, 16), anisotropy=(4, 4, 40))
    solid = kimimaro_amd.connect_points(bend[..., np.newaxis], (3, 5, 0), (25, 16, 0), anisotropy=(4, 4, 40))
    np.testing.assert_array_equal(flat.vertices, solid.vertices)
    np.testing.assert_array_equal(flat.radii, solid.radii)
    assert flat.space == "physical" and np.all(flat.vertices[:, 2] == 0)
    assert {tuple(flat.vertices[0].tolist()), tuple(flat.vertices[-1].tolist())} == {(12.0, 20.0, 0.0), (100.0, 64.0, 0.0)}
