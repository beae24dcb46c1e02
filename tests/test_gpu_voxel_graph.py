"""GPU: kh_voxel_graph (csrc/graph.hip) through Engine.voxel_graph, kimimaro_amd.voxel_connectivity_graph and
voxel_connectivity_graph_chunked -- word for word the numpy statement of tests/graph_ref.py, at the shapes where the kernel changes
its path (one voxel, one past a tile of 64 x 8 x 4 on every axis, more tiles than the grid has workgroups, a pair table in LDS and one
beyond it, labels of 1, 2, 4 and 8 bytes), and accepted as they are by the consumers of a graph (the CCL, skeletonize)."""
import numpy as np
import pytest

import graph_ref as G

pytestmark = pytest.mark.gpu

MERGES = [(5, 2), (1, 2), (2, 1), (3, 3), (0, 4), (6, 7), (2, 5)]      # five pairs, unsorted, a duplicate, a self pair, a pair with 0


@pytest.fixture(scope="module")
def eng():
    from kimimaro_amd import ops
    return ops.engine()


def labels_of(case, shape, seed):
    rng = np.random.default_rng(seed)
    low = rng.integers(0, 3, size=shape)                  # 0..2: most neighbour pairs are equal
    if case == "u64":
        return np.asfortranarray(low.astype(np.uint64) + (rng.integers(0, 2, size=shape).astype(np.uint64) << np.uint64(32)))
    if case == "i32":
        return np.asfortranarray((low - 1).astype(np.int32))          # -1, 0, 1
    if case == "bool":
        return np.asfortranarray(low > 0)
    return np.asfortranarray(low.astype({"u8": np.uint8, "u16": np.uint16, "u32": np.uint32}[case]))


CASES = [((1, 1, 1), "u32"), ((3, 1, 1), "u32"), ((257, 3, 2), "u32"), ((70, 9, 5), "u16"), ((33, 40, 1), "u8"), ((24, 24, 24), "u64"),
         ((65, 9, 5), "i32"), ((19, 17, 6), "bool"), ((40, 30), "u16")]


@pytest.mark.parametrize("connectivity", [6, 18, 26])
@pytest.mark.parametrize("shape,case", CASES)
def test_kernel_is_the_numpy_statement(shape, case, connectivity):
    import kimimaro_amd
    lab = labels_of(case, shape, len(shape) + shape[0])
    if case == "u64":
        assert len(np.unique(lab)) == 6 and len(np.unique(lab.astype(np.uint32))) == 3       # labels that differ above bit 32 only
    got = kimimaro_amd.voxel_connectivity_graph(lab, connectivity)
    assert got.dtype == np.uint32 and got.shape == lab.shape and got.flags.f_contiguous
    np.testing.assert_array_equal(got, G.graph_of(lab, connectivity, None))


def test_more_tiles_than_workgroups_and_other_forms_of_the_labels(eng):
    import kimimaro_amd
    # 1 x 1 x n: a tile holds four voxels, the grid at most 2^20 workgroups -- the last tiles are a workgroup's second turn
    lab = labels_of("u8", (1, 1, (4 << 20) + 9), 3)
    np.testing.assert_array_equal(kimimaro_amd.voxel_connectivity_graph(lab), G.graph_of(lab))
    # a C-ordered array, and a tensor on the GPU indexed [x, y, z]
    lab = labels_of("u32", (70, 9, 5), 4)
    want = G.graph_of(lab)
    np.testing.assert_array_equal(kimimaro_amd.voxel_connectivity_graph(np.ascontiguousarray(lab)), want)
    tensor = eng.torch.from_numpy(np.ascontiguousarray(lab).view(np.int32)).to(eng.device)
    np.testing.assert_array_equal(kimimaro_amd.voxel_connectivity_graph(tensor, 26, [(1, 2)]), G.graph_of(lab, 26, [(1, 2)]))


@pytest.mark.parametrize("case,shape", [("u8", (33, 20, 9)), ("u32", (70, 9, 5)), ("u64", (24, 24, 24))])
def test_five_pairs(case, shape):
    import kimimaro_amd
    dtype = {"u8": np.uint8, "u32": np.uint32, "u64": np.uint64}[case]
    lab = np.asfortranarray(np.random.default_rng(5).integers(0, 8, size=shape).astype(dtype))
    for connectivity in (6, 26):
        got = kimimaro_amd.voxel_connectivity_graph(lab, connectivity, MERGES)
        np.testing.assert_array_equal(got, G.graph_of(lab, connectivity, MERGES))
    plain = G.graph_of(lab)
    listed = G.graph_of(lab, 26, MERGES)
    assert (listed != plain).any() and not (plain & ~listed).any()
    # not transitive: 1-2 and 2-5 are listed, 1-5 is not
    one_five = np.where(np.isin(lab, (1, 5)), lab, 0)
    np.testing.assert_array_equal(kimimaro_amd.voxel_connectivity_graph(one_five, 26, MERGES), G.graph_of(one_five))


def test_pairs_of_wide_and_signed_labels():
    import kimimaro_amd
    rng = np.random.default_rng(6)
    wide = np.asfortranarray(rng.integers(0, 3, size=(24, 24, 24)).astype(np.uint64) + (rng.integers(0, 2, size=(24, 24, 24)).astype(np.uint64) << np.uint64(32)))
    pairs = np.array([[(1 << 32) + 1, 1], [2, (1 << 32) + 2], [1 << 32, (1 << 32) + 1]], dtype=np.uint64)
    got = kimimaro_amd.voxel_connectivity_graph(wide, 26, pairs)
    np.testing.assert_array_equal(got, G.graph_of(wide, 26, pairs.tolist()))
    assert (got != G.graph_of(wide)).any()
    signed = np.asfortranarray(rng.integers(-2, 3, size=(20, 9, 5)).astype(np.int32))
    merges = [(-1, 2), (-2, -1), (1, -2)]
    np.testing.assert_array_equal(kimimaro_amd.voxel_connectivity_graph(signed, 26, merges), G.graph_of(signed, 26, merges))
    narrow = signed.astype(np.int8)
    np.testing.assert_array_equal(kimimaro_amd.voxel_connectivity_graph(narrow, 18, merges), G.graph_of(narrow, 18, merges))


@pytest.mark.parametrize("dtype", [np.uint16, np.uint32])
def test_a_pair_table_in_lds_and_one_beyond_it(dtype):
    import kimimaro_amd
    from kimimaro_amd import _abi, ops
    rng = np.random.default_rng(7)
    lab = np.asfortranarray(rng.integers(0, 2001, size=(40, 33, 21)).astype(dtype))
    # pairs that do occur between neighbours (so that the verdicts are not all "no"), and random ones
    seen = np.stack([lab[:-1].ravel(), lab[1:].ravel()], axis=1)[::7]
    pairs = np.concatenate([seen, rng.integers(0, 2001, size=(3000, 2))]).astype(np.int64)
    for rows in (pairs, pairs[:1500]):
        table = ops.merge_pairs(rows, (0, int(np.iinfo(dtype).max)), np.dtype(dtype).itemsize)
        assert (table.shape[0] > _abi.GRAPH_LDS_PAIRS) == (rows is pairs) and table.shape[0] > 1000
        got = kimimaro_amd.voxel_connectivity_graph(lab, 26, rows)
        want = G.graph_of(lab, 26, table.tolist())
        np.testing.assert_array_equal(got, want)
        assert np.count_nonzero(want != G.graph_of(lab)) > 500


def test_refusals(eng):
    import kimimaro_amd
    from kimimaro_amd import _abi
    lab = labels_of("u8", (9, 8, 7), 8)
    for bad in ([(1, 256)], [(-1, 2)], [1, 2], [(1, 2, 3)], [(1.0, 2.0)]):
        with pytest.raises(ValueError):
            kimimaro_amd.voxel_connectivity_graph(lab, 26, bad)
    with pytest.raises(ValueError):
        kimimaro_amd.voxel_connectivity_graph(lab > 0, 26, [(1, 2)])
    with pytest.raises(ValueError):
        kimimaro_amd.voxel_connectivity_graph(lab, 8)
    with pytest.raises(kimimaro_amd.DimensionError):
        kimimaro_amd.voxel_connectivity_graph(lab[:, 0, 0])
    assert kimimaro_amd.voxel_connectivity_graph(np.zeros((0, 4, 4), np.uint8)).shape == (0, 4, 4)
    d_lab = eng.to_device(lab)
    for itemsize, shape, connectivity in ((1, (9, 8, 7), 7), (3, (9, 8, 7), 26), (1, (0, 8, 7), 26)):
        with pytest.raises(_abi.KimiHipError):
            eng.voxel_graph(d_lab, itemsize, shape, connectivity)
    P = eng.ptr
    out = eng.empty(lab.size, eng.torch.int32)
    assert eng.lib.kh_voxel_graph(None, 1, 9, 8, 7, 26, None, 0, P(out), eng.stream()) == 1        # KH_EINVAL: no labels
    assert eng.lib.kh_voxel_graph(P(d_lab), 1, 9, 8, 7, 26, None, 0, None, eng.stream()) == 1      # ... no graph
    assert eng.lib.kh_voxel_graph(P(d_lab), 1, 9, 8, 7, 26, None, 3, P(out), eng.stream()) == 1    # ... rows without a table


def test_ccl_of_the_graph_of_the_labels_is_the_plain_ccl(eng):
    """the volume of tests/test_gpu_graph.py::test_ccl_graph_of_the_labels_is_the_plain_ccl_of_the_foreground, the graph made on the device"""
    from shapes import voronoi_labels
    lab = np.asfortranarray(voronoi_labels((48, 40, 32), 12, seed=5))
    lab[20:23] = 0
    d_graph = eng.voxel_graph(eng.to_device(lab.view("u%d" % lab.dtype.itemsize)), lab.dtype.itemsize, lab.shape)
    assert d_graph.dtype == eng.torch.int32 and d_graph.numel() == lab.size
    d_a, n_a, _ = eng.ccl(lab, d_graph)
    d_b, n_b, _ = eng.ccl(lab)
    assert n_a == n_b and n_a >= 12
    np.testing.assert_array_equal(eng.to_host_volume(d_a, lab.shape), eng.to_host_volume(d_b, lab.shape))


def test_skeletonize_takes_the_device_graph_as_it_is(eng):
    """two tubes, the first cut into two supervoxels: skeletonize(voxel_graph=the words on the device) == with the words on the host"""
    import kimimaro_amd
    from shapes import random_walk_tube
    a = random_walk_tube((56, 48, 40), 11, steps=30, step=2.6, radius=(2.5, 4.5)) != 0
    b = random_walk_tube((56, 48, 40), 12, steps=30, step=2.6, radius=(2.5, 4.5)) != 0
    lab = np.zeros(a.shape, dtype=np.uint32, order="F")
    lab[a] = 7
    lab[b & ~a] = 9
    xs = np.flatnonzero(a.any(axis=(1, 2)))
    sv = lab.copy(order="F")
    sv[int(xs[len(xs) // 2]) + 1:][lab[int(xs[len(xs) // 2]) + 1:] == 7] = 8
    params = dict(scale=3.0, const=2.0, pdrf_scale=5000, pdrf_exponent=4, soma_detection_threshold=1e9,
                  soma_acceptance_threshold=1e9, soma_invalidation_scale=1.0, soma_invalidation_const=0.0)
    kw = dict(teasar_params=params, dust_threshold=20, progress=False, _engine=eng)
    d_graph = eng.voxel_graph(eng.to_device(sv), 4, sv.shape)
    host_graph = G.graph_of(sv)
    np.testing.assert_array_equal(d_graph.cpu().numpy().view(np.uint32).reshape(sv.shape, order="F"), host_graph)
    got = kimimaro_amd.skeletonize(lab, voxel_graph=d_graph, **kw)
    want = kimimaro_amd.skeletonize(lab, voxel_graph=host_graph, **kw)
    plain = kimimaro_amd.skeletonize(lab, **kw)
    assert sorted(got) == sorted(want) and 7 in want
    for k in want:
        assert got[k] == want[k]
    assert len(want[7].components()) > len(plain[7].components())             # the wall between the supervoxels cuts the tube's skeleton
    with pytest.raises(ValueError, match="voxel_graph must have the shape of the labels"):
        kimimaro_amd.skeletonize(lab, voxel_graph=d_graph[:-1], **kw)


@pytest.mark.parametrize("shape,chunk_shape", [((50, 37, 9), (24, 16, 8)), ((40, 30), (16, 16))])
@pytest.mark.parametrize("merges", [None, MERGES])
def test_chunked_is_the_whole_volume_call(shape, chunk_shape, merges, tmp_path):
    import kimimaro_amd
    lab = np.asfortranarray(np.random.default_rng(9).integers(0, 8, size=shape).astype(np.uint16))
    whole = kimimaro_amd.voxel_connectivity_graph(lab, 26, merges)
    np.testing.assert_array_equal(whole, G.graph_of(lab, 26, merges))
    stats = {}
    got = kimimaro_amd.voxel_connectivity_graph_chunked(lab, chunk_shape, merges=merges, stats=stats)
    assert got.dtype == np.uint32 and got.shape == lab.shape and got.flags.f_contiguous
    np.testing.assert_array_equal(got, whole)
    cores = int(np.prod([-(-n // c) for n, c in zip(shape, chunk_shape)]))
    assert stats["cores"] == cores and stats["voxels_loaded"] > lab.size and stats["kernel_ms"] > 0
    assert set(stats) == {"cores", "voxels_loaded", "kernel_ms", "load_s", "store_s"}
    mm = np.memmap(str(tmp_path / "graph.bin"), dtype=np.uint32, mode="w+", shape=lab.shape, order="F")
    assert kimimaro_amd.voxel_connectivity_graph_chunked(np.ascontiguousarray(lab), chunk_shape, out=mm, merges=merges) is mm
    np.testing.assert_array_equal(np.asarray(mm), whole)
    np.testing.assert_array_equal(kimimaro_amd.voxel_connectivity_graph_chunked(lab, chunk_shape, connectivity=6, merges=merges),
                                  whole & np.uint32(0x3F))
    with pytest.raises(ValueError):
        kimimaro_amd.voxel_connectivity_graph_chunked(lab, chunk_shape, out=np.zeros(shape, np.int32))
