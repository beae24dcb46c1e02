"""The whole-volume utility kernels of csrc/points.hip, csrc/feature.hip and csrc/ccl.hip PAST the caps of their grids, where a block
walks several tiles, a thread strides or a wave takes a second piece (tests/caps_ref.py names the caps; tests/test_caps_ref_host.py
holds them against the sources).  Integers are compared exactly and floats as bit patterns; outputs handed over through the C ABI
lie between guard words; every case first asserts that it is past its cap."""
import functools

import numpy as np
import pytest

import caps_ref as R
import fill_ref
import points_ref
from test_gpu_fill_holes import assert_region_graph
from test_gpu_prep import Out

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from kimimaro_amd import ops
    return ops.engine()


def words(eng, a):
    """u32 host words -> int32 device tensor"""
    return eng.torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).to(eng.device)


def call(eng, rc):
    from kimimaro_amd import _abi
    _abi.check(rc)
    eng.sync()


# ---------------------------------------------------------------------------------------------------------------- points.hip
@pytest.mark.parametrize("dtype", [np.uint16, np.uint64], ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("shape", R.NEAREST_SHAPES, ids=str)
def test_nearest_label_voxels_blocks_walk_several_tiles(eng, shape, dtype):
    from kimimaro_amd import points
    ntiles, grid, per_block, empty = R.nearest_launch(shape)
    assert ntiles > R.NEAREST_BLOCKS and per_block >= 2
    lab = R.banded_labels(shape, dtype)
    table, start, cen = R.nearest_queries(shape, dtype)
    got = points.nearest_label_voxels(eng, eng.to_device(lab), lab.dtype.itemsize, shape, table, start, cen)
    want = np.concatenate([R.nearest_c_index(lab, table[k], cen[start[k]:start[k + 1]]) for k in range(table.size)])
    np.testing.assert_array_equal(got, want)
    absent = int(np.flatnonzero(table == R.BAND_VALUES[np.dtype(dtype)]["ABSENT"])[0])
    assert (got[start[absent]:start[absent + 1]] == R.NONE64).all() and int((got == R.NONE64).sum()) == start[absent + 1] - start[absent]


def test_synapses_to_targets_blocks_walk_several_tiles():
    import kimimaro_amd
    shape = R.NEAREST_SHAPES[0]
    assert R.nearest_launch(shape)[2] == 2
    lab = R.banded_labels(shape, np.uint16)
    table, start, cen = R.nearest_queries(shape, np.uint16)
    synapses = {int(table[k]): [(tuple(c.tolist()), q % 3) for q, c in enumerate(cen[start[k]:start[k + 1]])] for k in range(table.size)}
    got = kimimaro_amd.synapses_to_targets(lab, synapses)
    want = points_ref.synapses_to_targets(lab, synapses)
    assert list(got.items()) == list(want.items()) and len(want) >= 8


def test_nearest_label_voxels_more_queries_than_one_pass_of_the_fill(eng):
    """one label with three voxels in three tiles, NQUERIES centroids: best_d and best_c are filled by a grid that strides"""
    from kimimaro_amd import points
    shape = R.NEAREST_SHAPES[0]
    assert R.NQUERIES > R.FILL_U64_ONE_PASS
    lab = np.zeros(shape, dtype=np.uint16, order="F")
    owned = [(1, 3, 2), (4, 60, 30), (2, 33, 58)]
    for v in owned:
        lab[v] = 9
    rows = [y + shape[1] * z for _, y, z in owned]
    assert len(set(rows)) == 3 and len({r // R.nearest_launch(shape)[2] for r in rows}) == 3       # three tiles, three blocks
    rng = np.random.default_rng(11)
    cen = rng.integers(-2 * 8, (np.array(shape) + 2) * 8, size=(R.NQUERIES, 3)) / 8.0
    got = points.nearest_label_voxels(eng, eng.to_device(lab), 2, shape, np.array([9], dtype=np.uint64),
                                      np.array([0, R.NQUERIES], dtype=np.uint32), cen)
    want = R.nearest_c_index(lab, 9, cen)
    np.testing.assert_array_equal(got, want)
    assert len(np.unique(want)) == 3


@functools.lru_cache(maxsize=None)
def sparse_big_image():
    rng = np.random.default_rng(15)
    return np.asfortranarray((rng.random(R.BIG) < 0.015).astype(np.uint8))


@pytest.mark.parametrize("connectivity", (26, 6))
def test_binary_edges_count_and_emit_stride(connectivity):
    from kimimaro_amd import ops
    assert np.prod(R.BIG) > R.EDGE_COUNT_ONE_PASS and R.tiles(R.BIG) > R.EDGE_EMIT_TILES
    image = sparse_big_image()
    got_v, got_e = ops.extract_edges_from_binary_image(image, connectivity)
    want_v, want_e = points_ref.extract_edges(image, connectivity)
    assert got_v.dtype == np.uint32 and got_e.dtype == np.uint32 and len(want_e) > 1000
    np.testing.assert_array_equal(got_v, want_v)
    np.testing.assert_array_equal(got_e, want_e)


@pytest.mark.parametrize("connectivity", (26, 6))
def test_binary_edges_rows_of_two_tiles(connectivity):
    from kimimaro_amd import ops
    shape = R.EDGE_XT2_SHAPE
    assert R.tiles(shape) == 2 * shape[1] * shape[2]
    image = np.asfortranarray((np.random.default_rng(16).random(shape) < 0.3).astype(np.uint8))
    got_v, got_e = ops.extract_edges_from_binary_image(image, connectivity)
    want_v, want_e = points_ref.extract_edges(image, connectivity)
    np.testing.assert_array_equal(got_v, want_v)
    np.testing.assert_array_equal(got_e, want_e)


# ---------------------------------------------------------------------------------------------------------------- feature.hip
def test_geodesic_seed_more_voxels_and_seeds_than_one_pass(eng):
    n = R.N1
    assert n > 2 * R.FEATURE_ONE_PASS
    lab, voxel, number, label = R.seed_case(n)
    assert (voxel >= n).sum() > 1000 and (label == 0).sum() > 1000
    want_dist, want_feature = R.seed(n, voxel, number, label, lab)
    dist, feature = Out(eng, n), Out(eng, n)
    d_lab, d_v, d_n, d_l = eng.to_device(lab), words(eng, voxel), words(eng, number), words(eng, label)
    call(eng, eng.lib.kh_geodesic_seed(eng.ptr(d_v), eng.ptr(d_n), n, eng.ptr(d_lab), 1, eng.ptr(d_l), n, dist.ptr, feature.ptr,
                                       eng.stream()))
    np.testing.assert_array_equal(dist.read(), want_dist.view(np.uint32))
    np.testing.assert_array_equal(feature.read(), want_feature)
    assert (want_dist[R.FEATURE_ONE_PASS:] == 0).sum() > 1000


def test_first_appearance_and_remap_more_chunks_than_one_pass(eng):
    n, nn = R.N1, R.APPEARANCE_NUMBERS
    assert (n + 255) // 256 > 2 * R.FEATURE_BLOCKS
    f = R.appearance_words(n)
    want = R.first_appearance(f, nn)
    first = Out(eng, nn + 1)
    d_f = Out(eng, n, init=f)
    call(eng, eng.lib.kh_first_appearance(d_f.ptr, n, nn, first.ptr, eng.stream()))
    np.testing.assert_array_equal(first.read(), want)
    np.testing.assert_array_equal(d_f.read(), f)
    lut = np.random.default_rng(17).integers(0, 1 << 32, size=nn + 1, dtype=np.uint64).astype(np.uint32)
    guarded_lut = Out(eng, nn + 1, init=lut)
    call(eng, eng.lib.kh_remap_u32(d_f.ptr, guarded_lut.ptr, nn, n, eng.stream()))
    np.testing.assert_array_equal(d_f.read(), R.remap(f, lut, nn))
    np.testing.assert_array_equal(guarded_lut.read(), lut)


def up(eng, a):
    """a host box [x, y, z] of 32-bit words -> device, Fortran order"""
    flat = np.asfortranarray(a).reshape(-1, order="F")
    return eng.torch.from_numpy(flat.view(np.int32)).to(eng.device)


@functools.lru_cache(maxsize=None)
def late_pieces():
    """the core voxels of BOX that lie in a piece a wave takes on its second trip, as a mask over the box"""
    lo, hi = R.CORE
    assert R.pieces(lo, hi)[1] > R.FEATURE_WAVES
    late = np.zeros(R.BOX, dtype=bool)
    late[tuple(slice(a, b) for a, b in zip(lo, hi))] = R.piece_of(lo, hi) >= R.FEATURE_WAVES
    assert late.sum() > 0 and late[lo[0]:hi[0], lo[1]:hi[1], hi[2] - 1].all()
    return late


def test_box_shell_diff_second_pieces(eng):
    from kimimaro_amd import feature, post
    lo, hi = R.CORE
    late = late_pieces()
    rng = np.random.default_rng(18)
    old = (rng.random(R.BOX) * 1000).astype(np.float32)
    old[rng.random(R.BOX) < 0.3] = np.inf
    # changes in second pieces only: single voxels, among them the last corner of the core and a voxel of its top layer's interior
    planted = old.copy()
    at = np.argwhere(late)[rng.choice(int(late.sum()), size=40, replace=False)]
    planted[tuple(at.T)] = (rng.random(40) * 500).astype(np.float32) + np.float32(1)
    planted[hi[0] - 1, hi[1] - 1, hi[2] - 1] = np.float32(5000.0)            # the largest finite value, in the last piece
    planted[lo[0], lo[1] + 50, hi[2] - 1] = np.float32(0.5)
    assert not (planted.view(np.uint32) != old.view(np.uint32))[~late].any()
    # and a random 1 % of the box
    spread = old.copy()
    hit = rng.random(R.BOX) < 0.01
    spread[hit] = (rng.random(int(hit.sum())) * 2000).astype(np.float32)
    for now in (planted, spread):
        want = post.shell_diff(old, now, lo, hi)
        got = feature.box_shell_diff(eng, up(eng, old), up(eng, now), R.BOX, lo, hi)
        assert got == want and want[1] > 0
    assert post.shell_diff(old, planted, lo, hi)[1] >= 41 and post.shell_diff(old, planted, lo, hi)[2] == int(np.float32(5000.0).view(np.uint32))


def test_first_appearance_box_second_pieces(eng):
    from kimimaro_amd import feature
    lo, hi = R.CORE
    late = late_pieces()
    (SX, SY), nn = R.DATASET_XY, 60
    assert R.ORIGIN[0] + R.BOX[0] <= SX and R.ORIGIN[1] + R.BOX[1] <= SY
    rng = np.random.default_rng(19)
    # runs of three along x; 0, numbers above nn and the "none" word among them; 41..60 only in second pieces, 39 and 40 nowhere
    f = rng.integers(0, 39, size=R.BOX, dtype=np.uint32)
    f = np.repeat(f[::3], 3, axis=0)[:R.BOX[0]]
    f[rng.random(R.BOX) < 0.05] = nn + 2
    f[rng.random(R.BOX) < 0.05] = R.NONE32
    only_late = late & np.repeat(rng.random(R.BOX)[::3] < 0.2, 3, axis=0)[:R.BOX[0]]
    f[only_late] = np.repeat(rng.integers(41, nn + 1, size=R.BOX, dtype=np.uint32)[::3], 3, axis=0)[:R.BOX[0]][only_late]
    f = np.asfortranarray(f)
    core = f[tuple(slice(a, b) for a, b in zip(lo, hi))]
    assert set(range(41, nn + 1)) <= set(np.unique(core).tolist()) and not np.isin(f[~late], np.arange(39, nn + 1)).any()
    d_first = feature.first_appearance_table(eng, nn)
    want = np.full(nn + 1, -1, dtype=np.int64)
    for origin in (R.ORIGIN, (0, 0, 0)):                  # the second call accumulates into what the first one left
        feature.first_appearance_box(eng, up(eng, f), R.BOX, lo, hi, origin, SX, SY, nn, d_first)
        R.first_appearance_box(f, lo, hi, origin, SX, SY, nn, want)
        np.testing.assert_array_equal(d_first.cpu().numpy(), want)
        if origin == R.ORIGIN:
            assert want[1:39].min() >= 2 ** 32 and (want[41:] >= 2 ** 32).all()
    assert want[0] == -1 and want[39] == -1 and want[40] == -1 and (want[41:] >= 0).all()


# ---------------------------------------------------------------------------------------------------------------- ccl.hip
def blocky(shape, seed, dtype=np.uint16):
    """six labels in tiles of 37 x 41 in (y, z), constant along x; 0.2 % of the voxels at x == 1 are 0: pockets no face path leaves"""
    rng = np.random.default_rng(seed)
    sx, sy, sz = shape
    coarse = rng.integers(1, 7, size=((sy + 36) // 37, (sz + 40) // 41)).astype(dtype) * dtype(11)
    plane = np.repeat(np.repeat(coarse, 37, axis=0), 41, axis=1)[:sy, :sz]
    cc = np.empty(shape, dtype=dtype, order="F")
    cc[...] = plane[None]
    cc[1][rng.random((sy, sz)) < 0.002] = 0
    return cc


@functools.lru_cache(maxsize=None)
def blocky_big():
    return blocky(R.BIG, 20)


@functools.lru_cache(maxsize=None)
def blocky_big2d():
    return blocky(R.BIG2D, 21)


def test_region_graph_past_the_tile_cap(eng):
    assert R.tiles(R.BIG) > R.CCL_TILES and np.prod(R.BIG) > R.CCL_ONE_PASS
    assert_region_graph(eng, blocky_big())


def test_region_graph_past_the_tile_cap_2d(eng):
    assert R.tiles(R.BIG2D) > R.CCL_TILES and np.prod(R.BIG2D) > R.CCL_ONE_PASS
    assert_region_graph(eng, blocky_big2d(), ndim=2)


@pytest.mark.parametrize("ndim", (3, 2))
def test_fill_all_holes_apply_strides(eng, ndim):
    cc = blocky_big() if ndim == 3 else blocky_big2d()
    assert cc.size > R.CCL_ONE_PASS
    want, want_n, _ = fill_ref.sequential(cc if ndim == 3 else cc[:, :, 0])
    d = eng.to_device(cc)
    n = eng.fill_all_holes(d, cc.dtype.itemsize, cc.shape, ndim=ndim)
    assert n == want_n and want_n > 1000
    np.testing.assert_array_equal(eng.to_host_volume(d, cc.shape, cc.dtype), want.reshape(cc.shape))


@pytest.mark.parametrize("shape,ndim", [(R.BIG2D, 2), (R.BIG, 3)], ids=["2d", "3d"])
def test_fill_voids_strides(eng, shape, ndim):
    import scipy.ndimage as ndi
    assert np.prod(shape) > R.CCL_ONE_PASS and R.tiles(shape) > R.CCL_TILES
    mask = np.asfortranarray(np.random.default_rng(22 + ndim).random(shape) < 0.7)
    want = ndi.binary_fill_holes(mask if ndim == 3 else mask[:, :, 0]).reshape(shape)
    d_out, n = eng.fill_voids(eng.to_device(mask.view(np.uint8)), shape, ndim=ndim)
    assert n == int(want.sum()) - int(mask.sum()) and n > 1000
    np.testing.assert_array_equal(eng.to_host_volume(d_out, shape, np.uint8), want.view(np.uint8))


def random_graph_words(shape, rng, keep):
    """u32 words of cc3d's layout, every one of the 26 direction bits set with probability `keep`, one way only"""
    g = np.zeros(int(np.prod(shape)), dtype=np.uint32)
    for bit in range(26):
        g |= (rng.integers(0, 256, size=g.size, dtype=np.uint8) < round(256 * keep)).astype(np.uint32) << np.uint32(bit)
    return g.reshape(shape, order="F")


@pytest.mark.parametrize("black_border", (0, 1))
def test_edt_graph_cells_stride(eng, black_border):
    sx, sy, sz = R.BIG
    n = sx * sy * sz
    assert n > R.CCL_ONE_PASS
    rng = np.random.default_rng(23 + black_border)
    lab = np.asfortranarray((rng.random(R.BIG) < 0.8).astype(np.uint16) * np.uint16(300))
    g = random_graph_words(R.BIG, rng, 0.5)
    cells = Out(eng, 8 * n, dtype=np.uint8)
    d_lab, d_g = eng.to_device(lab), eng.to_device(g)
    call(eng, eng.lib.kh_edt_graph_cells(eng.ptr(d_lab), 2, eng.ptr(d_g), sx, sy, sz, black_border, cells.ptr, eng.stream()))
    np.testing.assert_array_equal(cells.read(), R.graph_cells(lab, g, black_border).reshape(-1, order="F"))


def test_edt_graph_sample_stride(eng):
    sx, sy, sz = R.BIG
    n = sx * sy * sz
    assert n > R.CCL_ONE_PASS
    fine = np.asfortranarray(np.random.default_rng(25).random((2 * sx, 2 * sy, 2 * sz), dtype=np.float32))
    fine[::7, ::5, ::3] = np.inf
    out = Out(eng, n)
    d_fine = eng.to_device(fine)
    call(eng, eng.lib.kh_edt_graph_sample(eng.ptr(d_fine), sx, sy, sz, out.ptr, eng.stream()))
    np.testing.assert_array_equal(out.read(), R.graph_sample(fine, R.BIG).reshape(-1, order="F").view(np.uint32))


def test_ccl_graph_init_and_link_stride(eng):
    """a fifth of the voxels foreground, a fifth of the links removed: tens of thousands of components, one of tens of thousands of
    voxels"""
    import oracle as K
    assert np.prod(R.BIG) > R.CCL_ONE_PASS and R.tiles(R.BIG) > R.CCL_TILES
    rng = np.random.default_rng(26)
    lab = np.asfortranarray((rng.random(R.BIG) < 0.2).astype(np.uint16) * rng.integers(1, 4, size=R.BIG).astype(np.uint16))
    g = random_graph_words(R.BIG, rng, 0.8)
    want, n_want = K.color_connectivity_graph(lab, g)
    d_cc, n, rep = eng.ccl(lab, eng.to_device(g))
    assert n == n_want and n > 10000
    np.testing.assert_array_equal(eng.to_host_volume(d_cc, R.BIG), want)
    flat = want.reshape(-1, order="F")
    first = np.full(n + 1, flat.size, dtype=np.int64)
    np.minimum.at(first, flat, np.arange(flat.size))
    np.testing.assert_array_equal(rep[1:], first[1:])
    assert np.bincount(flat)[1:].max() > 10000
