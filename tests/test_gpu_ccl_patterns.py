"""kh_ccl26 and kh_regions6 (csrc/ccl.hip) where the existing tests only sample them: the link rules of ccl_link_kernel and
reg_link_kernel on EVERY arrangement of two adjacent rows at the chunk boundaries 63 | 64 and 255 | 256, the numbering kernels
beyond their grid caps and the scan's batch, and labels that differ in their high bits only.  All comparisons are exact.  The inputs
and the thresholds are those of tests/dispatch_shapes.py; tests/test_dispatch_shapes_host.py checks them on the CPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dispatch_shapes as D  # noqa: E402
import fill_ref  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from kimimaro_amd.engine import Engine
    return Engine()


def _first_voxels(flat, n):
    """the smallest linear index of each of the ids 1 .. n of a volume that numbers them by first appearance in the raster (the
    oracle's numbering): an id appears where the running maximum rises"""
    top = np.maximum.accumulate(flat)
    first = np.flatnonzero(top[1:] > top[:-1]) + 1
    if flat[0]:
        first = np.concatenate([[0], first])
    assert first.size == n and np.array_equal(flat[first], np.arange(1, n + 1, dtype=flat.dtype))
    return first


def _check_ccl(eng, lab):
    """components, count and representatives against the oracle, as tests/test_gpu_ccl.py::test_ccl_matches_oracle does
    -> (the device's volume, count, the oracle's volume)"""
    import oracle
    lab = np.asfortranarray(lab)
    want, n_want = oracle.connected_components(lab)
    d_cc, n, rep = eng.ccl(lab)
    got = eng.to_host_volume(d_cc, lab.shape)
    assert n == n_want
    assert got.dtype == want.dtype == np.uint32
    if not np.array_equal(got, want):
        np.testing.assert_array_equal(got, want)
    first = _first_voxels(want.reshape(-1, order="F"), n)
    assert rep.dtype == np.uint32 and rep.shape == (n + 1,)
    np.testing.assert_array_equal(rep[1:], first.astype(np.uint32))
    return d_cc, n, want


def _check_regions(eng, cc):
    """the device's regions against numpy's partition renumbered by first appearance in the raster, exactly; value, count and face
    as tests/test_gpu_fill_holes.py::test_region_graph_against_numpy compares them -> the device's region volume"""
    cc = np.asfortranarray(cc)
    value, count, face, _, region = fill_ref.region_graph(cc)
    flat = region.reshape(-1, order="F")
    ids, first = np.unique(flat, return_index=True)
    order = ids[np.argsort(first)]                        # numpy's ids in the order of their first voxel
    renumber = np.zeros(len(value), dtype=np.uint32)
    renumber[order] = np.arange(1, len(order) + 1, dtype=np.uint32)
    want = renumber[region]
    d_region, g_value, g_count, g_face, _, info = eng.region_graph(eng.to_device(cc), cc.dtype.itemsize, cc.shape)
    got = eng.to_host_volume(d_region, cc.shape)
    assert info["regions"] == len(value) - 1
    assert got.dtype == want.dtype == np.uint32
    if not np.array_equal(got, want):
        np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(g_value[1:], value[order])
    np.testing.assert_array_equal(g_count[1:], count[order])
    np.testing.assert_array_equal(g_face[1:], face[order])
    assert g_value.dtype == value.dtype and g_count.dtype == count.dtype and g_face.dtype == face.dtype
    return got


# -- the link rules, exhaustively ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width,xs,sx", D.LINK_CASES)
@pytest.mark.parametrize("offset", D.LINK_OFFSETS)
def test_ccl_link_rule_on_every_window(eng, offset, width, xs, sx):
    lw = D.link_windows(offset, width, xs, sx, (0, 1, 2), 0, dtype=np.uint8 if width == 4 else np.uint32)
    _, n, _ = _check_ccl(eng, lw.volume)
    assert n > 3 ** (2 * width)


@pytest.mark.parametrize("width,xs,sx", D.LINK_CASES)
@pytest.mark.parametrize("offset", D.FACE_OFFSETS)
def test_regions_link_rule_on_every_window(eng, offset, width, xs, sx):
    lw = D.link_windows(offset, width, xs, sx, (0, 1, 2), 0, dtype=np.uint8 if width == 4 else np.uint16)
    got = _check_regions(eng, lw.volume)
    assert int(got.max()) > 3 ** (2 * width)


# -- numbering at scale -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,dtype", D.CCL_SCALE_CASES)
def test_ccl_numbering_at_scale(eng, shape, dtype):
    lab = D.salt_and_pepper(shape, dtype, seed=shape[1])
    d_cc, n, _ = _check_ccl(eng, lab)
    if shape[2] == 1:                                     # a plane: its tiny components do not merge through a third axis
        assert n > D.CCL_U16_COMPONENTS                   # (the oracle's count: _check_ccl has compared the two)
        assert not hasattr(d_cc, "kh_u16") and eng.narrow(d_cc) == (d_cc, 4)    # the u16 copy of the ids is not used
    else:
        assert n > 1000


# -- labels that differ in their high bits only --------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,seed", [((70, 33, 21), 1), ((300, 5, 3), 3)])
@pytest.mark.parametrize("dtype", [np.uint16, np.uint32, np.uint64])
def test_ccl_wide_values(eng, shape, seed, dtype):
    import oracle
    small = D.salt_and_pepper(shape, np.uint8, seed)
    wide = D.widen(small, dtype)
    assert wide.dtype == dtype and len(np.unique(wide)) == 4
    _, n, want = _check_ccl(eng, wide)
    want_small, n_small = oracle.connected_components(small)
    assert n == n_small
    np.testing.assert_array_equal(want, want_small)       # the oracle tells the wide values apart like the small ones


@pytest.mark.parametrize("shape,seed", [((70, 33, 21), 1), ((300, 5, 3), 3)])
def test_regions_wide_values(eng, shape, seed):
    small = D.salt_and_pepper(shape, np.uint8, seed)
    wide = D.widen(small, np.uint64)
    got = _check_regions(eng, wide)
    region_small = fill_ref.region_graph(small)[4]
    assert np.array_equal(fill_ref.region_graph(wide)[4], region_small)
    assert int(got.max()) == int(region_small.max())
