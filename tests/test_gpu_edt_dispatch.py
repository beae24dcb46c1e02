"""kh_edt (csrc/edt.hip) against the oracle, bit for bit, at the shapes where edt_impl changes its code path: the two register x-pass
kernels and the LDS one on either side of 512 and 1024 voxels per row, several rows per wave (more than 32768 rows), the y pass that
reads labels (rows above 1024 voxels), y flags on +inf and on 0, and labels that differ in their high bits only.  The inputs and the
thresholds are those of tests/dispatch_shapes.py; tests/test_dispatch_shapes_host.py checks them on the CPU."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dispatch_shapes as D  # noqa: E402
from shapes import voronoi_labels  # noqa: E402
from test_gpu_edt import CASES, gpu_edt  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from kimimaro_amd.engine import Engine
    return Engine()


def _same(eng, lab, an, black_border):
    import oracle
    lab = np.asfortranarray(lab)
    want = oracle.edt(lab, an, black_border)
    got = gpu_edt(eng, lab, an, black_border)
    assert got.dtype == np.float32 and got.shape == want.shape
    if not np.array_equal(got, want):             # (the report of assert_array_equal costs seconds on the largest volume)
        np.testing.assert_array_equal(got, want)
    return want


# -- row length: 8 words, 16 words, LDS ---------------------------------------------------------------------------------------------
# The rows of the zoo differ from their neighbours in y and z, so with pitches alike a label change one step away in y would hide
# every x distance beyond one voxel.  X_ONLY makes a step in y or z longer than the longest row: the x pass shows through in every
# voxel of a row that has a change (or a border), the y and z passes in the others.
X_ONLY = (1, 1200, 1500)
ROW_CASES = [(sx, np.uint16, X_ONLY) for sx in D.ROW_LENGTHS] + \
            [(1024, np.uint16, (3, 1, 2)), (512, np.uint8, X_ONLY), (513, np.uint8, X_ONLY)]


@pytest.mark.parametrize("sx,dtype,an", ROW_CASES)
@pytest.mark.parametrize("black_border", [False, True])
def test_edt_row_lengths(eng, sx, dtype, an, black_border):
    sy, sz = D.ROW_LENGTH_YZ
    assert an[1] > sx and an[2] > sx or an == (3, 1, 2)
    lab = D.row_zoo(sx, sy * sz, dtype, seed=sx).reshape((sx, sy, sz), order="F")
    _same(eng, lab, an, black_border)


# -- the y pass that reads labels (sx > 1024), with halo and bands -------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _label_y_pass_input(kind):
    shape = D.LABEL_Y_PASS_SHAPE
    if kind == "one_label":
        lab = np.full(shape, 7, dtype=np.uint16, order="F")
        lab[np.random.default_rng(2).random(shape) < 0.005] = 0         # windows far wider than the halo of 8 rows: bands
        return lab
    return np.asfortranarray(voronoi_labels(shape, 9, seed=4, pts_per_label=4, step=40.0).astype(np.uint16))


@pytest.mark.parametrize("kind", ["one_label", "voronoi"])
@pytest.mark.parametrize("black_border", [False, True])
def test_edt_label_reading_y_pass(eng, kind, black_border):
    lab = _label_y_pass_input(kind)
    runs = np.diff(np.flatnonzero(np.concatenate([[True], lab[1:, 70, 2] != lab[:-1, 70, 2], [True]])))
    assert runs.max() > 4 * 2 * 8                 # the y pass starts from x distances of many halos (8 rows of pitch 2): bands
    _same(eng, lab, (1, 2, 1), black_border)


# -- several rows per wave -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def _rows_per_wave_input(shape, kind):
    if kind == "voronoi":
        lab = voronoi_labels(shape, 9, seed=sum(shape), pts_per_label=6, step=0.02 * shape[2]).astype(np.uint16)
        lab[np.random.default_rng(1).random(shape) < 0.05] = 0
        return np.asfortranarray(lab)
    # a function of (y, z) alone: every row is constant, so every y flag sits on +inf (or, on the background rows, on 0)
    y, z = np.meshgrid(np.arange(shape[1]), np.arange(shape[2]), indexing="ij")
    row = 1 + (y // 3 + z // 9 + z // 31) % 4
    row[(y + 2 * z) % 11 == 0] = 0
    return np.asfortranarray(np.broadcast_to(row[None, :, :], shape).astype(np.uint16))


@pytest.mark.parametrize("kind", ["voronoi", "yz_only"])
@pytest.mark.parametrize("shape,an,rpw", D.ROWS_PER_WAVE_CASES)
@pytest.mark.parametrize("black_border", [False, True])
def test_edt_several_rows_per_wave(eng, shape, an, rpw, kind, black_border):
    assert shape[1] * shape[2] > D.EDT_X_MAX_WAVES and D.edt_x_grid(shape)[1] == rpw
    lab = _rows_per_wave_input(shape, kind)
    if kind == "yz_only":
        assert (lab == lab[:1]).all()
    _same(eng, lab, an, black_border)


# -- the LDS x pass takes a second grid-stride step ----------------------------------------------------------------------------------
def _lds_second_step_input():
    sx, sy, sz = D.LDS_SECOND_STEP_SHAPE
    lab = D.row_zoo(sx, sy * sz, np.uint8, seed=9).reshape(-1, order="F")
    rng = np.random.default_rng(10)
    lab[rng.integers(0, lab.size, lab.size // 400)] = 0                 # noise: holes
    lab[rng.integers(0, lab.size, lab.size // 400)] = 200               # ... and a label of its own
    return lab.reshape((sx, sy, sz), order="F")


def test_edt_lds_x_pass_second_step(eng):
    shape = D.LDS_SECOND_STEP_SHAPE
    assert D.edt_x_path(shape[0]) == "lds" and shape[1] * shape[2] > D.EDT_X_MAX_WAVES
    _same(eng, _lds_second_step_input(), X_ONLY, True)    # (with three rows per plane and a black border, equal pitches would hide x)


# -- y flags on +inf and on 0 --------------------------------------------------------------------------------------------------------
def _slabs(shape):
    """labels constant along x: slabs stacked in y and in z, some of them background, no holes"""
    sx, sy, sz = shape
    ycut = np.searchsorted([7, 8, 20, 33], np.arange(sy), side="right")      # 5 slabs in y, one of them a single row
    zcut = np.searchsorted([3, 4, 9], np.arange(sz), side="right")           # 4 in z
    table = np.array([[1, 2, 0, 3], [0, 3, 1, 2], [2, 1, 3, 0], [3, 0, 2, 1], [1, 2, 3, 1]], dtype=np.uint16)
    row = table[ycut[:, None], zcut[None, :]]
    return np.asfortranarray(np.broadcast_to(row[None, :, :], shape).copy())


@pytest.mark.parametrize("shape", D.INF_FLAG_SHAPES)
def test_edt_flags_on_inf_and_zero(eng, shape):
    lab = _slabs(shape)
    fg = lab != 0
    assert (lab == lab[:1]).all() and fg.any() and (~fg).any()           # no change along x and no black border: the x pass gives +inf
    up = lab[:, 1:, :] != lab[:, :-1, :]                                 # on every foreground voxel, and the flags go onto +inf and onto 0
    assert (up & fg[:, :-1, :]).any() and (up & ~fg[:, :-1, :]).any()
    want = _same(eng, lab, (16, 16, 40), False)
    assert np.isfinite(want[fg]).all() and (want[fg] > 0).all() and (want[~fg] == 0).all()


# -- labels that differ in their high bits only --------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [1, 2])
@pytest.mark.parametrize("dtype", [np.uint16, np.uint32])
@pytest.mark.parametrize("black_border", [False, True])
def test_edt_wide_values(eng, case, dtype, black_border):
    import oracle
    shape, nlab, an, _ = CASES[case]                                     # (70, 33, 21) and (130, 40, 17)
    lab = voronoi_labels(shape, nlab, seed=sum(shape), anisotropy=(1, 1, 1), dtype=np.uint32)
    lab[np.random.default_rng(1).random(shape) < 0.05] = 0
    small = D.small_values(lab)
    wide = D.widen(small, dtype)
    assert len(np.unique(wide)) == 4 and len(np.unique(wide.astype(np.uint8 if dtype == np.uint16 else np.uint16))) == 2
    want = oracle.edt(small, an, black_border)
    np.testing.assert_array_equal(oracle.edt(wide, an, black_border), want)
    np.testing.assert_array_equal(gpu_edt(eng, wide, an, black_border), want)
