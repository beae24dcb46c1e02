"""Conditions on the inputs of tests/test_gpu_edt_dispatch.py and tests/test_gpu_ccl_patterns.py, asserted on the builders of
tests/dispatch_shapes.py alone (no GPU): the link windows are complete and isolated, the row zoo holds the rows it promises, the wide
values collide on the narrower type, and every shape lies on the side of its threshold that its test is about."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dispatch_shapes as D  # noqa: E402


def _changes(row):
    """the x at which a run starts (x > 0, label differs from x - 1): the bits the x pass ballots"""
    return (np.flatnonzero(row[1:] != row[:-1]) + 1).tolist()


# -- link_windows -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width,xs,sx", D.LINK_CASES)
@pytest.mark.parametrize("offset", D.LINK_OFFSETS)
def test_link_windows_are_complete_and_isolated(offset, width, xs, sx):
    import oracle
    lw = D.link_windows(offset, width, xs, sx, (0, 1, 2), 0)
    vol = lw.volume
    assert vol.flags.f_contiguous and vol.size < 6_000_000
    dy, dz = offset
    nassign = 3 ** (2 * width)
    cols = np.arange(width)
    later = vol[lw.x[:, None] + cols, lw.y[:, None], lw.z[:, None]].astype(np.int64)
    earlier = vol[lw.x[:, None] + cols, lw.y[:, None] + dy, lw.z[:, None] + dz].astype(np.int64)
    key = (np.concatenate([later, earlier], axis=1) * 3 ** np.arange(2 * width)).sum(axis=1)      # read back from the volume
    assert np.array_equal(key, lw.code)
    for x in xs:
        assert len(np.unique(key[lw.x == x])) == nassign          # every assignment at every requested x
    assert (lw.x.size == nassign * len(xs)) and int(vol.astype(bool).sum()) == int((np.concatenate([later, earlier], axis=1) != 0).sum())
    # the oracle's components never span two cells, and a cell holds one window
    cell = D.link_window_cells(lw, xs)
    inst = cell[lw.x, lw.y, lw.z]
    assert len(np.unique(inst)) == inst.size
    assert np.array_equal(cell[lw.x + width - 1, lw.y + dy, lw.z + dz], inst)
    cc, n = oracle.connected_components(vol)
    lo = np.full(n + 1, np.iinfo(np.int64).max)
    hi = np.full(n + 1, -1)
    fg = cc != 0
    np.minimum.at(lo, cc[fg], cell[fg])
    np.maximum.at(hi, cc[fg], cell[fg])
    assert n > nassign and np.array_equal(lo[1:], hi[1:])


@pytest.mark.parametrize("offset", D.FACE_OFFSETS)
def test_link_windows_for_regions(offset):
    """for reg_link_kernel 0 is a value like any other: the same volumes, and the offsets are face neighbours"""
    assert offset in D.LINK_OFFSETS and abs(offset[0]) + abs(offset[1]) == 1
    lw = D.link_windows(offset, 3, (253, 255, 257), 260, (0, 1, 2), 0, dtype=np.uint16)
    assert lw.volume.dtype == np.uint16 and set(np.unique(lw.volume).tolist()) == {0, 1, 2}


# -- row_zoo ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sx", [513, 1024, 1025])
def test_row_zoo_holds_its_rows(sx):
    nrows = D.ROW_LENGTH_YZ[0] * D.ROW_LENGTH_YZ[1]
    zoo = D.row_zoo(sx, nrows, np.uint16, 5)
    assert zoo.shape == (sx, nrows, 1) and zoo.dtype == np.uint16 and zoo.flags.f_contiguous and int(zoo.max()) <= 3
    assert np.array_equal(zoo, D.row_zoo(sx, nrows, np.uint16, 5))
    rows = [zoo[:, k, 0] for k in range(nrows)]
    changes = [_changes(r) for r in rows]
    bounds = list(range(D.EDT_WORD, sx, D.EDT_WORD))
    nwords = (sx + D.EDT_WORD - 1) // D.EDT_WORD
    assert len(bounds) == nwords - 1
    words = [sorted({c // D.EDT_WORD for c in ch}) for ch in changes]
    for b in bounds:
        assert any(b in ch for ch in changes)                              # a change at b - 1 | b
        if b + 1 < sx:
            assert any(b + 1 in ch for ch in changes)                      # a change at b | b + 1
    several = 3
    assert any(ch == [1] for ch in changes) and nwords > several           # one change at x = 1, then nothing for nwords - 1 words
    assert any(ch == [sx - 1] for ch in changes)                           # one change at x = sx - 1, nothing in the words before it
    assert any(ch == [] and r[0] != 0 for ch, r in zip(changes, rows))     # no change: foreground ...
    assert any(ch == [] and r[0] == 0 for ch, r in zip(changes, rows))     # ... and background
    assert any(len(w) >= 3 and len(w) == len(ch) and all(b - a == 2 for a, b in zip(w, w[1:])) for w, ch in zip(words, changes))
    assert any(r[0] == 0 and r[-1] != 0 for r in rows) and any(r[-1] == 0 and r[0] != 0 for r in rows)
    # a single change on either side of a boundary in the middle of the row: the words on both sides of it are empty
    assert any(len(ch) == 1 and ch[0] % D.EDT_WORD == 0 and several * D.EDT_WORD <= ch[0] <= sx - several * D.EDT_WORD for ch in changes)
    assert any(len(ch) == 1 and ch[0] % D.EDT_WORD in (0, 1) and ch[0] >= bounds[-1] for ch in changes)
    # the rest is random: many changes at no particular place, and another seed gives other rows
    fixed = len(D.zoo_fixed_rows(sx))
    assert sum(len(ch) > 8 for ch in changes[fixed:]) >= 2
    other = D.row_zoo(sx, nrows, np.uint16, 6)
    assert np.array_equal(other[:, :fixed], zoo[:, :fixed]) and not np.array_equal(other, zoo)


def test_row_zoo_scales_to_many_rows():
    sx, sy, sz = D.LDS_SECOND_STEP_SHAPE
    zoo = D.row_zoo(sx, 400, np.uint8, 1)
    assert zoo.shape == (sx, 400, 1) and zoo.dtype == np.uint8
    nchanges = np.count_nonzero(zoo[1:, :, 0] != zoo[:-1, :, 0], axis=0)
    assert nchanges.min() == 0 and nchanges.max() > sx // 4 and len(np.unique(nchanges)) > 50
    with pytest.raises(ValueError):
        D.row_zoo(sx, 10, np.uint8, 1)


# -- wide values --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,narrower", [(np.uint16, np.uint8), (np.uint32, np.uint16), (np.uint64, np.uint32)])
def test_wide_values_collide_on_the_narrower_type(dtype, narrower):
    v = D.wide_values(dtype)
    assert v.dtype == dtype and len(v) == 3 and len(set(v.tolist())) == 3 and (v != 0).all()
    assert set(v.astype(narrower).tolist()) == {1}
    assert [int(a) for a in v] == sorted(int(a) for a in v)          # ascending: rank-based references number them alike
    small = np.array([[[0, 1], [2, 3]], [[3, 0], [1, 2]]], dtype=np.uint8)
    wide = D.widen(small, dtype)
    assert wide.dtype == dtype and wide.flags.f_contiguous
    assert np.array_equal(D.small_values(wide), small)
    assert np.array_equal(wide == 0, small == 0) and np.array_equal(wide[small == 2], np.full(2, v[1]))
    with pytest.raises(ValueError):
        D.widen(small + 3, dtype)


def test_small_values_keeps_zero_and_folds_the_rest():
    lab = np.array([0, 1000, 1003, 1001, 1007, 0, 1003], dtype=np.uint32).reshape(7, 1, 1)
    assert D.small_values(lab).reshape(-1).tolist() == [0, 1, 3, 2, 1, 0, 3]


# -- the shapes lie where their tests need them -------------------------------------------------------------------------------------
def test_thresholds_as_stated():
    assert (D.EDT_ROWS8_MAX_SX, D.EDT_ROWS16_MAX_SX, D.EDT_X_MAX_WAVES) == (512, 1024, 32768)
    assert (D.CCL_SCAN_BATCH, D.CCL_RELABEL_CAP, D.CCL_NUMBER_CAP) == (1 << 20, 16384 * 256, 16384 * 1024)


def test_row_lengths_straddle_the_x_pass_switches():
    path = {sx: D.edt_x_path(sx) for sx in D.ROW_LENGTHS}
    assert path == {511: "rows8", 512: "rows8", 513: "rows16", 577: "rows16", 1023: "rows16", 1024: "rows16", 1025: "lds"}
    for limit in (D.EDT_ROWS8_MAX_SX, D.EDT_ROWS16_MAX_SX):
        assert limit in D.ROW_LENGTHS and limit + 1 in D.ROW_LENGTHS and limit - 1 in D.ROW_LENGTHS
        assert D.edt_x_path(limit) != D.edt_x_path(limit + 1) and D.edt_x_path(limit) == D.edt_x_path(limit - 1)
    assert D.edt_x_grid((513,) + D.ROW_LENGTH_YZ)[1] == 1


def test_rows_per_wave_cases():
    wraps_and_returns = 0
    for shape, _, rpw in D.ROWS_PER_WAVE_CASES:
        sx, sy, sz = shape
        assert sy * sz > D.EDT_X_MAX_WAVES and D.edt_x_path(sx) == "rows8"
        grid, per_wave = D.edt_x_grid(shape)
        assert grid == D.EDT_X_MAX_BLOCKS and per_wave == rpw >= 2
        # some wave's range r0 .. r0 + rpw - 1 holds the last row of one plane and the first of the next
        starts = np.arange(0, sy * sz, rpw)
        assert ((starts % sy) + rpw > sy).any()
        wraps_and_returns += rpw > sy                    # ... and comes to the last row of that next plane too
    assert wraps_and_returns >= 2
    assert any(sy % 2 == 1 and rpw == 2 for (_, sy, _), _, rpw in D.ROWS_PER_WAVE_CASES)


def test_lds_and_label_y_pass_shapes():
    sx, sy, sz = D.LDS_SECOND_STEP_SHAPE
    assert D.edt_x_path(sx) == "lds" and D.EDT_X_MAX_WAVES < sy * sz < 2 * D.EDT_X_MAX_WAVES and D.edt_x_grid((sx, sy, sz))[1] == 2
    assert sx * sy * sz < 1 << 32
    sx, sy, sz = D.LABEL_Y_PASS_SHAPE
    assert D.edt_x_path(sx) == "lds"                      # no sign flags: the y pass reads the labels
    assert sy > 2 * 64 and sy % 64 != 0                   # more than two tiles of 64 along y (edt.hip:234), the last one partial
    assert sx > 16 * 64 and sx % 64 != 0                  # a partial tile along x
    for sx, sy, sz in D.INF_FLAG_SHAPES:
        assert sy * sz <= D.EDT_X_MAX_WAVES
    assert [D.edt_x_path(s[0]) for s in D.INF_FLAG_SHAPES] == ["rows8", "rows16"]


def test_ccl_scale_cases():
    (scan, _), (relabel, _), (number, _) = D.CCL_SCALE_CASES
    n = int(np.prod(scan))
    assert D.CCL_SCAN_BATCH < n <= D.CCL_RELABEL_CAP and -(-n // D.CCL_CHUNK) == 1026
    n = int(np.prod(relabel))
    assert D.CCL_RELABEL_CAP < n <= D.CCL_NUMBER_CAP
    n = int(np.prod(number))
    assert D.CCL_NUMBER_CAP < n < (1 << 32) - 1 and -(-n // D.CCL_CHUNK) > D.CCL_GRID_CAP
    for shape, _ in D.CCL_SCALE_CASES:
        assert shape[0] > 4 * D.CCL_LINK_TILE and shape[0] % D.CCL_LINK_TILE != 0      # rows of several link tiles, the last partial


def test_link_cases_sit_on_the_chunk_boundaries():
    (w4, xs4, sx4), (w3, xs3, sx3) = D.LINK_CASES
    assert any(x < D.CCL_LINK_CHUNK < x + w4 for x in xs4) and 0 in xs4 and max(xs4) + w4 == sx4      # 63 | 64, the row's two ends
    assert D.CCL_LINK_CHUNK < sx4 < 2 * D.CCL_LINK_CHUNK
    assert any(x < D.CCL_LINK_TILE < x + w3 for x in xs3)           # 255 | 256 inside a window,
    assert any(x + w3 == D.CCL_LINK_TILE for x in xs3)              # a window that ends at 255
    assert any(x == D.CCL_LINK_TILE + 1 for x in xs3)               # and one that starts behind 256
    assert D.CCL_LINK_TILE < sx3 < 2 * D.CCL_LINK_TILE
