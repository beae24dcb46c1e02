"""Inputs for the tests of csrc/edt.hip and csrc/ccl.hip at the shapes where they switch code paths (numpy only, no GPU):

  row_zoo        rows of labels with their changes placed on and around every 64-voxel word boundary of the x pass
  wide_values    non-zero label values that agree in their low bits, widen() maps a small-valued volume through them
  link_windows   every assignment of three values to a window of two adjacent rows, for the link rules of ccl_link_kernel and
                 reg_link_kernel

and the shapes themselves, with the thresholds they are chosen around.  tests/test_dispatch_shapes_host.py holds the builders and
the shapes to what is claimed here; tests/test_gpu_edt_dispatch.py and tests/test_gpu_ccl_patterns.py run them on the device."""
from collections import namedtuple

import numpy as np

# -- the thresholds, with the line of kimimaro_amd/csrc each comes from ------------------------------------------------------------
EDT_WORD = 64                        # edt.hip:143   a wave's ballot covers 64 voxels of a row: x = (c << 6) + lane
EDT_ROWS8_MAX_SX = 512               # edt.hip:565   nwords <= 8: edt_x_rows_kernel<LT, 8>
EDT_ROWS16_MAX_SX = 1024             # edt.hip:567   nwords <= 16: edt_x_rows_kernel<LT, 16>; above: edt_x_kernel (LDS), edt.hip:570
EDT_X_MAX_BLOCKS = 8192              # edt.hip:562   the x pass's grid is capped; 4 waves, one row each, per block
EDT_X_MAX_WAVES = 4 * EDT_X_MAX_BLOCKS       # 32768 rows: beyond it a wave of edt_x_rows_kernel walks several rows (edt.hip:138), and
                                             # edt_x_kernel takes a second grid-stride step (edt.hip:74)
CCL_CHUNK = 1024                     # ccl.hip:119   voxels per chunk of the flatten, scan and number kernels
CCL_SCAN_BATCH = 1024 * CCL_CHUNK    # ccl.hip:150   2^20 voxels: ccl_scan_kernel scans 1024 chunks per step and carries the sum beyond
CCL_GRID_CAP = 16384                 # ccl.hip:213   ccl_grid's default cap on the number of blocks
CCL_RELABEL_CAP = CCL_GRID_CAP * 256         # ccl.hip:231   above it a thread of ccl_relabel_kernel loops (ccl.hip:201)
CCL_NUMBER_CAP = CCL_GRID_CAP * CCL_CHUNK    # ccl.hip:228, 230   above it a block of the flatten / number kernels loops over chunks
                                             # (ccl.hip:120, 174) and reuses its __shared__ counter
CCL_LINK_CHUNK = 64                  # ccl.hip:94, 518   the x runs are pre-linked inside 64-lane chunks
CCL_LINK_TILE = 256                  # ccl.hip:82, 507   a block of the link kernels covers 256 voxels of a row
CCL_U16_COMPONENTS = 65536           # ccl.hip:200   fewer components: the ids are written once more as u16

# -- the shapes of the device tests -------------------------------------------------------------------------------------------------
ROW_LENGTHS = (511, 512, 513, 577, 1023, 1024, 1025)       # x (sy, sz) = (9, 4)
ROW_LENGTH_YZ = (9, 4)
LABEL_Y_PASS_SHAPE = (1030, 140, 5)
# (shape, anisotropy, rows per wave).  The issue's three, and two where a wave walks MORE than sy rows: only there does the y
# counter of edt_x_rows_kernel wrap and come back to the last row of a plane inside one wave's range, which is the one place where a
# counter that does not wrap gives another flag (the last row of a plane must carry none).  Such a flag acts like a black border
# above the plane, one step of y away: y is the finest axis there, so that nothing nearer hides it.
ROWS_PER_WAVE_CASES = (
    ((5, 7, 5000), (1, 2, 1), 2),
    ((3, 5, 14000), (2, 3, 5), 3),
    ((64, 3, 11000), (1, 1, 1), 2),
    ((5, 2, 40000), (1, 1, 4), 3),
    ((3, 3, 44000), (2, 1, 3), 5),
)
LDS_SECOND_STEP_SHAPE = (1025, 3, 10930)
INF_FLAG_SHAPES = ((70, 40, 12), (600, 40, 12))
CCL_SCALE_CASES = (((1040, 1010, 1), np.uint32), ((1030, 64, 66), np.uint16), ((1030, 128, 128), np.uint8))
LINK_OFFSETS = ((-1, 0), (-1, -1), (0, -1), (1, -1))       # (dy, dz) of the four earlier rows of ccl_link_kernel
FACE_OFFSETS = ((-1, 0), (0, -1))                          # the two of reg_link_kernel
LINK_CASES = ((4, (0, 62, 68), 72), (3, (253, 255, 257), 260))      # (width, xs, sx)


def edt_x_path(sx):
    """the x pass edt_impl picks for rows of sx voxels"""
    nwords = (sx + EDT_WORD - 1) // EDT_WORD
    return "rows8" if nwords <= 8 else ("rows16" if nwords <= 16 else "lds")


def edt_x_grid(shape):
    """(blocks, rows per wave) of the x pass as edt_impl computes them: the rows a wave of edt_x_rows_kernel walks, which is also the
    number of grid-stride steps of edt_x_kernel"""
    nrows = shape[1] * shape[2]
    grid = min((nrows + 3) // 4, EDT_X_MAX_BLOCKS)
    grid = (grid + 7) & ~7
    nwaves = 4 * grid
    return grid, -(-nrows // nwaves)


# -- row_zoo ------------------------------------------------------------------------------------------------------------------------
def zoo_fixed_rows(sx):
    """the rows row_zoo always starts with -> {name: row of small labels 0 .. 3}"""
    x = np.arange(sx)
    bounds = np.arange(EDT_WORD, sx, EDT_WORD)
    rows = {}
    rows["change_before_every_boundary"] = 1 + (x // EDT_WORD) % 2                      # label change at b - 1 | b
    rows["change_after_every_boundary"] = 1 + (np.maximum(x - 1, 0) // EDT_WORD) % 2    # at b | b + 1
    r = np.full(sx, 1)
    r[0] = 2
    rows["single_change_at_1"] = r
    r = np.full(sx, 1)
    r[sx - 1] = 2
    rows["single_change_at_end"] = r
    rows["constant_foreground"] = np.full(sx, 3)
    rows["constant_background"] = np.zeros(sx, dtype=np.int64)
    rows["every_second_word"] = 1 + ((x + 2 * EDT_WORD - 37) // (2 * EDT_WORD)) % 2     # changes at 37, 165, 293, ...: empty words between
    rows["odd_words_last_bit"] = 2 + ((x + 1) // (2 * EDT_WORD)) % 2                    # changes at 127, 255, ...: bit 63 of the odd words
    r = np.full(sx, 1)
    r[:5] = 0
    rows["starts_with_background"] = r
    r = np.full(sx, 2)
    r[sx - 3:] = 0
    rows["ends_with_background"] = r
    mid = int(bounds[len(bounds) // 2])
    r = np.full(sx, 3)
    r[mid:] = 1
    rows["single_change_before_middle_boundary"] = r                                    # at mid - 1 | mid and nowhere else
    last = int(bounds[-1])
    r = np.full(sx, 2)
    if last + 1 < sx:
        r[last + 1:] = 3
    else:
        r[last:] = 3
    rows["single_change_after_last_boundary"] = r                                       # at last | last + 1 (a row that ends at last: before it)
    return rows


def _random_rows(sx, n, rng):
    """n rows of random runs of the labels 0 .. 3; the mean run length differs from row to row (2 .. 512 voxels)"""
    if n == 0:
        return np.zeros((sx, 0), dtype=np.uint8)
    p = np.exp2(-rng.integers(1, 10, n)).astype(np.float32)
    change = rng.random((n, sx), dtype=np.float32) < p[:, None]
    step = rng.integers(1, 4, (n, sx), dtype=np.uint8)
    step[~change] = 0
    step[:, 0] = rng.integers(0, 4, n, dtype=np.uint8)
    lab = np.cumsum(step, axis=1, dtype=np.uint8) & np.uint8(3)         # a step of 1 .. 3 modulo 4: neighbouring runs differ
    return lab.T


def row_zoo(sx, nrows, dtype, seed):
    """An F-ordered (sx, nrows, 1) block of labels 0 .. 3 (reshape it to any (sx, sy, sz) with sy * sz == nrows).  The first rows are
    zoo_fixed_rows(sx), then come rows with ONE label change each, on either side of one word boundary after the other (as many as
    leave a quarter of the block free), the rest are random runs drawn from `seed`."""
    if sx < 2 * EDT_WORD + 2:
        raise ValueError("row_zoo: rows of at least two words and two voxels")
    fixed = list(zoo_fixed_rows(sx).values())
    if nrows < len(fixed) + 4:
        raise ValueError("row_zoo: %d rows do not hold the %d fixed ones and four random ones" % (nrows, len(fixed)))
    bounds = np.arange(EDT_WORD, sx, EDT_WORD)
    singles = []
    for k, b in enumerate(bounds.tolist()):
        at = b if k % 2 == 0 else min(b + 1, sx - 1)
        r = np.full(sx, 1 + k % 3)
        r[at:] = 1 + (k + 1) % 3
        singles.append(r)
    singles = singles[:max(0, nrows - len(fixed) - max(4, nrows // 4))]
    head = np.stack(fixed + singles, axis=1).astype(np.uint8)
    rng = np.random.default_rng(seed)
    out = np.concatenate([head, _random_rows(sx, nrows - head.shape[1], rng)], axis=1)
    return np.asfortranarray(out.astype(dtype)[:, :, np.newaxis])


# -- wide values --------------------------------------------------------------------------------------------------------------------
def wide_values(dtype):
    """three non-zero labels of `dtype` that a comparison on the next narrower type cannot tell apart"""
    dtype = np.dtype(dtype)
    table = {2: (1, 257, 513), 4: (1, 65537, 1 + (1 << 24)), 8: (1, 1 + (1 << 32), 1 + (1 << 63))}
    return np.array(table[dtype.itemsize], dtype=dtype)


def small_values(labels):
    """a label volume folded onto 0 .. 3: 0 stays 0, the k-th non-zero value (ascending) becomes 1 + k % 3"""
    labels = np.asarray(labels)
    values = np.unique(labels)
    values = values[values != 0]
    rank = np.searchsorted(values, labels)
    return np.where(labels == 0, 0, 1 + rank % 3).astype(np.uint8, order="F")


def widen(small, dtype):
    """a volume of labels 0 .. 3 with 1, 2, 3 replaced by wide_values(dtype)"""
    small = np.asarray(small)
    if small.size and int(small.max()) > 3:
        raise ValueError("widen: labels 0 .. 3 only")
    table = np.concatenate([np.zeros(1, dtype=dtype), wide_values(dtype)])
    return np.asfortranarray(table[small.astype(np.intp)])


# -- link windows -------------------------------------------------------------------------------------------------------------------
LinkWindows = namedtuple("LinkWindows", "volume offset width x y z code cell_shape")
LinkWindows.__doc__ = """volume: the labels (F order); the k-th instance is the window whose LATER row starts at (x[k], y[k], z[k]) and
whose earlier row starts at (x[k], y[k] + dy, z[k] + dz); code[k] numbers its assignment (digit j, base 3: column j of the later
row for j < width, column j - width of the earlier row else); cell_shape: the (y, z) extent of a cell, separators included."""


def _x_groups(xs, width):
    """windows that leave a voxel between them share their rows; the others get rows of their own -> [[x, ...], ...]"""
    groups = []
    for x in sorted(xs):
        for g in groups:
            if x - (g[-1] + width) >= 1:
                g.append(x)
                break
        else:
            groups.append([x])
    return groups


def link_windows(offset, width, xs, sx, values, background, dtype=np.uint8):
    """Every assignment of `values` (three of them) to a window of two rows by `width` voxels, the rows being a row and the earlier
    row at `offset` = (dy, dz) from it, the window's first column at every x of `xs`: 3^(2 width) instances per x.  Every instance
    has a cell of its own, a box of the volume in which everything but the window is `background`; a window touches no face of its
    cell that another cell shares, so with a background that is no value no two windows are 26-neighbours.  The cells are laid out
    over y and z (over y alone for dz = 0: the volume is one plane); windows whose columns leave a voxel between them share rows and
    split them along x."""
    dy, dz = offset
    if (dy, dz) not in LINK_OFFSETS or len(values) != 3 or min(xs) < 0 or max(xs) + width > sx:
        raise ValueError("link_windows: bad arguments")
    groups = _x_groups(xs, width)
    nassign = 3 ** (2 * width)
    ncell = nassign * len(groups)
    cy, cz = 1 + abs(dy) + 1, (1 + abs(dz) + 1 if dz else 1)
    gy = ncell if dz == 0 else int(np.ceil(np.sqrt(ncell)))
    gz = -(-ncell // gy)
    vol = np.full((sx, gy * cy, gz * cz), background, dtype=dtype, order="F")
    code = np.arange(nassign)
    digits = (code[:, None] // 3 ** np.arange(2 * width)[None, :]) % 3
    cells = np.asarray(values, dtype=dtype)[digits]                     # [assignment, 2 width]
    X, Y, Z, K = [], [], [], []
    for g, gx in enumerate(groups):
        cell = g * nassign + code
        y0 = (cell % gy) * cy + (1 if dy < 0 else 0)                    # the later row inside its cell
        z0 = (cell // gy) * cz + (1 if dz < 0 else 0)
        for x in gx:
            for j in range(width):
                vol[x + j, y0, z0] = cells[:, j]
                vol[x + j, y0 + dy, z0 + dz] = cells[:, width + j]
            X.append(np.full(nassign, x))
            Y.append(y0)
            Z.append(z0)
            K.append(code)
    return LinkWindows(vol, (dy, dz), width, np.concatenate(X), np.concatenate(Y), np.concatenate(Z), np.concatenate(K), (cy, cz))


def link_window_cells(lw, xs):
    """the number of the cell every voxel of lw.volume lies in (int64, lw.volume's shape): rows first, and the rows that several
    windows share are split at the first column of the second, third, ... window"""
    sx, sy, sz = lw.volume.shape
    cy, cz = lw.cell_shape
    groups = _x_groups(xs, lw.width)
    nassign = 3 ** (2 * lw.width)
    gy = sy // cy
    yz = (np.arange(sy) // cy)[:, None] + gy * (np.arange(sz) // cz)[None, :]          # the cell of a row [sy, sz]
    group = np.minimum(yz // nassign, len(groups) - 1)
    part = np.zeros((len(groups), sx), dtype=np.int64)                                 # the part of a row a column lies in, per group
    for g, gx in enumerate(groups):
        for x in gx[1:]:
            part[g, x:] += 1
    nparts = max(len(g) for g in groups)
    return np.asfortranarray(yz[None, :, :] * nparts + part[group].transpose(2, 0, 1))


def salt_and_pepper(shape, dtype, seed):
    """the input of tests/test_gpu_ccl.py::test_ccl_matches_oracle: labels 0 .. 3, thousands of tiny components"""
    rng = np.random.default_rng(seed)
    lab = rng.integers(0, 4, size=shape).astype(dtype)
    lab[rng.random(shape) < 0.3] = 0
    return np.asfortranarray(lab)
