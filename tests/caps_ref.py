"""What tests/test_gpu_grid_caps.py needs and nothing of the product: the grid caps of the whole-volume utility launchers of
csrc/points.hip, csrc/feature.hip and csrc/ccl.hip (each with the file:function it mirrors; tests/test_caps_ref_host.py reads the
literals back out of the sources), the shapes that lie past them, and vectorised numpy restatements of the kernels whose existing
reference is a Python loop (pinned against those loops at the small shapes by the same host file)."""
import numpy as np

# ---- the caps: (file, function whose body holds the literal) ---------------------------------------------------------------------
NEAREST_BLOCKS = 4096            # points.hip:kh_nearest_label_voxels      points_grid(ntiles, 4096); a block walks per_block tiles
FILL_U64_BLOCKS = 1024           # points.hip:kh_nearest_label_voxels      points_grid((nqueries + 255) / 256, 1024)
EDGE_COUNT_BLOCKS = 4096         # points.hip:kh_binary_edge_count         points_grid((nvox + 255) / 256, 4096)
EDGE_EMIT_TILES = 1 << 20        # points.hip:kh_binary_edge_emit          points_grid(ntiles, 1 << 20)
FEATURE_BLOCKS = 8192            # feature.hip:blocks_for                  if (g > 8192) g = 8192
CCL_TILES = 1 << 20              # ccl.hip:regions_impl / cclg_impl / kh_fill_voids_nd    ccl_grid(ntiles, 1, 1 << 20)
CCL_BLOCKS = 16384               # ccl.hip:ccl_grid                        int64_t cap = 16384
APPLY_BOX_BLOCKS = 2048          # ccl.hip:kh_region_apply_box             ccl_grid(nvox, 256, 2048)
THREADS = 256                    # threads of a block, voxels of an x tile
WAVES_PER_BLOCK = 4              # feature.hip:blocks_for_pieces           blocks_for(pieces * 64): four waves, four pieces per block

FILL_U64_ONE_PASS = FILL_U64_BLOCKS * THREADS        # 262 144 queries
EDGE_COUNT_ONE_PASS = EDGE_COUNT_BLOCKS * THREADS    # 1 048 576 voxels
FEATURE_ONE_PASS = FEATURE_BLOCKS * THREADS          # 2 097 152 voxels / seeds; 8192 chunks of 256 words
FEATURE_WAVES = FEATURE_BLOCKS * WAVES_PER_BLOCK     # 32 768 waves, one piece each per trip
CCL_ONE_PASS = CCL_BLOCKS * THREADS                  # 4 194 304 voxels
APPLY_BOX_ONE_PASS = APPLY_BOX_BLOCKS * THREADS      # 524 288 voxels

# ---- the shapes ----------------------------------------------------------------------------------------------------------------
BIG = (3, 1183, 1183)            # 4 198 467 voxels > CCL_ONE_PASS, 1 399 489 rows > CCL_TILES; x == 1 is interior: holes exist
BIG2D = (3, 1_400_000, 1)        # its 2-D twin
NEAREST_SHAPES = [(6, 70, 59), (6, 97, 85), (300, 70, 31)]      # per_block == 2 with empty blocks; per_block == 3; xt == 2
EDGE_XT2_SHAPE = (300, 41, 7)
N1 = 2 * FEATURE_ONE_PASS + 77   # 1-D arrays of feature.hip: two full passes of the capped grid and a partial chunk
NQUERIES = FILL_U64_ONE_PASS + 77
BOX = (70, 150, 120)             # box of the two piece kernels ...
CORE = ((1, 1, 1), (69, 149, 119))       # ... and its core: 2 * 148 * 118 = 34 928 pieces, 2160 waves take a second one
DATASET_XY = (3000, 3000)        # a virtual dataset around BOX whose raster indices pass 2^32
# the box flush with the dataset's end in y: kh_first_appearance_box refuses a box that leaves the dataset's SX x SY rows
ORIGIN = (2900, 2850, 590)
APPLY_BOX_NVOX = [APPLY_BOX_ONE_PASS, APPLY_BOX_ONE_PASS + 1, 2 * APPLY_BOX_ONE_PASS + 77]

NONE32 = 0xFFFFFFFF
NONE64 = 0xFFFFFFFFFFFFFFFF


def tiles(shape):
    """x tiles of 256 voxels of a volume: ((sx + 255) / 256) * sy * sz"""
    return ((shape[0] + THREADS - 1) // THREADS) * shape[1] * shape[2]


def nearest_launch(shape):
    """(ntiles, grid, per_block, blocks that get no tile at all) of kh_nearest_label_voxels"""
    ntiles = tiles(shape)
    grid = max(1, min(ntiles, NEAREST_BLOCKS))
    per_block = (ntiles + grid - 1) // grid
    used = (ntiles + per_block - 1) // per_block
    return ntiles, grid, per_block, grid - used


def pieces(lo, hi):
    """(pieces_x, pieces) of a core: 64 voxels of one x row each (feature.hip:make_box_core)"""
    n = [int(h) - int(l) for l, h in zip(lo, hi)]
    px = (n[0] + 63) // 64
    return px, px * n[1] * n[2]


def piece_of(lo, hi):
    """the piece of every core voxel, an int64 array of the core's shape: x piece fastest, then y, then z"""
    n = [int(h) - int(l) for l, h in zip(lo, hi)]
    px = (n[0] + 63) // 64
    cx, cy, cz = np.meshgrid(np.arange(n[0]), np.arange(n[1]), np.arange(n[2]), indexing="ij")
    return cx // 64 + px * (cy + n[1] * cz)


# ---- restatements ----------------------------------------------------------------------------------------------------------------
def first_appearance(flat, nnumbers):
    """kh_first_appearance: u32 [nnumbers + 1], the smallest index of every number 1..nnumbers in `flat`, NONE32 where it has none
    (entry 0 too)"""
    flat = np.asarray(flat, dtype=np.uint32).reshape(-1)
    first = np.full(nnumbers + 1, NONE32, dtype=np.uint32)
    at = np.flatnonzero((flat != 0) & (flat <= nnumbers))
    np.minimum.at(first, flat[at], at.astype(np.uint32))
    return first


def first_appearance_box(f, lo, hi, origin, SX, SY, nnumbers, first):
    """kh_first_appearance_box: `first` (int64 [nnumbers + 1], -1 = none) takes the smaller of what it holds and the smallest dataset
    raster index (ox + x) + SX * ((oy + y) + SY * (oz + z)) of every number 1..nnumbers among the core voxels [lo, hi) of the box f"""
    core = np.asarray(f)[tuple(slice(int(a), int(b)) for a, b in zip(lo, hi))].astype(np.int64)
    x, y, z = np.meshgrid(*[np.arange(int(a), int(b), dtype=np.int64) + int(o) for a, b, o in zip(lo, hi, origin)], indexing="ij")
    index = x + int(SX) * (y + int(SY) * z)
    ok = (core != 0) & (core <= nnumbers)
    seen = np.full(nnumbers + 1, np.iinfo(np.int64).max, dtype=np.int64)
    np.minimum.at(seen, core[ok], index[ok])
    held = np.where(first < 0, np.iinfo(np.int64).max, first)
    best = np.minimum(held, seen)
    first[...] = np.where(best == np.iinfo(np.int64).max, -1, best)
    return first


def seed(nvox, voxel, number, label, lab):
    """kh_geodesic_seed: (dist f32 [nvox], feature u32 [nvox]) -- +inf and NONE32 everywhere, then 0.0 and the smallest number at the
    voxel of every seed that lies inside the array on a voxel of its own non-zero label"""
    voxel, number, label = (np.asarray(a, dtype=np.uint32) for a in (voxel, number, label))
    lab = np.asarray(lab).reshape(-1)
    dist = np.full(nvox, np.inf, dtype=np.float32)
    feature = np.full(nvox, NONE32, dtype=np.uint32)
    inside = voxel.astype(np.int64) < nvox
    at = voxel[inside].astype(np.int64)
    ok = (label[inside] != 0) & (lab[at].astype(np.uint32) == label[inside])
    dist[at[ok]] = 0.0
    np.minimum.at(feature, at[ok], number[inside][ok])
    return dist, feature


def remap(f, lut, nnumbers):
    """kh_remap_u32: lut[f] for the numbers 1..nnumbers, 0 for everything else"""
    f = np.asarray(f, dtype=np.uint32)
    ok = (f != 0) & (f <= nnumbers)
    return np.where(ok, np.asarray(lut, dtype=np.uint32)[np.where(ok, f, 0)], 0).astype(np.uint32)


def graph_cells(lab, graph, black_border):
    """kh_edt_graph_cells: the doubled image u8 [2sx, 2sy, 2sz] -- voxel (x, y, z) at cell (2x, 2y, 2z); the cell towards its +x / +y /
    +z neighbour is foreground iff the voxel is and bit 0 / 2 / 4 of its graph word is set (without a black border: iff the voxel is,
    behind the last voxel of an axis); the other four cells of its 2 x 2 x 2 block follow the voxel"""
    fg = np.asarray(lab) != 0
    g = np.asarray(graph, dtype=np.uint32)
    px, py, pz = fg & ((g & 1) != 0), fg & ((g & 4) != 0), fg & ((g & 16) != 0)
    if not black_border:
        px[-1, :, :], py[:, -1, :], pz[:, :, -1] = fg[-1, :, :], fg[:, -1, :], fg[:, :, -1]
    cells = np.zeros(tuple(2 * s for s in fg.shape), dtype=np.uint8, order="F")
    cells[0::2, 0::2, 0::2] = fg
    cells[1::2, 0::2, 0::2] = px
    cells[0::2, 1::2, 0::2] = py
    cells[0::2, 0::2, 1::2] = pz
    cells[1::2, 1::2, 0::2] = cells[1::2, 0::2, 1::2] = cells[0::2, 1::2, 1::2] = cells[1::2, 1::2, 1::2] = fg
    return cells


def graph_sample(fine, shape):
    """kh_edt_graph_sample: the doubled field [2sx, 2sy, 2sz] at the voxel cells"""
    assert tuple(fine.shape) == tuple(2 * s for s in shape)
    return np.asfortranarray(fine[0::2, 0::2, 0::2])


def nearest_c_index(lab, label, centroids):
    """kh_nearest_label_voxels for the queries of one label: u64 [Q], per centroid the C-order index x*sy*sz + y*sz + z of the first
    voxel in C order among those of `label` at the smallest distance sqrt((dx*dx + dy*dy) + dz*dz), every operation rounded to
    float64 in that order; NONE64 when the label owns no voxel"""
    lab = np.asarray(lab)
    cen = np.asarray(centroids, dtype=np.float64).reshape(-1, 3)
    cloud = np.argwhere(lab == label)                      # C order
    if cloud.shape[0] == 0:
        return np.full(cen.shape[0], NONE64, dtype=np.uint64)
    d = cloud[:, None, :].astype(np.float64) - cen[None, :, :]
    dist = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
    win = cloud[np.argmin(dist, axis=0)]
    return ((win[:, 0] * lab.shape[1] + win[:, 1]) * lab.shape[2] + win[:, 2]).astype(np.uint64)


# ---- inputs whose layout is the point (tests/test_caps_ref_host.py asserts the layout) -------------------------------------------------
BAND_VALUES = {            # smallest (asked for), A, B (asked for), N (present, not asked for), largest (asked for), absent (asked for)
    np.dtype(np.uint16): dict(S=3, A=40, B=41, N=500, T=0xFFFF, ABSENT=7),
    np.dtype(np.uint64): dict(S=3, A=(1 << 40) + 1, B=(1 << 40) + 2, N=1 << 50, T=NONE64, ABSENT=1 << 33),
}
BAND_PATTERN = "AABNA0BNNTS"      # consecutive rows: the same label, another one, not in the table then in it (twice running too), 0


def banded_labels(shape, dtype):
    """labels constant along x and over the rows r = y + sy * z with the period of BAND_PATTERN (11: prime to the 2 and 3 tiles of a
    block, so every pair of neighbours of the pattern falls into one block somewhere); the voxels past x == 255 carry the next row's
    label -- the two halves of a long row, one block's two tiles, differ --, and the column x == 0 the label four rows on, so the
    lanes of one wave hold different cached labels"""
    v = dict(BAND_VALUES[np.dtype(dtype)], **{"0": 0})
    period = np.array([v[c] for c in BAND_PATTERN], dtype=dtype)
    sx, sy, sz = shape
    r = (np.arange(sy)[:, None] + sy * np.arange(sz)[None, :])
    lab = np.empty(shape, dtype=dtype, order="F")
    lab[:256] = period[r % period.size][None]
    lab[256:] = period[(r + 1) % period.size][None]
    lab[0] = period[(r + 4) % period.size]
    return lab


def nearest_queries(shape, dtype, per_label=5):
    """(words u64 ascending, query_start u32, centroids f64 [Q, 3]) for banded_labels(shape, dtype): the smallest and the largest
    label present, A, B and an absent one; centroids on the 1/8 grid, some outside the volume, the last of each label at half-integer
    coordinates, where the nearest voxels tie"""
    v = BAND_VALUES[np.dtype(dtype)]
    words = np.array(sorted(v[k] for k in ("S", "A", "B", "T", "ABSENT")), dtype=np.uint64)
    rng = np.random.default_rng(sum(shape) + np.dtype(dtype).itemsize)
    cen = rng.integers(-3 * 8, (np.array(shape) + 3) * 8, size=(words.size, per_label, 3)) / 8.0
    cen[:, -1] = rng.integers(0, np.array(shape) - 1, size=(words.size, 3)) + 0.5
    start = np.arange(words.size + 1, dtype=np.uint32) * np.uint32(per_label)
    return words, start, cen.reshape(-1, 3)


APPEARANCE_NUMBERS = 1000
EARLY, LATE, LAST = (1, 900), (900, 986), (990, 1001)     # numbers anywhere / behind the first pass only / in the last partial chunk only


def appearance_words(n=N1, seed=5):
    """u32 [n] for kh_first_appearance with APPEARANCE_NUMBERS: runs of 1..39 equal numbers; 0, nnumbers + 1 and NONE32 among them;
    a run across every multiple of 256 (six words long: the chunk and the pass boundaries) and across every multiple of 64 but those
    that are 64 mod 1024 (a number may start at a wave's first lane too); the numbers of LATE only behind the first pass of the capped
    grid, those of LAST only in the last, partial chunk, 986..989 nowhere"""
    rng = np.random.default_rng(seed)
    length = rng.integers(1, 40, size=n // 8)
    assert int(length.sum()) >= n
    start = np.cumsum(length) - length
    number = rng.integers(*EARLY, size=length.size).astype(np.uint32)
    late = (start >= FEATURE_ONE_PASS) & (rng.random(length.size) < 0.1)
    number[late] = rng.integers(*LATE, size=int(late.sum()))
    special = rng.random(length.size) < 0.03
    number[special] = rng.choice(np.array([0, APPEARANCE_NUMBERS + 1, NONE32], dtype=np.uint32), size=int(special.sum()))
    f = np.repeat(number, length)[:n]
    b = np.arange(64, n - 3, 64)
    b = b[b % 1024 != 64]
    f[b] = f[b - 1]
    b = np.arange(256, n - 3, 256)
    for k in range(-2, 3):
        f[b + k] = f[b - 3]
    last = (n // 256) * 256
    assert n - last >= 5 + 6 * (LAST[1] - LAST[0])
    for k, value in enumerate(range(*LAST)):
        f[last + 5 + 6 * k:last + 11 + 6 * k] = value
    return f


def seed_case(n=N1, seed=6):
    """(lab u8 [n], voxel, number, label u32 [n]) for kh_geodesic_seed: n seeds on n voxels; voxels repeat with different numbers,
    one seed in ten names a label its voxel does not carry, label 0 seeds nothing, one in a hundred lies at or past nvox"""
    rng = np.random.default_rng(seed)
    lab = rng.integers(0, 4, size=n, dtype=np.uint8)
    voxel = rng.integers(0, n, size=n, dtype=np.int64)
    voxel[1::7] = voxel[0::7][:voxel[1::7].size]                   # the same voxel twice, a different number each time
    label = lab[voxel].astype(np.uint32)
    off = rng.random(n) < 0.1
    label[off] = (label[off] + 1) % 4
    past = rng.random(n) < 0.01
    voxel[past] = np.where(rng.random(int(past.sum())) < 0.5, n + rng.integers(0, 1000, size=int(past.sum())), NONE32)
    voxel[-1], label[-1] = n, 1                                    # the first index outside, as the last seed
    number = rng.integers(1, 1 << 31, size=n, dtype=np.int64).astype(np.uint32)
    return lab, voxel.astype(np.uint32), number, label
