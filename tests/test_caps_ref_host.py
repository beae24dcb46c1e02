"""Host tier of tests/test_gpu_grid_caps.py: the numpy restatements of tests/caps_ref.py against the slow references the suite has
already (at their small shapes), the arithmetic that puts every big shape past its cap, the layout of the generated inputs, and the
cap literals of caps_ref against the launch lines of the .hip sources -- a changed cap fails here instead of silently turning the big
shapes into small ones."""
import os
import re

import numpy as np
import pytest

import caps_ref as R
import points_ref

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "kimimaro_amd", "csrc")


# ---- the restatements against the slow references ---------------------------------------------------------------------------------
def test_first_appearance_box_equals_the_loop():
    from test_gpu_oversegment_chunked import BOXES, cores_of, first_appearance_host, runs_of_numbers
    rng = np.random.default_rng(5)
    nn = 40
    for box in BOXES:
        for lo, hi in cores_of(box):
            f = runs_of_numbers(rng, box, nn)
            got, want = np.full(nn + 1, -1, dtype=np.int64), np.full(nn + 1, -1, dtype=np.int64)
            for origin, SX, SY in (((2900, 2950, 590), 3000, 3000), ((0, 0, 0), box[0], box[1])):       # the second accumulates
                first_appearance_host(f, lo, hi, origin, SX, SY, nn, want)
                assert R.first_appearance_box(f, lo, hi, origin, SX, SY, nn, got) is got
                np.testing.assert_array_equal(got, want)
            assert want.max() < 2 ** 32 and (want >= 0).any() and want[0] == -1


def test_first_appearance_equals_the_loop():
    """the 1-D kernel is the box kernel on a box of one row at the origin of a dataset of that row"""
    from test_gpu_oversegment_chunked import first_appearance_host
    rng = np.random.default_rng(6)
    n, nn = 700, 30
    f = np.repeat(rng.integers(0, nn + 3, size=n, dtype=np.uint32), 3)[:n]
    f[rng.random(n) < 0.1] = R.NONE32
    f[f == 17] = 0                                                              # a number without a voxel
    want = np.full(nn + 1, -1, dtype=np.int64)
    first_appearance_host(f.reshape(n, 1, 1), (0, 0, 0), (n, 1, 1), (0, 0, 0), n, 1, nn, want)
    got = R.first_appearance(f, nn)
    assert got.dtype == np.uint32 and got[0] == R.NONE32 and got[17] == R.NONE32
    np.testing.assert_array_equal(got, np.where(want < 0, R.NONE32, want).astype(np.uint32))


def test_seed_and_remap_equal_their_loops():
    lab, voxel, number, label = R.seed_case(900, seed=3)
    dist, feature = np.full(900, np.inf, dtype=np.float32), np.full(900, R.NONE32, dtype=np.uint32)
    hits = 0
    for v, k, L in zip(voxel.tolist(), number.tolist(), label.tolist()):
        if v >= 900 or L == 0 or int(lab[v]) != L:
            continue
        hits += 1
        dist[v] = 0.0
        feature[v] = min(int(feature[v]), k)
    got_dist, got_feature = R.seed(900, voxel, number, label, lab)
    np.testing.assert_array_equal(got_dist.view(np.uint32), dist.view(np.uint32))
    np.testing.assert_array_equal(got_feature, feature)
    assert 300 < hits and (voxel >= 900).sum() >= 2 and hits > (feature != R.NONE32).sum()      # some voxel was seeded twice
    rng = np.random.default_rng(4)
    f = rng.integers(0, 25, size=500).astype(np.uint32)
    f[::9] = R.NONE32
    lut = rng.integers(0, 1 << 32, size=21, dtype=np.uint64).astype(np.uint32)
    want = np.array([int(lut[v]) if 0 < v <= 20 else 0 for v in f.tolist()], dtype=np.uint32)
    np.testing.assert_array_equal(R.remap(f, lut, 20), want)


def test_nearest_c_index_equals_the_statement():
    from shapes import voronoi_labels
    from test_points_host import dyadic_synapses
    labels = voronoi_labels((13, 11, 9), 4, seed=3, pts_per_label=2, step=3.0, dtype=np.uint16)
    synapses = dyadic_synapses(labels, 11)
    synapses[int(labels[6, 5, 4])].append(((6.5, 5.5, 4.5), 0))                # a tie between the voxels around a corner
    asked = 0
    for label, pairs in synapses.items():
        got = R.nearest_c_index(labels, label, [c for c, _ in pairs])
        for (centroid, swc), index in zip(pairs, got.tolist()):
            (chosen, _), = points_ref.synapses_to_targets(labels, {label: [(centroid, swc)]}).items()
            assert index == (chosen[0] * 11 + chosen[1]) * 9 + chosen[2]
            asked += 1
    assert asked > 20
    assert R.nearest_c_index(labels, 999, [(1.0, 2.0, 3.0)] * 2).tolist() == [R.NONE64] * 2


def test_graph_cells_and_sample(monkeypatch):
    # by hand: two voxels along x, the second one background; the first may step to +y only
    lab = np.zeros((2, 2, 2), dtype=np.uint8, order="F")
    lab[0, 0, 0] = lab[0, 1, 1] = 1
    g = np.zeros((2, 2, 2), dtype=np.uint32, order="F")
    g[0, 0, 0] = 4
    g[0, 1, 1] = 1 | 4 | 16
    g[1, 0, 0] = 0x3FFFFFF                                                      # a background voxel's word counts for nothing
    for black in (0, 1):
        cells = R.graph_cells(lab, g, black)
        assert cells.shape == (4, 4, 4) and cells.dtype == np.uint8
        want = np.zeros((4, 4, 4), dtype=np.uint8)
        want[0:2, 0:2, 0:2] = 1
        want[1, 0, 0] = want[0, 0, 1] = 0                                       # no step to +x, none to +z
        want[0:2, 2:4, 2:4] = 1                                                 # (0, 1, 1) has all three bits: border or not, its cells stay
        np.testing.assert_array_equal(cells, want)
    g[0, 1, 1] = 0                                                              # no bits: only without a black border the cells behind
    assert R.graph_cells(lab, g, 0)[0, 3, 2] == 1 and R.graph_cells(lab, g, 1)[0, 3, 2] == 0      # the last voxel follow the voxel
    assert R.graph_cells(lab, g, 0)[1, 2, 2] == 0                               # (x == 0 is not the last voxel of its axis)
    # the oracle's cells: what oracle.edt_graph hands to its transform
    import oracle
    from voxel_graphs import random_graph
    rng = np.random.default_rng(8)
    shape = (7, 5, 4)
    lab = np.asfortranarray((rng.random(shape) < 0.8).astype(np.uint16) * np.uint16(300))
    g = random_graph(shape, rng, 0.4, symmetric=False)
    seen = []

    def capture(cells, anisotropy, black_border):
        seen.append(cells.copy())
        return np.arange(cells.size, dtype=np.float32).reshape(cells.shape, order="F")
    monkeypatch.setattr(oracle, "edt", capture)
    for black in (False, True):
        sampled = oracle.edt_graph(lab, g, (1, 1, 1), black_border=black)
        np.testing.assert_array_equal(R.graph_cells(lab, g, black), seen[-1])
        fine = np.arange(8 * lab.size, dtype=np.float32).reshape(tuple(2 * s for s in shape), order="F")
        np.testing.assert_array_equal(R.graph_sample(fine, shape), sampled)
    assert not np.array_equal(seen[0], seen[1])


# ---- every big shape is past its cap -----------------------------------------------------------------------------------------------
def test_the_shapes_lie_past_the_caps():
    assert [R.nearest_launch(s) for s in R.NEAREST_SHAPES] == [(4130, 4096, 2, 2031), (8245, 4096, 3, 1347), (4340, 4096, 2, 1926)]
    assert (R.NEAREST_SHAPES[2][0] + 255) // 256 == 2 and R.NEAREST_SHAPES[2][0] - 256 == 44
    assert R.NQUERIES == 262_144 + 77 > R.FILL_U64_ONE_PASS == 262_144
    nvox, rows = int(np.prod(R.BIG)), R.BIG[1] * R.BIG[2]
    assert nvox == 4_198_467 > R.CCL_ONE_PASS == 4_194_304 > R.FEATURE_ONE_PASS > R.EDGE_COUNT_ONE_PASS == 1_048_576
    assert rows == R.tiles(R.BIG) == 1_399_489 > R.CCL_TILES == R.EDGE_EMIT_TILES == 1 << 20
    assert int(np.prod(R.BIG2D)) > R.CCL_ONE_PASS and R.tiles(R.BIG2D) > R.CCL_TILES and R.BIG2D[2] == 1
    assert 8 * nvox < 2 ** 32                                                   # kh_edt_graph_cells takes the doubled image
    assert R.tiles(R.EDGE_XT2_SHAPE) == 2 * 41 * 7
    assert R.N1 == 2 * 2_097_152 + 77 and (R.N1 + 255) // 256 == 2 * R.FEATURE_BLOCKS + 1 and R.N1 % 256 == 77
    assert R.pieces(*R.CORE) == (2, 34_928) and R.FEATURE_WAVES == 32_768 and 34_928 - 32_768 == 2160
    piece = R.piece_of(*R.CORE)
    assert piece.shape == (68, 148, 118) and piece.max() == 34_927 and len(np.unique(piece)) == 34_928
    assert piece[63, 0, 0] == 0 and piece[64, 0, 0] == 1 and piece[0, 1, 0] == 2 and piece[0, 0, 1] == 2 * 148
    (SX, SY), top = R.DATASET_XY, [o + b - 1 for o, b in zip(R.ORIGIN, R.BOX)]
    assert top[0] < SX and top[1] < SY and R.ORIGIN[0] + SX * (R.ORIGIN[1] + SY * R.ORIGIN[2]) > 2 ** 32
    assert R.APPLY_BOX_NVOX == [524_288, 524_289, 2 * 524_288 + 77]
    assert all((n + 255) // 256 >= R.APPLY_BOX_BLOCKS for n in R.APPLY_BOX_NVOX) and R.APPLY_BOX_NVOX[1] > R.APPLY_BOX_ONE_PASS


@pytest.mark.parametrize("dtype", [np.uint16, np.uint64], ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("shape", R.NEAREST_SHAPES, ids=str)
def test_banded_labels_put_every_pair_into_one_block(shape, dtype):
    """what thread 1 of a block sees on consecutive tiles of its range: the same asked-for label, another asked-for one, one that
    is not in the table and then one that is, one that is not twice running, and 0"""
    v = R.BAND_VALUES[np.dtype(dtype)]
    lab = R.banded_labels(shape, dtype)
    table, start, cen = R.nearest_queries(shape, dtype)
    present = set(np.unique(lab).tolist())
    assert present == {0, v["S"], v["A"], v["B"], v["N"], v["T"]} and v["ABSENT"] not in present
    assert v["S"] == min(present - {0}) and v["T"] == max(present) == np.iinfo(dtype).max
    assert set(table.tolist()) == {v["S"], v["A"], v["B"], v["T"], v["ABSENT"]} and (np.diff(table.astype(object)) > 0).all()
    assert table[0] < v["ABSENT"] < table[-1] and cen.shape == (int(start[-1]), 3) and np.array_equal(cen * 8, np.round(cen * 8))
    ntiles, grid, per_block, empty = R.nearest_launch(shape)
    xt = (shape[0] + 255) // 256
    t = np.arange(ntiles)
    seen = lab[(t % xt) * 256 + 1, (t // xt) % shape[1], (t // xt) // shape[1]]
    asked = np.isin(seen, table)
    inside = (t[1:] // per_block) == (t[:-1] // per_block)                      # tile t and tile t + 1 belong to one block
    a, b, ka, kb = seen[:-1][inside], seen[1:][inside], asked[:-1][inside], asked[1:][inside]
    assert (ka & kb & (a == b)).any() and (ka & kb & (a != b)).any()
    assert (~ka & (a != 0) & kb).any() and (~ka & ~kb & (a == b) & (a != 0)).any()
    assert ((a == 0) & kb).any() and (ka & (b == 0)).any()
    assert empty > 0 and (grid - empty) * per_block >= ntiles
    assert (lab[0] != lab[1]).any() and (lab[1] == lab[min(shape[0], 256) - 1]).all()      # the lanes of one wave hold two labels
    if xt == 2:
        assert (lab[255] != lab[256]).any()


def test_appearance_words_straddle_the_boundaries():
    f = R.appearance_words()
    n, nn, one = R.N1, R.APPEARANCE_NUMBERS, R.FEATURE_ONE_PASS
    assert f.shape == (n,) and f.dtype == np.uint32
    b = np.arange(256, n - 3, 256)
    assert all((f[b + k] == f[b]).all() for k in (-3, -2, -1, 1, 2)) and one in b and 2 * one in b
    b = np.arange(64, n - 3, 64)
    assert (f[b] == f[b - 1])[b % 1024 != 64].all() and (f[b] != f[b - 1])[b % 1024 == 64].sum() > 100
    for special in (0, nn + 1, R.NONE32):
        assert (f[:one] == special).sum() > 1000 and (f[one:] == special).sum() > 1000
    first = R.first_appearance(f, nn)
    assert first.shape == (nn + 1,) and first[0] == R.NONE32
    assert (first[R.EARLY[0]:R.EARLY[1]] < one).all()
    assert ((first[R.LATE[0]:R.LATE[1]] >= one) & (first[R.LATE[0]:R.LATE[1]] < (n // 256) * 256)).all()
    assert (first[R.LATE[1]:R.LAST[0]] == R.NONE32).all() and R.LAST[0] - R.LATE[1] == 4
    assert (first[R.LAST[0]:R.LAST[1]] >= (n // 256) * 256).all() and R.LAST[1] == nn + 1
    starts = np.concatenate([[0], np.flatnonzero(f[1:] != f[:-1]) + 1])
    assert np.isin(first[1:R.LATE[1]], starts).all()
    assert (first[1:R.LATE[1]] % 64 != 0).any() and (first[1:R.LATE[1]] % 64 == 0).any()


# ---- the caps are the sources' ----------------------------------------------------------------------------------------------------
LAUNCH = re.compile(r"hipLaunchKernelGGL\(\(?(?:kh::)?(\w+)(?:<[^>]*>)?\)?,\s*(.*?),\s*dim3\((\d+)\),")


def launches(name):
    """kernel -> the set of grid expressions it is launched with in csrc/<name> (`kh::` dropped); every launch has 256 threads but
    the listed ones"""
    with open(os.path.join(CSRC, name)) as fh:
        text = fh.read()
    found = {}
    for kernel, grid, threads in LAUNCH.findall(text):
        assert int(threads) == R.THREADS or kernel in ("ccl_scan_kernel",) or (kernel, grid) == ("fill_u64_kernel", "dim3(1)"), kernel
        found.setdefault(kernel, set()).add(grid.replace("kh::", ""))
    return found, text


def log2(v):
    assert v & (v - 1) == 0
    return v.bit_length() - 1


def test_caps_of_points_hip():
    found, text = launches("points.hip")
    assert found["fill_u64_kernel"] == {"dim3(points_grid((nqueries + 255) / 256, %d))" % R.FILL_U64_BLOCKS, "dim3(1)"}
    assert found["nearest_kernel"] == {"dim3(grid)"}
    assert re.findall(r"const unsigned grid = points_grid\(ntiles, (\d+)\);", text) == [str(R.NEAREST_BLOCKS)]
    assert "const int64_t per_block = (ntiles + grid - 1) / grid;" in text and "(int)sz, per_block," in text
    assert found["binary_edge_count_kernel"] == {"dim3(points_grid((nvox + 255) / 256, %d))" % R.EDGE_COUNT_BLOCKS}
    assert found["binary_edge_emit_kernel"] == {"dim3(points_grid(ntiles, 1 << %d))" % log2(R.EDGE_EMIT_TILES)}
    assert text.count("const int64_t ntiles = ((sx + 255) / 256) * sy * sz;") == 2


def test_caps_of_feature_hip():
    found, text = launches("feature.hip")
    body = re.search(r"static inline unsigned blocks_for\(int64_t n\) \{(.*?)\n\}", text, re.S).group(1)
    assert "int64_t g = (n + 255) / 256;" in body
    assert re.findall(r"if \(g > (\d+)\) g = (\d+);", body) == [(str(R.FEATURE_BLOCKS),) * 2]
    assert "blocks_for_pieces(int64_t pieces) { return blocks_for(pieces * 64); }" in text
    assert text.count("wave = (int64_t)blockIdx.x * %d + (threadIdx.x >> 6), waves = (int64_t)gridDim.x * %d;"
                      % (R.WAVES_PER_BLOCK, R.WAVES_PER_BLOCK)) == 2
    assert found["geodesic_init_kernel"] == found["first_appearance_kernel"] == found["remap_u32_kernel"] == {"dim3(blocks_for(nvox))"}
    assert found["geodesic_seed_kernel"] == {"dim3(blocks_for(nseeds))"}
    assert found["box_shell_diff_kernel"] == found["first_appearance_box_kernel"] == {"dim3(blocks_for_pieces(c.pieces))"}


def test_caps_of_ccl_hip():
    found, text = launches("ccl.hip")
    assert re.findall(r"static inline unsigned ccl_grid\(int64_t n, int per_block, int64_t cap = (\d+)\)", text) == [str(R.CCL_BLOCKS)]
    by_tile = "dim3(ccl_grid(ntiles, 1, 1 << %d))" % log2(R.CCL_TILES)
    for kernel in ("reg_init_kernel", "reg_link_kernel", "reg_table_kernel", "reg_pairs_kernel", "fill_link_kernel", "cclg_link_kernel"):
        assert found[kernel] == {by_tile}, kernel
    for kernel in ("fill_init_kernel", "fill_mark_open_kernel", "fill_apply_kernel", "cclg_init_kernel"):
        assert found[kernel] == {"dim3(ccl_grid(n, 256))"}, kernel                        # the default cap
    assert found["reg_apply_kernel"] == {"dim3(ccl_grid(nvox, 256))"}
    assert found["edt_graph_cells_kernel"] == {"grid"} and "const dim3 grid(kh::ccl_grid(n, 256));" in text
    assert found["edt_graph_sample_kernel"] == {"dim3(ccl_grid(sx * sy * sz, 256))"}
    assert found["reg_apply_box_kernel"] == {"dim3(ccl_grid(nvox, 256, %d))" % R.APPLY_BOX_BLOCKS}
    assert text.count("const int64_t ntiles = ((sx + 255) / 256) * sy * sz;") >= 5
