"""The voxel connectivity graph without a GPU: tests/graph_ref.py against the builder the graph tests have used so
far, its clip rule box by box, the rules of `merges`, and the host pieces of the product that restate them (ops.merge_pairs,
boxes.clip_graph, boxes.GRAPH_STEP_OF_BIT)."""
import numpy as np
import pytest

import graph_ref as G
from kimimaro_amd import boxes, ops
from kimimaro_amd.plan import chunk_grid
from prep_ref import CC3D_STEP_OF_BIT

MERGES = [(5, 2), (1, 2), (2, 1), (3, 3), (0, 4), (6, 7), (2, 5)]      # unsorted, duplicates, a self pair, a pair with 0


def random_labels(shape, top, seed, dtype=np.uint32):
    return np.asfortranarray(np.random.default_rng(seed).integers(0, top + 1, size=shape).astype(dtype))


def test_graph_of_is_the_graph_of_labels_of_the_graph_tests():
    from test_gpu_graph import graph_of_labels
    assert boxes.GRAPH_STEP_OF_BIT == CC3D_STEP_OF_BIT                         # the product and this statement read one layout
    lab = random_labels((17, 11, 6), 2, 0)
    want = graph_of_labels(lab)
    got = G.graph_of(lab, 26, None)
    assert got.dtype == np.uint32 and got.flags.f_contiguous and want.any()
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(G.graph_of(lab, 6, None), want & np.uint32(0x3F))
    np.testing.assert_array_equal(G.graph_of(lab, 18, None), want & np.uint32(0x3FFFF))
    assert not (got >> np.uint32(26)).any()
    assert got[3, 3, 3] & 1 == int(lab[3, 3, 3] == lab[4, 3, 3])               # bit 0 is the step towards +x
    # background joins background: a volume of zeros allows every step that stays inside
    np.testing.assert_array_equal(G.graph_of(np.zeros((3, 3, 3), np.uint8))[1, 1, 1], 0x3FFFFFF)
    assert G.graph_of(np.zeros((1, 1, 1), np.uint8))[0, 0, 0] == 0
    # two axes: a unit z axis inside, two axes back, no step along z
    flat = G.graph_of(lab[:, :, 0])
    assert flat.shape == lab.shape[:2]
    np.testing.assert_array_equal(flat, G.graph_of(lab[:, :, :1])[:, :, 0])
    assert not (flat & np.uint32(0x3FFFC30)).any()


@pytest.mark.parametrize("merges", [None, MERGES])
def test_the_clipped_slice_is_the_graph_of_the_box(merges):
    lab = random_labels((50, 37, 9), 7, 1)
    whole = G.graph_of(lab, 26, merges)
    grid = chunk_grid(lab.shape, (24, 16, 8))
    assert grid.box_lo.shape[0] == 3 * 3 * 1                                   # (z: 9 planes are one box of 8 and its overlap plane)
    differ = 0
    for lo, hi in zip(grid.box_lo, grid.box_hi):
        cut = tuple(slice(int(a), int(b)) for a, b in zip(lo, hi))
        want = G.graph_of(lab[cut], 26, merges)
        np.testing.assert_array_equal(G.clip(whole[cut]), want)
        np.testing.assert_array_equal(boxes.clip_graph(whole[cut]), want)      # the product's clip is the same function
        differ += int(np.count_nonzero(whole[cut] != want))
    assert differ > 1000                                                        # the slices do carry bits that leave their box
    np.testing.assert_array_equal(G.clip(whole), whole)
    assert boxes.clip_graph(whole).flags.f_contiguous and boxes.clip_graph(whole).dtype == np.uint32
    np.testing.assert_array_equal(boxes.clip_graph(np.full((1, 1, 1), 0xFFFFFFFF, np.uint32)), [[[0xFC000000]]])   # (bits 26..31 are not its business)


def test_merges_join_as_listed_and_nothing_more():
    row = np.array([1, 2, 3, 1, 0, 4, 4, 5], dtype=np.uint16).reshape(8, 1, 1)
    px = lambda g: [int(v) & 1 for v in g[:, 0, 0]]                             # the +x bit along the row
    assert px(G.graph_of(row)) == [0, 0, 0, 0, 0, 1, 0, 0]
    assert px(G.graph_of(row, 26, [(1, 2), (2, 3)])) == [1, 1, 0, 0, 0, 1, 0, 0]      # 1-2 and 2-3 join; 3-1 does not: no closure
    assert px(G.graph_of(row, 26, [(3, 1)])) == [0, 0, 1, 0, 0, 1, 0, 0]               # either order names the pair
    assert px(G.graph_of(row, 26, [(0, 1), (4, 0)])) == px(G.graph_of(row))           # a pair with 0 is dropped
    assert px(G.graph_of(row, 26, [(5, 5)])) == px(G.graph_of(row))                   # so is a self pair
    lab = random_labels((9, 8, 7), 7, 2)
    tidy = [(1, 2), (2, 5), (6, 7)]
    assert G.pair_list(MERGES) == tidy and ops.merge_pairs(MERGES, (0, 255), 1).tolist() == [list(p) for p in tidy]
    np.testing.assert_array_equal(G.graph_of(lab, 26, MERGES), G.graph_of(lab, 26, tidy))
    assert (G.graph_of(lab, 26, tidy) != G.graph_of(lab)).any()
    # symmetric: the step back is allowed exactly where the step there is
    g = G.graph_of(lab, 26, tidy)
    for u, v in (((2, 3, 4), (3, 4, 5)), ((5, 5, 5), (5, 4, 5)), ((0, 0, 0), (1, 0, 0))):
        assert G.allowed_step(g, u, v) == G.allowed_step(g, v, u)
    assert not G.allowed_step(g, (0, 0, 0), (2, 0, 0)) and not G.allowed_step(g, (0, 0, 0), (0, 0, 0))


def test_merge_pairs_is_the_table_of_the_pair_list():
    for dtype in (np.uint8, np.uint16, np.int32, np.uint64):
        info = np.iinfo(dtype)
        table = ops.merge_pairs(MERGES, (int(info.min), int(info.max)), np.dtype(dtype).itemsize)
        assert table.dtype == np.uint64 and table.tolist() == [list(p) for p in G.pair_list(MERGES)]
    for empty in (None, [], np.zeros((0, 2), np.int64)):
        assert ops.merge_pairs(empty, (0, 255), 1).shape == (0, 2)
    assert ops.merge_pairs([(0, 3), (4, 4)], (0, 255), 1).shape == (0, 2)
    # signed labels are compared as their bit patterns: -1 in four bytes is 0xFFFFFFFF, and rows sort by the words
    got = ops.merge_pairs([(-1, 5), (7, -2)], (-2 ** 31, 2 ** 31 - 1), 4)
    assert got.tolist() == [[5, 0xFFFFFFFF], [7, 0xFFFFFFFE]]
    assert ops.merge_pairs([(-1, 5)], (-2 ** 63, 2 ** 63 - 1), 8).tolist() == [[5, 0xFFFFFFFFFFFFFFFF]]
    big = np.array([[2 ** 63 + 1, 1]], dtype=np.uint64)
    assert ops.merge_pairs(big, (0, 2 ** 64 - 1), 8).tolist() == [[1, 2 ** 63 + 1]]
    for bad in ([1, 2, 3], [[1, 2, 3]], [[[1, 2]]], [(1.5, 2.0)], [(1, 256)], [(-1, 2)]):
        with pytest.raises(ValueError):
            ops.merge_pairs(bad, (0, 255), 1)
    with pytest.raises(ValueError):
        ops.merge_pairs([(1, 2)], (0, 1), 1)                                    # bool labels hold 0 and 1


def test_the_product_reads_the_same_layout():
    assert boxes.GRAPH_STEP_OF_BIT == CC3D_STEP_OF_BIT
    assert boxes.graph_side_bits(0, 1) == sum(1 << b for b, s in enumerate(CC3D_STEP_OF_BIT) if s[0] == 1) == 0x1544541
    g = np.full((4, 3, 2), 0x3FFFFFF, dtype=np.uint32)
    np.testing.assert_array_equal(boxes.clip_graph(g), G.clip(g))
    np.testing.assert_array_equal(G.wall(g, 1, 0)[:, 0, :] & np.uint32(1 << 2), 0)
