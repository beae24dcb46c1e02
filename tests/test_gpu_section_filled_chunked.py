"""cross_sectional_area_filled_chunked on the MI355X: kh_region_seam_pairs against np.unique, kh_region_table_box
against numpy, kh_cross_sections_filled_box against kh_cross_sections_filled on the whole volume and against kh_cross_sections_box,
and the driver against cross_sectional_area_filled on a volume that fits.

Between two device runs areas are compared as bits (the same voxels are summed as integers of the same fixed point); sets of keys
and tables of small integers are compared for equality."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import section_box_ref as B  # noqa: E402
import section_filled_chunked_ref as H  # noqa: E402
from section_filled_chunked_ref import box_walls  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPE, CHUNK, HALO = (100, 20, 18), (70, 12, 10), 4
_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


# ---- kh_region_seam_pairs -----------------------------------------------------------------------------------------------------------

def seam_planes(kind, m):
    rng = np.random.default_rng(m)
    if kind == "equal":
        return np.full(m, 7, dtype=np.uint32), np.full(m, 9, dtype=np.uint32)
    if kind == "distinct":
        return rng.permutation(m).astype(np.uint32) + np.uint32(1), np.arange(m, dtype=np.uint32) + np.uint32(m + 1)
    if kind == "runs":                                   # long runs of equal neighbours, of unrelated lengths on the two sides
        return (np.arange(m) // 50 + 1).astype(np.uint32), (np.arange(m) // 37 + 100).astype(np.uint32)
    assert kind == "top"                                 # ids with the top bit set, up to 2^32 - 1
    low = (2 ** 31 + rng.integers(0, 5, size=m)).astype(np.uint32)
    high = (2 ** 32 - 1 - rng.integers(0, 5, size=m)).astype(np.uint32)
    high[-1] = 2 ** 32 - 1
    return low, high


def seam_call(eng, low, high, capacity):
    """one call of kh_region_seam_pairs -> (the keys in the table, state)"""
    from kimimaro_amd import _abi
    t = eng.torch
    d_low = t.from_numpy(low.view(np.int32)).to(eng.device)
    d_high = t.from_numpy(high.view(np.int32)).to(eng.device)
    d_table, d_state = eng.empty(capacity, t.int64), eng.empty(2, t.int32)
    _abi.check(eng.lib.kh_region_seam_pairs(eng.ptr(d_low), eng.ptr(d_high), low.size, eng.ptr(d_table), capacity, eng.ptr(d_state),
                                            eng.stream()))
    table = d_table.cpu().numpy().view(np.uint64)
    return table[table != 0], d_state.cpu().numpy().view(np.uint32)


def unique_keys(low, high):
    return np.unique((low.astype(np.uint64) << np.uint64(32)) | high.astype(np.uint64))


@pytest.mark.parametrize("kind", ["equal", "distinct", "runs", "top"])
@pytest.mark.parametrize("m", [1, 63, 64, 65, 70 * 12])
def test_seam_pairs_against_numpy(m, kind):
    from kimimaro_amd import ops
    eng = ops.engine()
    low, high = seam_planes(kind, m)
    want = unique_keys(low, high)
    keys, state = seam_call(eng, low, high, 4096)
    assert state[1] == 0 and state[0] == want.size and np.array_equal(np.sort(keys), want)
    t = eng.torch
    got, capacity, tries = eng.region_seam_pairs(t.from_numpy(low.view(np.int32)).to(eng.device),
                                                 t.from_numpy(high.view(np.int32)).to(eng.device))
    assert np.array_equal(np.sort(got), want) and tries == 1 and capacity >= 4 * m


def test_seam_pairs_report_a_table_that_is_too_small():
    from kimimaro_amd import _abi, ops
    eng = ops.engine()
    low, high = seam_planes("distinct", 70 * 12)
    want = unique_keys(low, high)
    assert want.size == 840
    keys, state = seam_call(eng, low, high, 512)         # 840 keys cannot go into 512 slots: the kernel says so, and writes no further
    assert state[1] != 0 and keys.size <= 512 and np.all(np.isin(keys, want))
    keys, state = seam_call(eng, low, high, 2048)        # the retry, 4 x larger
    assert state[1] == 0 and state[0] == 840 and np.array_equal(np.sort(keys), want)
    t = eng.torch
    got, capacity, tries = eng.region_seam_pairs(t.from_numpy(low.view(np.int32)).to(eng.device),
                                                 t.from_numpy(high.view(np.int32)).to(eng.device), capacity=512)
    assert np.array_equal(np.sort(got), want) and (capacity, tries) == (2048, 2)
    for bad in (0, 63, 96):
        assert eng.lib.kh_region_seam_pairs(1, 1, 4, 1, bad, 1, None) == 1 and "kh_region_seam_pairs" in _abi.last_error()


# ---- kh_region_table_box ------------------------------------------------------------------------------------------------------------

def blocky(sx):
    """values 0..2 in runs of three along x (a run crosses the 64-lane chunks), ragged in y and z"""
    rng = np.random.default_rng(sx)
    coarse = rng.integers(0, 3, size=(-(-sx // 3), 9, 7)).astype(np.uint16)
    return np.asfortranarray(np.repeat(coarse, 3, axis=0)[:sx])


@pytest.mark.parametrize("sx", [100, 30])
def test_region_table_box_against_numpy(sx):
    from kimimaro_amd import ops, utility
    eng = ops.engine()
    labels = blocky(sx)
    d_flat, itemsize, _, shape, _, _ = utility._device_labels(eng, labels)
    d_region, value, count, face, _, _ = eng.region_graph(d_flat, itemsize, shape, 3)
    region = d_region.cpu().numpy().view(np.uint32).reshape(shape, order="F")
    assert value.size - 1 == region.max() and value.size > 50
    for mask in (63, 1 | 4 | 16, 2 | 8 | 32, 8, 1, 0):   # every face (kh_region_table's), two corners of a dataset, one face, the interior
        d_again, v, c, f, _, _ = eng.region_graph(d_flat, itemsize, shape, 3, faces=mask)
        assert np.array_equal(d_again.cpu().numpy().view(np.uint32).reshape(shape, order="F"), region)
        want = np.zeros(value.size, dtype=np.uint8)
        for axis in range(3):
            for bit, index in ((1 << (2 * axis), 0), (2 << (2 * axis), -1)):
                if mask & bit:
                    want[np.unique(np.take(region, index, axis=axis))] = 1
        assert np.array_equal(v, value) and np.array_equal(c, count) and np.array_equal(f, want), mask
        assert c[1:].sum() == labels.size and np.array_equal(v[1:], labels.reshape(-1, order="F")[np.unique(region.reshape(-1, order="F"),
                                                                                                        return_index=True)[1]])
        if mask == 63:
            assert np.array_equal(f, face) and f.any() and not f.all()
        if mask == 0:
            assert not f.any()


# ---- the volume of the section tests ------------------------------------------------------------------------------------------------

def volume():
    """100 x 20 x 18, cores (70, 12, 10): label 5 a box wall whose cavity lies across x = 70, y = 12 and z = 10, with a blob of label 9
    in it; label 3 a shell inside the first core; label 7 a tube capped at x = 30 and open at the face x = 99, its wall on the faces
    y = 19 and z = 17"""
    def make():
        lab = np.zeros(SHAPE, dtype=np.uint16, order="F")
        lab[box_walls(SHAPE, (64, 3, 2), (78, 15, 12))] = 5
        lab[69:72, 8:11, 5:8] = 9
        lab[box_walls(SHAPE, (10, 2, 2), (20, 9, 8))] = 3
        lab[30:, 15:20, 13:18] = 7
        lab[31:, 16:19, 14:17] = 0
        return lab
    return cached("volume", make)


def skeletons():
    from kimimaro_amd import Skeleton
    line = lambda pts: (np.array(pts), np.array([[i, i + 1] for i in range(len(pts) - 1)]))
    parts = {5: line([[x, 9, 7] for x in range(64, 79)]),            # wall, cavity, blob, cavity, wall: through the straddling cavity
             3: line([[x, 5, 5] for x in range(10, 21)]),
             9: line([[69, 9, 6], [70, 9, 6], [71, 9, 6]]),
             7: line([[x, 15, 13] for x in range(35, 96, 3)])}
    return {k: Skeleton(v, e, segid=k, space="voxel") for k, (v, e) in parts.items()}


def items():
    """(seeds, normals, labels): the vertices of the skeletons, each with the x axis and with a random normal"""
    def make():
        rng = np.random.default_rng(11)
        seeds, normals, wants = [], [], []
        for k, s in skeletons().items():
            for v in s.vertices.astype(np.int64):
                for n in ((1.0, 0.0, 0.0), rng.normal(size=3)):
                    seeds.append(v), normals.append(n), wants.append(k)
        return np.array(seeds), np.array(normals, dtype=np.float64), np.array(wants)
    return cached("items", make)


def dataset_graph():
    """region_graph_chunked on the device and the lists of the four labels, provisional ids"""
    def make():
        from kimimaro_amd import post
        timings = {}
        graph = post.region_graph_chunked(volume(), CHUNK, timings=timings)
        print(timings)
        assert timings["cores"] == 8 and timings["merged_regions"] < timings["provisional_regions"] and timings["seam_pairs"] >= 8
        return graph, dict(zip((5, 3, 9, 7), post.hole_lists(graph, [5, 3, 9, 7])))
    return cached("graph", make)


def test_dataset_graph_lists_the_straddling_cavity():
    from section_filled_ref import filled_mask
    graph, lists = dataset_graph()
    lab = volume()
    for L, ids in lists.items():
        assert np.array_equal(np.isin(graph.store, ids), filled_mask(lab, L) & (lab != L)), L
    assert lists[5].size >= 9 and lists[3].size == 1 and lists[9].size == 0 and lists[7].size == 0


def device_whole(seeds, normals, wants):
    def make():
        from kimimaro_amd import ops, section, utility
        eng = ops.engine()
        d_flat, itemsize, _, shape, _, _ = utility._device_labels(eng, volume())
        d_region, word_range, d_list = section.hole_tables(eng, d_flat, itemsize, shape, set(int(w) for w in wants))
        ranges = np.array([word_range[int(w)] for w in wants], dtype=np.uint32).reshape(-1, 2)
        return section.cross_sections(eng, d_flat, itemsize, shape, (1, 1, 1), section.seed_index(seeds, shape), wants.astype(np.uint32),
                                      normals, filled=(d_region, ranges[:, 0], ranges[:, 1], d_list))
    return cached("whole", make)


def device_boxes(seeds, normals, wants, chunk, halo, holes=True, plain=False):
    """every item in the box of its core: kh_cross_sections_filled_box with the box of the store and the whole lists, with empty
    lists (holes=False), or kh_cross_sections_box (plain) -> (area, contact, clip, voxels)"""
    from kimimaro_amd import ops, section, utility
    eng = ops.engine()
    t = eng.torch
    graph, lists = dataset_graph()
    labels = volume()
    order = sorted(lists)
    begin = np.cumsum([0] + [lists[k].size for k in order])
    d_list = t.from_numpy(np.concatenate([lists[k] for k in order]).view(np.int32)).to(eng.device)
    at = np.array([order.index(int(w)) for w in wants])
    n = len(seeds)
    out = np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint32)
    boxes = np.array([B.halo_box(s, chunk, halo, labels.shape) for s in seeds])
    for lo, hi in sorted({(tuple(b[0]), tuple(b[1])) for b in boxes.tolist()}):
        sel = np.flatnonzero(np.all(boxes[:, 0] == lo, axis=1) & np.all(boxes[:, 1] == hi, axis=1))
        cut = tuple(slice(a, b) for a, b in zip(lo, hi))
        d_flat, itemsize, _, shape, _, _ = utility._device_labels(eng, np.asfortranarray(labels[cut]))
        seed = section.seed_index(seeds[sel] - np.array(lo), shape)
        if plain:
            got = section.cross_sections_box(eng, d_flat, itemsize, lo, shape, labels.shape, (1, 1, 1), seed, wants[sel].astype(np.uint32),
                                             normals[sel])
        else:
            d_region = t.from_numpy(np.asfortranarray(graph.store[cut]).reshape(-1, order="F").view(np.int32)).to(eng.device)
            count = (begin[at[sel] + 1] - begin[at[sel]]) * (1 if holes else 0)
            got = section.cross_sections_filled_box(eng, d_flat, itemsize, lo, shape, labels.shape, (1, 1, 1), seed,
                                                    wants[sel].astype(np.uint32), normals[sel], (d_region, begin[at[sel]], count, d_list))
        for a, g in zip(out, got):
            a[sel] = g
    return out


def test_filled_box_equal_to_the_volume():
    seeds, normals, wants = items()
    w_area, w_contact, w_voxels = device_whole(seeds, normals, wants)
    area, contact, clip, voxels = device_boxes(seeds, normals, wants, SHAPE, 1)
    assert np.all(clip == 0) and np.array_equal(voxels, w_voxels) and np.array_equal(contact, w_contact)
    assert area.tobytes() == w_area.tobytes()
    in_hole = volume()[tuple(seeds.T)] != wants
    assert in_hole.sum() >= 20 and np.all(voxels[in_hole & (wants == 5)] > 0) and np.all(voxels[wants == 7] > 0)


def test_filled_box_equals_the_volume_where_nothing_is_clipped():
    seeds, normals, wants = items()
    w_area, w_contact, w_voxels = device_whole(seeds, normals, wants)
    area, contact, clip, voxels = device_boxes(seeds, normals, wants, CHUNK, HALO)
    free = clip == 0
    print("clipped: %d of %d" % ((~free).sum(), free.size))
    assert free.sum() >= 10 and (~free).sum() >= 10
    assert np.array_equal(voxels[free], w_voxels[free]) and np.array_equal(contact[free], w_contact[free])
    assert area[free].tobytes() == w_area[free].tobytes()
    assert np.all(voxels[~free] <= w_voxels[~free]) and np.all(voxels[~free] > 0)
    # a seed in a hole of its label, in a box of round 0, with a section that no cut clips
    in_hole = volume()[tuple(seeds.T)] != wants
    assert np.any(free & in_hole & (voxels > 0))


def test_filled_box_without_holes_is_the_box_kernel():
    seeds, normals, wants = items()
    got = device_boxes(seeds, normals, wants, CHUNK, HALO, holes=False)
    want = device_boxes(seeds, normals, wants, CHUNK, HALO, plain=True)
    assert got[0].tobytes() == want[0].tobytes() and all(np.array_equal(a, b) for a, b in zip(got[1:], want[1:]))
    assert np.any(want[3] > 0) and np.any(want[3] == 0)


# ---- the driver against the whole volume --------------------------------------------------------------------------------------------

def assert_same_sections(got, want):
    assert list(got) == list(want)
    for k in want:
        a, b = got[k], want[k]
        assert a.cross_sectional_area.dtype == np.float32 and a.cross_sectional_area_contacts.dtype == np.uint8
        assert a.cross_sectional_area.tobytes() == b.cross_sectional_area.tobytes(), k
        assert np.array_equal(a.cross_sectional_area_contacts, b.cross_sectional_area_contacts), k
        ids = [p["id"] for p in a.extra_attributes]
        assert ids.count("cross_sectional_area") == 1 and ids.count("cross_sectional_area_contacts") == 1


def test_driver_equals_cross_sectional_area_filled():
    import kimimaro_amd
    want = kimimaro_amd.cross_sectional_area_filled(volume(), skeletons())
    mine, timings = skeletons(), {}
    out = kimimaro_amd.cross_sectional_area_filled_chunked(volume(), mine, chunk_shape=CHUNK, halo=HALO, timings=timings)
    print(timings)
    assert out is mine
    assert_same_sections(mine, want)
    # through the straddling cavity: every vertex of skeleton 5 has the section of the filled box wall, 13 x 11 voxels
    assert np.all(mine[5].cross_sectional_area == 13 * 11) and np.all(mine[3].cross_sectional_area == 8 * 7)
    assert np.all(mine[7].cross_sectional_area == 5 * 5 - 3 * 3) and np.all(mine[7].cross_sectional_area_contacts == 8 | 32)
    plain = kimimaro_amd.cross_sectional_area_chunked(volume(), skeletons(), chunk_shape=CHUNK, halo=HALO)
    assert np.sum(plain[5].cross_sectional_area == 0) >= 10            # (unfilled, the vertices in the cavity have no section)
    assert timings["cores"] == 8 and timings["calls"][0]["boxes"][0] == 8 and timings["items_rerun"] >= 1 and timings["capped_items"] == 0
    assert timings["merged_regions"] < timings["provisional_regions"] and timings["listed_ids"] >= 10 and timings["seam_ms"] > 0
    # once more on top of the values, as a second volume and a repair would
    again = kimimaro_amd.cross_sectional_area_filled(volume(), want, multipass=True, repair_contacts=True)
    kimimaro_amd.cross_sectional_area_filled_chunked(volume(), mine, chunk_shape=CHUNK, halo=HALO, multipass=True, repair_contacts=True)
    assert_same_sections(mine, again)


def test_driver_eight_byte_labels_and_a_box_without_the_label():
    """the room of the host tests with labels above 2^40: the box of the middle core at halo 1 lies inside the room and holds no voxel
    of its wall, whose renumbered labels then have no word for it; the seeds in it are in the wall's hole all the same"""
    import kimimaro_amd
    from kimimaro_amd import Skeleton
    lab, skels = H.room()
    big = np.asfortranarray(lab.astype(np.uint64) * np.uint64(2 ** 40 + 1))
    assert not np.any(big[9:21, 7:17, 6:15] == 5 * (2 ** 40 + 1))
    fresh = lambda: {k: Skeleton(s.vertices.copy(), s.edges.copy(), segid=k * (2 ** 40 + 1), space="voxel") for k, s in skels.items()}
    want = kimimaro_amd.cross_sectional_area_filled(big, fresh())
    mine, timings = fresh(), {}
    kimimaro_amd.cross_sectional_area_filled_chunked(big, mine, chunk_shape=H.CORES, halo=1, timings=timings)
    print(timings)
    assert_same_sections(mine, want)
    assert np.all(mine[5].cross_sectional_area == 18 * 16) and np.all(mine[9].cross_sectional_area == 9)
    assert np.all(mine[77].cross_sectional_area == -1) and timings["cores"] == 27 and timings["items_rerun"] >= 19
