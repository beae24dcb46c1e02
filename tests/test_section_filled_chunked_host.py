"""cross_sectional_area_filled_chunked without a GPU: the region graph of a dataset composed from its cores
(post.region_graph_chunked with fill_ref.region_graph per core) against fill_ref.region_graph and section_filled_ref.filled_mask on the
whole dataset, and the driver's bookkeeping with the statement of the filled box section (tests/section_filled_chunked_ref.py) in
place of the kernel against the statement on the whole dataset."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fill_ref  # noqa: E402
import section_box_ref as B  # noqa: E402
import section_filled_chunked_ref as H  # noqa: E402
import section_filled_ref  # noqa: E402
import section_ref  # noqa: E402


def graph_of(dataset, chunk=H.CORES, **kw):
    from kimimaro_amd import post
    return post.region_graph_chunked(dataset, chunk, _regions=H.regions_on_host, **kw)


def merged_volume(graph):
    """the merged region id of every voxel, from the store and the members"""
    merged = np.zeros(int(graph.bases[-1]) + 1, dtype=np.int64)
    counts = np.diff(graph.member_offsets)
    merged[graph.members] = np.repeat(np.arange(counts.size), counts)
    assert np.all(merged[1:] >= 1) and graph.member_offsets[1] == 0
    return merged[np.asarray(graph.store)]


def listed_voxels(graph, word):
    from kimimaro_amd import post
    ids, = post.hole_lists(graph, [word])
    assert ids.dtype == np.uint32 and np.all(np.diff(ids.astype(np.int64)) > 0) and not np.any(ids == 0)
    return np.isin(np.asarray(graph.store), ids), ids


def check_composition(whole):
    """the three statements of the issue; `whole` with three axes"""
    graph = graph_of(whole)
    value, count, face, pairs, region = fill_ref.region_graph(whole)
    mine = merged_volume(graph)
    assert graph.store.dtype == np.uint32 and np.all(np.asarray(graph.store) != 0)
    # the same partition: the pairs (mine, theirs) that occur are a bijection
    both = np.unique(np.stack([mine.reshape(-1), region.reshape(-1)], axis=1), axis=0)
    assert len(both) == len(np.unique(mine)) == len(np.unique(region)) == len(value) - 1 == len(graph.value) - 1
    theirs = np.zeros(len(graph.value), dtype=np.int64)
    theirs[both[:, 0]] = both[:, 1]
    assert np.array_equal(graph.value[1:], value[theirs[1:]]) and np.array_equal(graph.face[1:], face[theirs[1:]])
    a, b = theirs[(graph.pairs >> np.uint64(32)).astype(np.int64)], theirs[(graph.pairs & np.uint64(0xFFFFFFFF)).astype(np.int64)]
    assert len(np.unique(graph.pairs)) == len(graph.pairs)
    mapped = (np.minimum(a, b).astype(np.uint64) << np.uint64(32)) | np.maximum(a, b).astype(np.uint64)
    assert np.array_equal(np.sort(mapped), np.sort(pairs))
    # hole(L) for every label
    plain = whole.view(np.uint8) if whole.dtype == np.bool_ else whole
    for L in np.unique(plain).tolist():
        if L != 0:
            got, _ = listed_voxels(graph, L)
            assert np.array_equal(got, section_filled_ref.filled_mask(plain, L) & (plain != L)), L
    return graph


# ---- composition ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", range(36))
def test_composition_random(seed):
    check_composition(H.random_dataset(seed))


@pytest.mark.parametrize("name", ["x", "y", "z", "corner"])
def test_composition_straddling_shell(name):
    whole = H.straddling_shells()[name]
    graph = check_composition(whole)
    got, ids = listed_voxels(graph, 5)
    core_of = np.searchsorted(graph.bases, ids, side="left") - 1
    assert len(set(core_of.tolist())) == {"x": 2, "y": 2, "z": 2, "corner": 8}[name]          # the cavity has a piece in that many cores
    assert got.sum() == {"x": 5 * 4 * 3, "y": 5 * 5 * 3, "z": 5 * 4 * 5, "corner": 5 * 5 * 5}[name]


def test_composition_nested_shells():
    whole = H.nested_shells()
    graph = check_composition(whole)
    in3, in4 = listed_voxels(graph, 3)[0], listed_voxels(graph, 4)[0]
    assert np.all(in3[whole == 4]) and np.all(in3[whole == 6]) and np.all(in4[whole == 6]) and not np.any(in4[whole == 3])


def test_a_cavity_that_only_the_dataset_sees_closed():
    from kimimaro_amd import holes, plan
    whole = H.straddling_shells()["corner"]
    graph = graph_of(whole)
    got, ids = listed_voxels(graph, 5)
    cavity = np.zeros(H.SHAPE, dtype=bool)
    cavity[8:13, 6:11, 5:10] = True
    assert np.array_equal(got, cavity) and ids.size == 8                # one piece in each of the eight cores
    # no core sees it closed: on its own (every face of the core a face) no core lists a hole of 5
    core_lo, core_hi, _, _ = plan.halo_boxes(H.SHAPE, H.CORES, 0)
    for lo, hi in zip(core_lo, core_hi):
        core = whole[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]]
        _, value, _, face, pairs, _ = H.regions_on_host(core, 2, core.shape, 3, None, 63)
        assert holes.enclosed_regions(value, face, pairs, np.array([5], dtype=np.uint64))[1].size == 0


def test_a_tube_that_only_its_core_sees_closed():
    from kimimaro_amd import holes
    whole = H.open_tube()
    graph = check_composition(whole)
    got, ids = listed_voxels(graph, 7)
    assert ids.size == 0 and not got.any()
    # the first core, with the faces the sweep gives it (x = 9, y = 7 and z = 6 are cuts), lists the bore
    core = whole[:10, :8, :7]
    region, value, _, face, pairs, _ = H.regions_on_host(core, 2, core.shape, 3, None, 1 | 4 | 16)
    mine = holes.enclosed_regions(value, face, pairs, np.array([7], dtype=np.uint64))[1]
    bore = np.zeros(core.shape, dtype=bool)
    bore[3:, 3:6, 2:5] = True
    assert mine.size == 1 and np.array_equal(region == mine[0], bore)


def test_composition_disconnected_value_and_dtypes():
    whole = np.zeros(H.SHAPE, dtype=np.uint16, order="F")
    whole[H.box_walls(H.SHAPE, (1, 1, 1), (5, 5, 5))] = 4            # inside the first core
    whole[H.box_walls(H.SHAPE, (12, 10, 9), (18, 14, 12))] = 4       # inside the middle core
    whole[H.box_walls(H.SHAPE, (19, 15, 13), (23, 19, 17))] = 4      # across the cuts x = 20, y = 16, z = 14, on three faces ...
    whole[23, 17, 15] = 0                                            # ... and open there
    whole[21, 17, 15] = 8
    graph = check_composition(whole)
    assert listed_voxels(graph, 4)[0].sum() == 27 + 5 * 3 * 2          # the two closed shells' cavities
    big = np.asfortranarray(whole.astype(np.uint64) * np.uint64(2 ** 40 + 3))
    graph = check_composition(big)
    assert graph.value.dtype == np.uint64 and int(graph.value.max()) == 8 * (2 ** 40 + 3)
    check_composition(np.asfortranarray(whole == 4))


def test_extent_one_and_two_axes():
    from kimimaro_amd import post
    flat = np.zeros((24, 20), dtype=np.uint16, order="F")
    flat[3:15, 2:14] = 3
    flat[5:13, 4:12] = 0
    for whole in (flat, flat.reshape(24, 1, 20), flat.reshape(24, 20, 1)):
        graph = graph_of(whole, chunk=H.CORES[:whole.ndim] if whole.ndim == 2 else (10, 8, 7))
        assert np.all(graph.face[1:] == 1)
        assert all(ids.size == 0 for ids in post.hole_lists(graph, [3, 0]))
    check_composition(flat.reshape(24, 20, 1))


def test_region_store_as_a_memmap(tmp_path):
    whole = H.nested_shells()
    store = np.memmap(str(tmp_path / "regions.u32"), dtype=np.uint32, mode="w+", shape=H.SHAPE, order="F")
    a, b = graph_of(whole), graph_of(whole, region_store=store)
    assert b.store is store and np.array_equal(np.asarray(a.store), np.asarray(store))
    for name in ("value", "face", "pairs", "bases", "member_offsets", "members"):
        assert np.array_equal(getattr(a, name), getattr(b, name)), name
    with pytest.raises(ValueError):
        graph_of(whole, region_store=np.zeros(H.SHAPE, dtype=np.int64))
    with pytest.raises(ValueError):
        graph_of(whole, region_store=np.zeros((24, 20, 17), dtype=np.uint32))


def test_fewer_than_2_to_the_32_regions():
    from kimimaro_amd import post

    def many(core, label_bytes, shape, ndim, mark, faces):
        out = list(H.regions_on_host(core, label_bytes, shape, ndim, mark, faces))
        out[1] = np.broadcast_to(np.zeros(1, dtype=np.uint64), (2 ** 31 + 1,))     # "2^31 regions" in every core
        return tuple(out)

    with pytest.raises(ValueError, match="2\\^32"):
        post.region_graph_chunked(np.zeros(H.SHAPE, dtype=np.uint8), H.CORES, _regions=many)


# ---- the driver -------------------------------------------------------------------------------------------------------------------------

def whole_volume(lab, skels, labels):
    """the statement on the whole dataset: section_ref.single_skeleton on filled_mask(lab, L)"""
    out = {}
    for L in labels:
        sections = section_ref.SectionCache(section_filled_ref.filled_mask(lab, L), (1, 1, 1))
        out[L] = section_ref.single_skeleton(sections, lab.shape, skels[L].vertices, skels[L].edges, "voxel", True, (1, 1, 1))
    return out


def run(lab, skels, **kw):
    from kimimaro_amd import post
    fake, timings = H.FakeFilledSections(), {}
    out = post.cross_sectional_area_filled_chunked(lab, skels, chunk_shape=H.CORES, timings=timings, _sections=fake,
                                                   _regions=H.regions_on_host, **kw)
    assert out is skels
    return fake, timings


def test_driver_a_seed_in_a_hole_and_growth_rounds():
    lab, skels = H.room()
    fake, timings = run(lab, skels, halo=1)
    want = whole_volume(lab, skels, (5, 9))
    for L in (5, 9):
        assert skels[L].cross_sectional_area.tobytes() == want[L][0].tobytes()
        assert np.array_equal(skels[L].cross_sectional_area_contacts, want[L][1])
    assert np.all(skels[5].cross_sectional_area == 18 * 16) and np.all(skels[9].cross_sectional_area == 9)
    assert np.all(skels[77].cross_sectional_area == -1) and np.all(skels[77].cross_sectional_area_contacts == 0)
    # the box of the middle core at halo 1 holds no voxel of 5, and the seeds in it were run all the same
    middle = [c for c in fake.calls[:27] if c[0] == (9, 7, 6)]
    assert len(middle) == 1 and middle[0][1] == (12, 10, 9) and not np.any(lab[9:21, 7:17, 6:15] == 5)
    assert sum(1 for s in middle[0][2] if s is not None and lab[s] == 0) >= 3
    # rounds: halo 1, 2, 4, 8, 16 until the room's section fits
    first = timings["calls"][0]
    assert timings["cores"] == 27 and first["boxes"][0] == 27 and len(first["boxes"]) >= 4 and timings["items_rerun"] >= 19
    assert timings["capped_items"] == 0
    for name in ("regions_s", "seam_ms", "merge_s", "enclosed_ms", "provisional_regions", "merged_regions", "seam_pairs", "listed_ids"):
        assert name in timings, name
    assert timings["merged_regions"] == 4 and timings["provisional_regions"] >= 27 + 8 and timings["listed_ids"] >= 27


def test_driver_bit_64():
    lab, skels = H.room()
    fake, timings = run(lab, skels, halo=1, max_box_voxels=12 * 10 * 9)
    assert timings["capped_items"] >= 19 and np.all(skels[5].cross_sectional_area_contacts & 64)
    inside = (skels[5].vertices[:, 0] >= 10) & (skels[5].vertices[:, 0] < 20)
    assert np.all(skels[5].cross_sectional_area[inside] == 10 * 9)         # the whole y-z face of the box of round 0
    assert not np.any(skels[9].cross_sectional_area_contacts & 64) and np.all(skels[9].cross_sectional_area == 9)
    with pytest.raises(ValueError):
        run(lab, H.room()[1], halo=1, max_box_voxels=12 * 10 * 9 - 1)


def test_driver_lists_are_cut_down_to_the_cores_of_the_box():
    from kimimaro_amd import plan, post
    lab, skels = H.room()
    fake, _ = run(lab, skels, halo=1)
    graph = graph_of(lab)
    full, = post.hole_lists(graph, [5])
    core_lo, core_hi, _, _ = plan.halo_boxes(H.SHAPE, H.CORES, 0)
    shorter = 0
    for lo, ext, seeds, ids, begin, count in fake.calls:
        lo, hi = np.array(lo), np.array(lo) + np.array(ext)
        meets = np.all((core_lo < hi) & (core_hi > lo), axis=1)
        owner = np.searchsorted(graph.bases, ids, side="left") - 1
        assert np.all(meets[owner])
        mine = full[meets[np.searchsorted(graph.bases, full, side="left") - 1]]
        assert np.array_equal(np.sort(ids), mine)                      # (9 and 77 have no holes: the list is that of 5)
        # ... and nothing is lost: every listed region with a voxel in the box is there
        here = np.unique(np.asarray(graph.store)[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]])
        assert np.all(np.isin(np.intersect1d(here, full), ids))
        shorter += ids.size < full.size
    assert shorter >= 8 and any(c[3].size == full.size for c in fake.calls)


def test_driver_without_holes_equals_the_unfilled_driver():
    from kimimaro_amd import Skeleton, post
    flat = np.zeros((24, 20), dtype=np.uint16, order="F")
    flat[3:15, 2:14] = 3
    flat[5:13, 4:12] = 0
    ring = np.array([[x, 3] for x in range(4, 14)] + [[9, 8]])        # along the ring's side, and one vertex in its middle
    edges = np.array([[i, i + 1] for i in range(9)] + [[5, 10]])
    for whole in (flat, flat.reshape(24, 20, 1), flat.reshape(24, 1, 20)):
        chunk = (10, 8) if whole.ndim == 2 else tuple(min(c, s) for c, s in zip((10, 8, 8), whole.shape))
        verts = np.concatenate([ring, np.zeros((len(ring), 1), dtype=int)], axis=1)
        if whole.shape[1:] == (1, 20):
            verts = verts[:, [0, 2, 1]]
        a, b = (Skeleton(verts, edges, segid=3, space="voxel") for _ in range(2))
        post.cross_sectional_area_chunked(whole, a, chunk_shape=chunk, halo=2, _sections=B.FakeSections())
        fake = H.FakeFilledSections()
        post.cross_sectional_area_filled_chunked(whole, b, chunk_shape=chunk, halo=2, _sections=fake, _regions=H.regions_on_host)
        assert all(c[3].size == 0 and not c[5].any() for c in fake.calls) and len(fake.calls) >= 6
        assert a.cross_sectional_area.tobytes() == b.cross_sectional_area.tobytes() and np.any(a.cross_sectional_area > 0)
        assert np.array_equal(a.cross_sectional_area_contacts, b.cross_sectional_area_contacts)
        assert b.cross_sectional_area[10] == 0


def test_arguments_and_export():
    import kimimaro_amd
    from kimimaro_amd import post
    assert kimimaro_amd.cross_sectional_area_filled_chunked is post.cross_sectional_area_filled_chunked
    lab, skels = H.room()
    for halo in (0, -3, 1.5):
        with pytest.raises(ValueError):
            run(lab, skels, halo=halo)
    with pytest.raises(NotImplementedError):
        run(lab, skels, halo=2, visualize_section_planes=True)
    with pytest.raises(NotImplementedError, match="cross_sectional_area_filled_chunked"):
        post.cross_sectional_area_chunked(lab, skels, chunk_shape=H.CORES, halo=2, fill_holes=True, _sections=B.FakeSections())
    assert not hasattr(skels[5], "cross_sectional_area")
