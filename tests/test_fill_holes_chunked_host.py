"""fill_all_holes_chunked without a GPU: the driver with its two hooks on the host (region_graph_chunked on
fill_ref.region_graph per core, the painting by fill_ref.owner_volume) against fill_ref.static of the whole dataset -- the volume, the
fill count and the state of every label, all exact --, its forms of dataset and `out`, its refusals, and
skeletonize_chunked(fill_holes_global=True) on the CPU oracle."""
import numpy as np
import pytest

import chunked_ref as R
import fill_chunked_ref as F
import fill_ref
import section_filled_chunked_ref as H
from kimimaro_amd import _abi, post
from kimimaro_amd.volume import DimensionError

SEEDS = range(24)


def filled(dataset, chunk_shape=H.CORES, **kwargs):
    """the in-place run on a copy, held against fill_ref.static -> (volume, count, stats, what fill_ref.static says)"""
    mine, stats = np.array(dataset, copy=True, order="F"), {}
    got, count = F.fill_on_host(mine, chunk_shape, return_fill_count=True, stats=stats, **kwargs)
    assert got is mine
    return got, count, stats, F.assert_same_fill(got, count, stats, dataset)


# -- the definition ----------------------------------------------------------------------------------------------------------------
def test_random_datasets_equal_the_whole_and_are_no_empty_cases():
    with_fill = with_killed = differ = 0
    for seed in SEEDS:
        dataset = H.random_dataset(seed)
        got, count, stats, want = filled(dataset)
        with_fill += count > 0
        with_killed += any(bits & fill_ref.KILLED for bits in want[2].values())
        differ += not np.array_equal(F.by_cores(dataset), want[0])
        assert stats["cores"] == 27 and stats["merged_regions"] <= stats["provisional_regions"]
        assert (stats["cores_painted"] > 0) == (count > 0)
    print("of 24 seeds: %d with a fill, %d with a killed label, %d differ from core-by-core filling" % (with_fill, with_killed, differ))
    assert with_fill >= 15 and with_killed >= 12 and differ >= 12         # (20, 18 and 19 when this was written)


@pytest.mark.parametrize("name", ["x", "y", "z", "corner"])
def test_a_cavity_across_a_cut_is_filled(name):
    dataset = H.straddling_shells()[name]
    got, count, stats, _ = filled(dataset)
    assert count > 0 and np.all(got[dataset == 0][got[dataset == 0] != 0] == 5)
    assert not np.array_equal(F.by_cores(dataset), got)                   # each core sees an open cavity
    assert states_of(stats) == {5: _abi.HOLES_PROCESSED | _abi.HOLES_FILLED}
    assert 0 < stats["cores_painted"] < stats["cores"]


def states_of(stats):
    return F.states(stats)


def test_nested_shells_and_the_double_count():
    dataset = H.nested_shells()
    got, count, stats, _ = filled(dataset)
    assert count == int(np.count_nonzero(got != dataset))                 # 3 fills everything at its turn: 4 and 6 never get theirs
    assert states_of(stats) == {3: 3, 4: _abi.HOLES_KILLED, 6: _abi.HOLES_KILLED}
    assert not np.array_equal(F.by_cores(dataset), got)
    swapped = F.swapped_nested_shells()
    got, count, stats, _ = filled(swapped)
    assert (count, int(np.count_nonzero(got != swapped))) == (466, 396)  # 3 fills first, 4 paints over it: those voxels count twice
    assert states_of(stats) == {3: 3 | _abi.HOLES_KILLED, 4: 3, 6: _abi.HOLES_KILLED}


def test_a_tube_open_at_a_face_of_the_dataset_is_not_filled():
    dataset = H.open_tube()
    got, count, stats, _ = filled(dataset)
    assert count == 0 and np.array_equal(got, dataset) and stats["cores_painted"] == 0
    assert np.array_equal(F.by_cores(dataset), dataset)                   # (a core's own faces leave the bore open as well)


def test_bool_and_eight_byte_labels():
    got, count, stats, _ = filled(F.bool_dataset())
    assert got.dtype == np.bool_ and count > 0 and states_of(stats) == {1: 3}
    dataset = F.uint64_dataset()
    got, count, stats, _ = filled(dataset)
    # unsigned words: 7 comes first and kills 2^40, the label above 2^63 comes last and paints over both
    assert states_of(stats) == {7: 3 | _abi.HOLES_KILLED, 2 ** 40: _abi.HOLES_KILLED, F.BIG: 3}
    assert count > int(np.count_nonzero(got != dataset)) and set(np.unique(got).tolist()) == {0, F.BIG}


def test_two_axes_are_an_image_and_a_unit_axis_is_all_faces():
    ring = F.ring_2d()
    got, count, stats, _ = filled(ring, F.CORES_2D)
    assert got.shape == ring.shape and count == 7 * 6 and np.all(got[7:14, 5:11] == 9)
    assert states_of(stats) == {2: 1 | _abi.HOLES_KILLED, 9: 3} and stats["cores"] == 9
    got, count, _, _ = filled(ring, F.CORES_2D + (1,))                   # three entries are accepted for two axes
    assert count == 42
    flat = F.flat_dataset()
    got, count, stats, _ = filled(flat, F.CORES_2D + (1,))
    assert count == 0 and np.array_equal(got, flat) and states_of(stats) == {2: 1, 9: 1}
    # region_graph_chunked on its own keeps today's rule: the ends of a unit z axis are faces
    assert post.region_graph_chunked(ring, F.CORES_2D, _regions=H.regions_on_host).face[1:].all()
    graph, voxels = post.region_graph_chunked(ring, F.CORES_2D, _regions=H.regions_on_host, face_axes=2, return_counts=True)
    assert not graph.face[1:].all() and voxels.dtype == np.int64 and voxels[0] == 0 and voxels.sum() == ring.size
    assert sorted(voxels[1:].tolist()) == sorted(np.bincount(fill_ref.region_graph(ring)[4].reshape(-1))[1:].tolist())


# -- out= and the forms of the dataset ---------------------------------------------------------------------------------------------
def test_out_leaves_the_dataset_alone_and_equals_the_run_in_place():
    for dataset in (H.random_dataset(4), H.straddling_shells()["corner"], F.ring_2d()):
        chunk = H.CORES[:dataset.ndim]
        want = filled(dataset, chunk)[0]
        before = dataset.copy()
        out = np.full(dataset.shape, 77, dtype=dataset.dtype)             # (C order, and every voxel has to be written)
        got, count = F.fill_on_host(dataset, chunk, out=out, return_fill_count=True)
        assert got is out and np.array_equal(out, want) and np.array_equal(dataset, before)
        assert F.fill_on_host(dataset.copy(), chunk).dtype == dataset.dtype              # without the count: the volume alone


class Recording:
    """a dataset that takes slices only and notes every write"""

    def __init__(self, array):
        self.array, self.shape, self.written = array, array.shape, []

    def __getitem__(self, key):
        assert isinstance(key, tuple) and all(isinstance(s, slice) for s in key)
        return self.array[key].copy()

    def __setitem__(self, key, value):
        assert isinstance(key, tuple) and all(isinstance(s, slice) for s in key)
        self.written.append(key)
        self.array[key] = value


def test_an_in_place_run_writes_only_the_cores_it_paints():
    for dataset in (H.straddling_shells()["x"], H.random_dataset(2)):
        want = fill_ref.static(dataset)[0]
        changed = [cut for cut in F.core_slices(dataset.shape, H.CORES) if np.any(want[cut] != dataset[cut])]
        rec, stats = Recording(dataset.copy()), {}
        assert F.fill_on_host(rec, stats=stats) is rec and np.array_equal(rec.array, want)
        assert sorted(rec.written, key=str) == sorted(changed, key=str) and 0 < len(changed) < 27
        assert stats["cores_painted"] == len(changed)
    rec = Recording(H.open_tube())
    F.fill_on_host(rec)
    assert rec.written == []


def test_memmap_and_sliced_datasets(tmp_path):
    dataset = H.random_dataset(10)
    want = fill_ref.static(dataset)
    assert want[1] > 0
    mm = np.memmap(str(tmp_path / "labels.bin"), dtype=dataset.dtype, mode="w+", shape=dataset.shape, order="F")
    mm[...] = dataset
    store = np.memmap(str(tmp_path / "regions.bin"), dtype=np.uint32, mode="w+", shape=dataset.shape, order="F")
    got, count = F.fill_on_host(mm, region_store=store, return_fill_count=True)
    assert got is mm and count == want[1] and np.array_equal(mm, want[0]) and store.min() >= 1

    class Sliced:
        """the h5py / zarr form: a shape and __getitem__ over a tuple of slices, nothing else"""
        shape = dataset.shape

        def __getitem__(self, key):
            assert isinstance(key, tuple) and len(key) == 3 and all(isinstance(s, slice) for s in key)
            return dataset[key].copy()

    out = np.memmap(str(tmp_path / "filled.bin"), dtype=dataset.dtype, mode="w+", shape=dataset.shape, order="F")
    assert F.fill_on_host(Sliced(), out=out) is out and np.array_equal(out, want[0])
    assert np.array_equal(F.fill_on_host(np.ascontiguousarray(dataset)), want[0])


# -- refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals():
    dataset = H.straddling_shells()["x"]
    for bad in (np.zeros((24, 20, 17), np.uint16), np.zeros(H.SHAPE, np.uint32), np.zeros(H.SHAPE[:2], np.uint16)):
        with pytest.raises(ValueError, match="out"):
            F.fill_on_host(dataset.copy(), out=bad)
    for bad in (np.zeros((24, 20, 17), np.uint32), np.zeros(H.SHAPE, np.int64)):
        with pytest.raises(ValueError, match="region_store"):
            F.fill_on_host(dataset.copy(), region_store=bad)
    for shape in ((24,), (6, 5, 4, 3)):
        with pytest.raises(DimensionError, match="fill_all_holes_chunked"):
            F.fill_on_host(np.zeros(shape, np.uint8), (4,) * len(shape))
    with pytest.raises(TypeError):
        F.fill_on_host(np.zeros(H.SHAPE, np.float32))
    with pytest.raises(ValueError, match="come together"):
        post.fill_all_holes_chunked(dataset.copy(), H.CORES, _regions=H.regions_on_host)
    with pytest.raises(ValueError, match="come together"):
        post.fill_all_holes_chunked(dataset.copy(), H.CORES, _apply=F.apply_on_host)


def test_counts_are_summed_in_64_bits_and_refused_only_where_they_matter():
    def heavy(core, *args):
        """every piece of a region weighs 2^31 voxels"""
        region, value, count, face, pairs, info = H.regions_on_host(core, *args)
        return region, value, np.where(count > 0, 2 ** 31, 0).astype(np.uint32), face, pairs, info

    graph, voxels = post.region_graph_chunked(H.open_tube(), H.CORES, _regions=heavy, return_counts=True)
    assert voxels.dtype == np.int64 and voxels.max() >= 2 ** 32 and voxels.sum() == 2 ** 31 * int(graph.bases[-1])
    # every region of the tube owns a face of the dataset: none is ever painted, its count is clamped
    mine = H.open_tube()
    got, count = post.fill_all_holes_chunked(mine, H.CORES, return_fill_count=True, _regions=heavy, _apply=F.apply_on_host)
    assert count == 0 and np.array_equal(got, H.open_tube())
    # the cavity of the shell lies in two cores and owns no face: 2^32 voxels cannot be handed to the resolver
    with pytest.raises(ValueError, match="2\\^32"):
        post.fill_all_holes_chunked(H.straddling_shells()["x"].copy(), H.CORES, _regions=heavy, _apply=F.apply_on_host)


def test_no_cpu_fallback_without_the_hooks():
    import torch
    import kimimaro_amd
    from kimimaro_amd import region_boxes
    assert kimimaro_amd.fill_all_holes_chunked is post.fill_all_holes_chunked is region_boxes.fill_all_holes_chunked
    assert post.fill_all_holes_chunked.__module__ == "kimimaro_amd.region_boxes"
    if torch.cuda.is_available():
        return
    with pytest.raises(kimimaro_amd.HipUnavailableError):
        kimimaro_amd.fill_all_holes_chunked(H.open_tube(), H.CORES)
    with pytest.raises(kimimaro_amd.HipUnavailableError):
        kimimaro_amd.skeletonize_chunked(H.open_tube(), H.CORES, fill_holes_global=True, merge=False, _skeletonize=oracle_run)


# -- skeletonize_chunked(fill_holes_global=True) on the oracle ----------------------------------------------------------------------
CHUNK = (32, 40, 30)


def walled_dataset():
    """label 5: a block with a cavity across the cut x = 32; label 9: a rod in the cavity, on the low side of the cut; label 3: a rod
    outside.  Filled, 9 is gone."""
    lab = np.zeros((64, 40, 30), dtype=np.uint16, order="F")
    lab[8:56, 6:34, 4:26] = 5
    lab[20:44, 14:26, 10:20] = 0
    lab[22:31, 18:21, 13:16] = 9
    lab[2:6, 4:36, 10:14] = 3
    return lab


def oracle_run(labels, **kwargs):
    from oracle import pipeline as P
    return P.skeletonize(labels, **kwargs)


def host_postprocess(skeletons, dust_threshold, tick_threshold):
    return [post.postprocess(s, dust_threshold, tick_threshold) for s in skeletons]


def host_fill(dataset, chunk_shape, **kwargs):
    return F.fill_on_host(dataset, chunk_shape, **kwargs)


def test_skeletonize_chunked_on_the_globally_filled_dataset():
    dataset = walled_dataset()
    before = dataset.copy()
    seen = []

    def run(labels, **kwargs):
        seen.append(kwargs["fill_holes"])
        return oracle_run(labels, **kwargs)

    kw = dict(teasar_params=R.TP, anisotropy=R.AN, dust_threshold=20, post_dust_threshold=0, tick_threshold=0, _skeletonize=run,
              _postprocess=host_postprocess)
    plain = post.skeletonize_chunked(dataset, CHUNK, **kw)
    assert set(plain) == {3, 5, 9} and seen == [False, False]
    want_volume, want_count, _ = fill_ref.static(dataset)
    assert want_count == 24 * 12 * 10 and not np.any(want_volume == 9)
    assert np.any(F.by_cores(dataset, CHUNK) == 9)                        # box by box the cavity is open: the rod survives
    want = post.skeletonize_chunked(want_volume, CHUNK, fill_holes=False, **kw)
    del seen[:]
    timings = {}
    got = post.skeletonize_chunked(dataset, CHUNK, fill_holes=True, fill_holes_global=True, _fill=host_fill, timings=timings, **kw)
    assert seen == [False, False] and np.array_equal(dataset, before)
    R.assert_same(got, want)
    assert set(got) == {3, 5}
    assert set(timings) == {"count_s", "chunks_s", "place_s", "fuse_s", "post_s", "chunks", "fragments", "vertices", "fill_s", "filled"}
    assert timings["filled"] == want_count and timings["fill_s"] > 0
    # the filled store may be the caller's, and dust_global counts on it
    store = np.zeros(dataset.shape, dtype=dataset.dtype)
    got = post.skeletonize_chunked(dataset, CHUNK, fill_holes_global=True, filled_store=store, _fill=host_fill, dust_global=True, **kw)
    assert np.array_equal(store, want_volume) and np.array_equal(dataset, before)
    R.assert_same(got, post.skeletonize_chunked(want_volume, CHUNK, dust_global=True, **kw))
    # without the keyword the timings keep their eight keys
    timings = {}
    post.skeletonize_chunked(dataset, CHUNK, timings=timings, **kw)
    assert set(timings) == {"count_s", "chunks_s", "place_s", "fuse_s", "post_s", "chunks", "fragments", "vertices"}
