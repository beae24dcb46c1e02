"""oversegment_chunked without a GPU: the whole driver -- boxes, seeds, rounds, dirty marks, stores, single-voxel
labels, numbering, segments -- runs through its `_box` seam on numpy Jacobi sweeps (tests/oversegment_chunked_ref.py) and has to
equal tests/feature_ref.oversegment of the WHOLE dataset: features, dtype, segments and the distance store, exactly."""
import inspect

import numpy as np
import pytest

import feature_ref as R
import oversegment_chunked_ref as H
from kimimaro_amd import post


def run(dataset, skels, an, chunk, **kw):
    timings = {}
    got_f, got_s = post.oversegment_chunked(dataset, skels, chunk_shape=chunk, anisotropy=an, timings=timings, _box=H.relax_box, **kw)
    return got_f, got_s, timings


def assert_same(dataset, skels, an, chunk, whole=None, **kw):
    """the chunked call on `dataset` == the reference on `whole` (default: the dataset itself, a numpy array)"""
    whole = dataset if whole is None else whole
    shape = (tuple(whole.shape) + (1,))[:3]
    store = np.full(shape, -1.0, dtype=np.float32, order="F")
    got_f, got_s, timings = run(dataset, skels, an, chunk, distance_store=store, **kw)
    want_f, want_s, (want_d, _, _) = R.oversegment(whole, skels, an)
    if "feature_store" not in kw:
        assert got_f.dtype == want_f.dtype and got_f.shape == want_f.shape
        np.testing.assert_array_equal(got_f, want_f)
    H.assert_skeletons(got_s, want_s, skels)
    np.testing.assert_array_equal(store.view(np.uint32), want_d.view(np.uint32))
    assert timings["segments"] == int(want_f.max())
    return got_f, got_s, timings


RANDOM = [((21, 9, 6), (8, 4, 3)), ((6, 21, 7), (3, 8, 5)), ((13, 11, 10), (5, 5, 5)), ((17, 8, 9), (6, 3, 4)),
          ((9, 9, 21), (4, 7, 8)), ((20, 6, 6), (7, 6, 3)), ((11, 14, 8), (8, 8, 8)), ((15, 15, 6), (3, 4, 5)),
          ((7, 6, 19), (6, 5, 7)), ((12, 10, 11), (5, 3, 6)), ((21, 21, 6), (8, 8, 4)), ((10, 13, 12), (4, 6, 5))]


@pytest.mark.parametrize("case", range(len(RANDOM)))
def test_random_volumes(case):
    """random blobs with holes, 9 seeds on 4 labels, chunk entries 3..8, the four anisotropies in turn"""
    shape, chunk = RANDOM[case]
    an = H.ANISOTROPIES[case % 4]
    lab, skels = H.random_blobs(np.random.default_rng(1000 + case), shape, an=an)
    _, _, timings = assert_same(lab, skels, an, chunk)
    assert timings["distance_visits"] >= timings["cores"] and timings["feature_visits"] >= timings["cores"]
    assert timings["boxes_loaded"] == timings["distance_visits"] + timings["feature_visits"]


@pytest.mark.parametrize("name,build", H.CASES, ids=[c[0] for c in H.CASES])
def test_shared_cases(name, build):
    lab, skels, an, chunk = build()
    assert_same(lab, skels, an, chunk)


def test_serpentine_needs_a_visit_per_crossing():
    """six rows that cross the cut x = 8 once each, seeded at one end: any box-by-box scheme needs a visit per crossing, and the
    call ends (by "no core is dirty", not by a count)"""
    lab = H.serpentine(6, 16)
    got_f, _, timings = assert_same(lab, H.skel(7, [[0, 0, 0]]), (1, 1, 1), (8, 64, 1))
    assert timings["cores"] == 2 and timings["distance_visits"] >= 6 and timings["feature_visits"] >= 6
    assert timings["distance_rounds"] >= 3 and np.all(got_f[lab != 0] == 1)


def test_u_turn_revisits_the_seed_core():
    """the shortest path from the seed in core A to the other arm, also in core A, runs through core B: A is visited again"""
    lab, s = H.u_turn()
    got_f, _, timings = assert_same(lab, s, (1, 1, 1), (6, 9, 3))
    assert timings["cores"] == 2 and timings["distance_visits"] >= 3
    assert got_f[1, 5, 1] == 1


def test_ties_across_cuts_go_to_the_smaller_number():
    lab, skels = H.tie_volume()
    got_f, got_s, _ = assert_same(lab, skels, (1, 1, 1), (8, 8, 8))
    for s, tie in zip(got_s, [(8, 1, 1), (8, 8, 3), (8, 8, 8)]):
        assert got_f[tie] == s.segments[0] != s.segments[1]              # vertex 0 has the smaller provisional number


def test_numbering_follows_the_dataset_raster_not_the_visiting_order():
    lab, skels = H.numbering_volume()
    got_f, got_s, _ = assert_same(lab, skels, (1, 1, 1), (4, 8, 1))
    assert got_f[5, 0, 0] == 1 and got_f[0, 1, 0] == 2                   # core 1 holds segment 1, core 0 segment 2
    assert got_s[0].segments.tolist() == [2] and got_s[1].segments.tolist() == [1]


def test_uint16_result():
    lab, s = H.long_line()
    got_f, got_s, timings = assert_same(lab, s, (1, 1, 1), (64, 2, 2))
    assert timings["cores"] == 5 and got_f.dtype == np.uint16 and got_f.max() == 300
    assert got_s.segments.tolist() == list(range(1, 301))


def test_skip_rules_next_to_a_cut():
    lab, skels = H.skip_volume()
    got_f, got_s, _ = assert_same(lab, skels, (1, 1, 1), (6, 5, 4))
    assert got_f[5, 3, 1] == 0 and got_s[5].segments.tolist() == [0]     # one voxel in the dataset: skipped
    assert got_f[5, 3, 3] != 0 and got_f[5, 3, 3] == got_f[6, 3, 3]      # one voxel in each of two cores: not skipped
    # (segments is the feature AT the vertex's voxel, whoever seeded it: skeleton 11 seeds nothing but sits on label 7)
    assert np.all(got_f[lab == 3] == 0) and got_s[11].segments.tolist() == [got_f[5, 1, 1]] and got_s[0].segments.tolist() == [0]
    seg = got_s[7].segments
    assert seg[0] == seg[2] != 0 and seg[3] == got_f[6, 3, 3] and seg[4] == 0
    assert len(set(seg[[0, 1, 5]].tolist())) == 3


def test_dataset_forms(tmp_path):
    lab, skels = H.random_blobs(np.random.default_rng(7), (14, 9, 8))

    class Sliced:
        """the h5py / zarr form: a shape and __getitem__ over a tuple of slices, nothing else"""
        shape = lab.shape

        def __getitem__(self, key):
            assert isinstance(key, tuple) and len(key) == 3 and all(isinstance(s, slice) for s in key)
            return lab[key].copy()

    path = str(tmp_path / "labels.bin")
    np.memmap(path, dtype=lab.dtype, mode="w+", shape=lab.shape, order="F")[:] = lab
    for form in (np.asfortranarray(lab), np.ascontiguousarray(lab), np.memmap(path, dtype=lab.dtype, mode="r", shape=lab.shape, order="F"),
                 Sliced()):
        assert_same(form, skels, (4, 4, 40), (5, 4, 3), whole=lab)


def test_stores_as_memmaps_and_by_slices_only(tmp_path):
    lab, skels = H.random_blobs(np.random.default_rng(8), (12, 10, 7))
    an, chunk = (16, 16, 40), (5, 4, 3)
    want_f, _, (want_d, _, _) = R.oversegment(lab, skels, an)
    d_map = np.memmap(str(tmp_path / "d.bin"), dtype=np.float32, mode="w+", shape=lab.shape, order="F")
    f_map = np.memmap(str(tmp_path / "f.bin"), dtype=np.uint32, mode="w+", shape=lab.shape, order="F")
    got_f, _, _ = run(lab, skels, an, chunk, distance_store=d_map, feature_store=f_map)
    assert got_f is f_map and got_f.dtype == np.uint32                   # a store that was passed comes back, as u32
    np.testing.assert_array_equal(np.asarray(f_map), want_f)
    np.testing.assert_array_equal(np.asarray(d_map).view(np.uint32), want_d.view(np.uint32))

    class Store:
        """read and written by a tuple of three slices, nothing else"""

        def __init__(self, dtype):
            self.a = np.zeros(lab.shape, dtype=dtype)
            self.shape, self.dtype = self.a.shape, self.a.dtype

        def __getitem__(self, key):
            assert isinstance(key, tuple) and len(key) == 3 and all(isinstance(s, slice) for s in key)
            return self.a[key].copy()

        def __setitem__(self, key, value):
            assert isinstance(key, tuple) and len(key) == 3 and all(isinstance(s, slice) for s in key)
            self.a[key] = value

    d_own, f_own = Store(np.float32), Store(np.uint32)
    got_f, _, _ = run(lab, skels, an, chunk, distance_store=d_own, feature_store=f_own)
    assert got_f is f_own
    np.testing.assert_array_equal(f_own.a, want_f)
    np.testing.assert_array_equal(d_own.a.view(np.uint32), want_d.view(np.uint32))


def test_argument_errors():
    lab, skels = H.skip_volume()
    with pytest.raises(NotImplementedError, match="fill_holes"):
        post.oversegment_chunked(lab, skels, fill_holes=True)
    with pytest.raises(NotImplementedError, match="downsample"):
        post.oversegment_chunked(lab, skels, downsample=1)
    for kw in (dict(distance_store=np.zeros((12, 5, 3), dtype=np.float32)), dict(distance_store=np.zeros(lab.shape, dtype=np.float64)),
               dict(feature_store=np.zeros((12, 5), dtype=np.uint32)), dict(feature_store=np.zeros(lab.shape, dtype=np.int32)),
               dict(chunk_shape=(6, 0, 4))):
        with pytest.raises(ValueError):
            post.oversegment_chunked(lab, skels, _box=H.relax_box, **kw)


def test_fails_loudly_without_gpu():
    import torch
    import kimimaro_amd
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")

    class Untouched:
        shape = (4, 4, 4)

        def __getitem__(self, key):
            raise AssertionError("nothing is loaded before the device is known to be there")

    with pytest.raises(kimimaro_amd.HipUnavailableError):
        kimimaro_amd.oversegment_chunked(Untouched(), H.skel(1, [[1, 1, 1]]))


def test_interface():
    import kimimaro_amd
    assert kimimaro_amd.oversegment_chunked is post.oversegment_chunked
    sig = inspect.signature(post.oversegment_chunked)
    assert list(sig.parameters) == ["dataset", "skeletons", "chunk_shape", "anisotropy", "progress", "fill_holes", "in_place", "downsample",
                                    "distance_store", "feature_store", "timings", "_box"]
    defaults = [p.default for p in sig.parameters.values()][2:]
    assert defaults == [(512, 512, 512), (1, 1, 1), False, False, False, 0, None, None, None, None]
    lab, skels = H.skip_volume()
    as_list = list(skels.values())
    one = skels[7]
    for container in (skels, as_list, one):
        got_f, got_s, timings = assert_same(lab, container, (1, 1, 1), (6, 5, 4), progress=True, in_place=True)
        assert type(got_s) is type(container)
    assert hasattr(got_s, "vertices") and set(np.unique(got_f[lab != 7])) == {0}
    assert set(timings) >= {"cores", "distance_rounds", "distance_visits", "feature_rounds", "feature_visits", "boxes_loaded",
                            "voxels_loaded", "load_s", "relax_ms", "number_s", "segments"}
