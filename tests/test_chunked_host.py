"""skeletonize_chunked without a GPU: plan.chunk_grid, post.place_fragment and post.route_targets on numbers, and the
whole driver run on the CPU oracle through its two private hooks, against the composition written out in tests/chunked_ref.py."""
import numpy as np
import pytest

import chunked_ref as R
from kimimaro_amd import post, skeletonize_chunked
from kimimaro_amd.plan import chunk_grid
from kimimaro_amd.skeleton import Skeleton


def host_postprocess(skeletons, dust_threshold, tick_threshold):
    return [post.postprocess(s, dust_threshold, tick_threshold) for s in skeletons]


def oracle_run(labels, **kwargs):
    from oracle import pipeline as P
    return P.skeletonize(labels, **kwargs)


def on_oracle(lab, chunk_shape, **kwargs):
    kw = dict(teasar_params=R.TP, anisotropy=R.AN, dust_threshold=R.CHUNK_DUST, post_dust_threshold=R.POST_DUST, tick_threshold=R.TICK)
    kw.update(kwargs)
    return skeletonize_chunked(lab, chunk_shape, _skeletonize=oracle_run, _postprocess=host_postprocess, **kw)


# -- chunk_grid ------------------------------------------------------------------------------------------------------------------
def axis(n, c):
    g = chunk_grid((n, 1, 1), (c, 1, 1))
    return [(int(a), int(b), int(d)) for a, b, d in zip(g.core_lo[:, 0], g.core_hi[:, 0], g.box_hi[:, 0])]


def test_grid_axis_rules():
    assert axis(96, 48) == [(0, 48, 49), (48, 96, 96)]                       # exact division
    assert axis(100, 48) == [(0, 48, 49), (48, 96, 97), (96, 100, 100)]      # a remainder
    assert axis(97, 48) == [(0, 48, 49), (48, 97, 97)]                       # the trailing overlap plane is no chunk
    assert axis(98, 48) == [(0, 48, 49), (48, 96, 97), (96, 98, 98)]
    assert axis(49, 48) == [(0, 49, 49)]
    assert axis(5, 48) == [(0, 5, 5)]                                        # c > n: one chunk, no overlap
    assert axis(1, 48) == [(0, 1, 1)] and axis(1, 1) == [(0, 1, 1)]
    assert axis(4, 1) == [(0, 1, 2), (1, 2, 3), (2, 4, 4)]
    for n in range(1, 40):
        for c in range(1, 12):
            assert axis(n, c) == R.axis_boxes(n, c), (n, c)


@pytest.mark.parametrize("shape,chunk_shape", [((96, 80, 48), (48, 40, 48)), ((100, 70, 40), (48, 48, 48)), ((97, 5, 1), (48, 2, 7)),
                                               ((7, 6, 5), (3, 2, 4)), ((9, 4), (4, 4)), ((9, 4), (4, 4, 3))])
def test_grid_order_partition_and_boxes(shape, chunk_shape):
    g = chunk_grid(shape, chunk_shape)
    shape3, chunk3 = (tuple(shape) + (1,))[:3], (tuple(chunk_shape) + (1,))[:3]
    want = R.boxes(shape3, chunk3)
    n = len(want)
    assert g.grid_index.shape == (n, 3) and int(np.prod(g.grid)) == n
    for name, col in (("core_lo", 0), ("core_hi", 1), ("box_lo", 2), ("box_hi", 3)):
        got = getattr(g, name)
        assert got.dtype == np.int64
        np.testing.assert_array_equal(got, np.array([w[col] for w in want]))
    # x fastest, then y, then z
    flat = g.grid_index[:, 0] + g.grid[0] * (g.grid_index[:, 1] + g.grid[1] * g.grid_index[:, 2])
    np.testing.assert_array_equal(flat, np.arange(n))
    # the cores are disjoint and sum to the dataset
    hits = np.zeros(shape3, dtype=np.int32)
    for lo, hi in zip(g.core_lo, g.core_hi):
        hits[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] += 1
    assert (hits == 1).all()
    # every box is its core plus one clamped plane on the high side
    np.testing.assert_array_equal(g.box_lo, g.core_lo)
    last = g.core_hi == np.array(shape3)
    np.testing.assert_array_equal(g.box_hi, np.where(last, g.core_hi, np.minimum(g.core_hi + 1, np.array(shape3))))


def test_grid_of_the_test_datasets():
    for shape, _, _, chunk_shape, chunks, _ in R.DATASETS:
        assert chunk_grid(shape, chunk_shape).box_lo.shape[0] == chunks


def test_grid_refusals():
    for shape, chunk_shape in (((96, 80, 48), (48, 0, 48)), ((96, 80, 48), (48, -1, 48)), ((96, 0, 48), (48, 40, 48)), ((96, 80, 48), (48, 40)),
                               ((96, 80), (48,)), ((96,), (48,)), ((4, 4, 4, 4), (2, 2, 2, 2)), ((96, 80, 48), (48, 40, 48, 1)),
                               ((96, 80, 48), (48.5, 40, 48))):
        with pytest.raises(ValueError):
            chunk_grid(shape, chunk_shape)


# -- place_fragment --------------------------------------------------------------------------------------------------------------
def test_placement_is_bit_exact_where_adding_in_physical_space_is_not():
    an = np.array([3.7, 3.7, 40.1], dtype=np.float32)
    rng = np.random.default_rng(3)
    differs = 0
    for off in (48, 96, 144, 1000):
        voxel = rng.integers(0, 49, size=(640, 3))
        low = np.array([off, 2 * off, off + 1])
        skel = Skeleton(voxel.astype(np.float32) * an, np.stack([np.arange(639), np.arange(1, 640)], axis=1),
                        rng.uniform(1, 9, 640).astype(np.float32), segid=5, space="physical")
        before = skel.clone()
        got = post.place_fragment(skel, low, an, label=77)
        want = (voxel + low).astype(np.float32) * an
        assert want.dtype == np.float32 and got.vertices.dtype == np.float32
        np.testing.assert_array_equal(got.vertices.view(np.uint32), want.view(np.uint32))
        np.testing.assert_array_equal(got.edges, skel.edges)
        np.testing.assert_array_equal(got.radii, skel.radii)
        assert got.id == 77 and got.space == "physical" and post.place_fragment(skel, low, an).id == 5
        assert skel == before                                                   # the input is not modified
        differs += int(np.count_nonzero(skel.vertices + low.astype(np.float32) * an != want))
    assert differs > 1000            # the form one would write by hand does miss


def test_placement_refuses_vertices_off_the_lattice():
    an = np.array([3.7, 3.7, 40.1], dtype=np.float32)
    v = np.array([[1, 2, 3], [4, 5, 6]], dtype=np.float32) * an
    ok = Skeleton(v, [[0, 1]], [1, 1], space="physical")
    post.place_fragment(ok, (48, 0, 0), an)
    for bad in (np.nextafter(v[1, 2], np.float32(np.inf)), v[1, 2] + np.float32(20.0)):
        w = v.copy()
        w[1, 2] = bad
        with pytest.raises(ValueError):
            post.place_fragment(Skeleton(w, [[0, 1]], [1, 1], space="physical"), (48, 0, 0), an)
    assert post.place_fragment(Skeleton(), (48, 0, 0), an).empty()


# -- route_targets ---------------------------------------------------------------------------------------------------------------
def test_targets_reach_every_box_that_holds_them():
    shape, chunk_shape = (96, 80, 48), (48, 40, 48)
    g = chunk_grid(shape, chunk_shape)
    pts = [(10, 10, 10), (48, 10, 10), (47, 39, 0), (48, 40, 47), (95, 79, 47), np.array([49, 41, 5])]
    got = post.route_targets(pts, g, shape)
    assert got == [[(10, 10, 10), (48, 10, 10), (47, 39, 0), (48, 40, 47)],           # x = 48 and y = 40 are overlap planes
                   [(0, 10, 10), (0, 40, 47)],
                   [(48, 0, 47)],
                   [(0, 0, 47), (47, 39, 47), (1, 1, 5)]]
    assert post.route_targets([], g, shape) == [[], [], [], []]
    assert post.route_targets([(4, 3), (5, 0)], chunk_grid((9, 4), (4, 4)), (9, 4)) == [[(4, 3, 0)], [(0, 3, 0), (1, 0, 0)]]
    for bad in ((96, 0, 0), (0, -1, 0), (0, 0, 48)):
        with pytest.raises(IndexError, match=str(bad[0])):
            post.route_targets([(1, 1, 1), bad], g, shape)
    with pytest.raises(IndexError, match="96"):
        skeletonize_chunked(np.zeros(shape, np.uint8), chunk_shape, extra_targets_after=[(96, 0, 0)], _skeletonize=oracle_run,
                            _postprocess=host_postprocess)


# -- the whole driver on the oracle ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def oracle_fragments():
    return [R.fragments(R.dataset(k), R.DATASETS[k][3], oracle_run) for k in range(len(R.DATASETS))]


@pytest.mark.parametrize("k", range(len(R.DATASETS)))
def test_driver_on_the_oracle_equals_the_composition(k, oracle_fragments):
    lab, chunk_shape, spanning = R.dataset(k), R.DATASETS[k][3], R.DATASETS[k][5]
    timings = {}
    got = on_oracle(lab, chunk_shape, timings=timings)
    frags = oracle_fragments[k]
    want = R.compose(frags, post.postprocess)
    R.assert_same(got, want)
    several = [label for label, f in frags.items() if len(f) > 1]
    assert len(several) >= spanning
    for label in several:
        assert label in got and len(got[label].components()) == 1, label       # the pieces of a label come out as ONE skeleton
    for skel in got.values():
        for comp in skel.components():
            assert comp.edges.shape[0] == comp.vertices.shape[0] - 1 and post.find_cycle(comp.edges) == []
    assert timings["chunks"] == R.DATASETS[k][4] and timings["fragments"] == sum(len(f) for f in frags.values())
    assert timings["vertices"] == sum(s.vertices.shape[0] for f in frags.values() for s in f)
    assert set(timings) == {"count_s", "chunks_s", "place_s", "fuse_s", "post_s", "chunks", "fragments", "vertices"}

    raw = on_oracle(lab, chunk_shape, merge=False)
    assert list(raw) == list(frags)
    seam = 0
    for label in frags:
        assert len(raw[label]) == len(frags[label])
        for a, b in zip(raw[label], frags[label]):
            assert a == b and a.id == label and a.space == "physical"
            np.testing.assert_array_equal(a.transform, b.transform)
        seam += sum(s.vertices.shape[0] for s in raw[label]) - Skeleton.simple_merge(raw[label]).consolidate().vertices.shape[0]
    assert seam >= 20                 # fused seam vertices (69 and 27 when this was written)


def test_dust_global_keeps_the_labels_the_cut_makes_small():
    lab, chunk_shape = R.dataset(0), R.DATASETS[0][3]
    per_chunk = on_oracle(lab, chunk_shape, dust_threshold=R.GLOBAL_DUST, merge=False)
    whole = on_oracle(lab, chunk_shape, dust_threshold=R.GLOBAL_DUST, dust_global=True, merge=False)
    assert len(per_chunk) == 8 and len(whole) == 12 and set(per_chunk) < set(whole)
    for label in (1003, 1012):
        assert label in np.unique(lab) and label not in per_chunk and label not in whole
    want = R.fragments(lab, chunk_shape, oracle_run, dust_threshold=R.GLOBAL_DUST, dust_global=True)
    assert list(whole) == list(want)
    for label in want:
        assert len(whole[label]) == len(want[label]) and all(a == b for a, b in zip(whole[label], want[label]))
    # a given object_ids is intersected with the kept labels
    some = on_oracle(lab, chunk_shape, dust_threshold=R.GLOBAL_DUST, dust_global=True, merge=False, object_ids=[1003, sorted(whole)[0]])
    assert list(some) == sorted(whole)[:1]
    assert post.count_labels(lab, chunk_grid(lab.shape, chunk_shape)) == dict(zip(*(a.tolist() for a in np.unique(lab, return_counts=True))))


def test_dataset_forms_give_equal_results(tmp_path, oracle_fragments):
    lab, chunk_shape = R.dataset(1), R.DATASETS[1][3]
    want = R.compose(oracle_fragments[1], post.postprocess)
    mm = np.memmap(str(tmp_path / "labels.bin"), dtype=lab.dtype, mode="w+", shape=lab.shape, order="F")
    mm[...] = lab
    mm.flush()

    class Sliced:
        """the h5py / zarr form: a shape and __getitem__ over a tuple of slices, nothing else"""
        shape = lab.shape

        def __getitem__(self, key):
            assert isinstance(key, tuple) and len(key) == 3 and all(isinstance(s, slice) for s in key)
            return lab[key].copy()

    for form in (np.asfortranarray(lab), np.ascontiguousarray(lab), np.memmap(str(tmp_path / "labels.bin"), dtype=lab.dtype, mode="r",
                                                                                shape=lab.shape, order="F"), Sliced()):
        R.assert_same(on_oracle(form, chunk_shape), want)


def test_no_voxel_graph_parameter_and_empty_datasets():
    with pytest.raises(TypeError):
        skeletonize_chunked(np.zeros((4, 4, 4), np.uint8), voxel_graph=np.zeros((4, 4, 4), np.uint32))
    assert on_oracle(np.zeros((60, 50, 8), np.uint8), (48, 48, 48)) == {}
    assert on_oracle(np.zeros((60, 50, 8), np.uint8), (48, 48, 48), dust_global=True, merge=False) == {}
    with pytest.raises(ValueError):
        on_oracle(np.zeros((60, 50, 8), np.uint8), (48, 0, 48))


def test_no_cpu_fallback_without_the_hooks():
    import torch
    import kimimaro_amd
    assert kimimaro_amd.skeletonize_chunked is post.skeletonize_chunked
    if torch.cuda.is_available():
        return
    lab = np.ones((8, 8, 8), np.uint8)
    with pytest.raises(kimimaro_amd.HipUnavailableError):
        skeletonize_chunked(lab, (4, 4, 4))
    with pytest.raises(kimimaro_amd.HipUnavailableError):
        skeletonize_chunked(lab, (4, 4, 4), _skeletonize=oracle_run)            # the merge still needs postprocess_many
    with pytest.raises(kimimaro_amd.HipUnavailableError):
        skeletonize_chunked(lab, (4, 4, 4), _postprocess=host_postprocess)
    assert skeletonize_chunked(lab, (4, 4, 4), dust_threshold=0, merge=False, _skeletonize=oracle_run) is not None
