"""synapses_to_targets_chunked without a GPU: the whole driver on the numpy statement of one visit
(tests/synapses_chunked_ref.py) against tests/points_ref.py::synapses_to_targets of the whole dataset, item for item in insertion
order; the bound that decides which cores are visited; the forms of a dataset, the refusals and the signatures."""
import inspect

import numpy as np
import pytest

import chunked_ref
import points_ref
import synapses_chunked_ref as S

KINDS = ("scattered", "clustered", "cut_ties")


def synapses_of(kind, chunk_shape):
    lab = S.dataset()
    return {"scattered": S.scattered, "clustered": S.clustered}[kind](lab) if kind != "cut_ties" else S.cut_ties(lab, chunk_shape)


@pytest.mark.parametrize("chunk_shape", S.CHUNKS)
@pytest.mark.parametrize("kind", KINDS)
def test_driver_equals_the_whole_dataset(kind, chunk_shape):
    lab = S.dataset()
    if kind == "cut_ties" and not S.cut_planes(lab.shape, chunk_shape):
        synapses = S.cut_ties(lab, S.CHUNKS[0])           # one chunk has no cut: the ties of another grid, all in its one core
    else:
        synapses = synapses_of(kind, chunk_shape)
    want = list(points_ref.synapses_to_targets(lab, synapses).items())
    assert want
    seen = {}
    for name, order in S.ORDERS.items():
        stats = {}
        got = S.host_driver(lab, synapses, chunk_shape, stats=stats, _order=order)
        assert list(got.items()) == want, name
        assert all(type(v) is int for key in got for v in key)
        assert set(stats) == {"cores", "cores_visited", "cores_skipped", "pairs", "load_s", "visit_s"}
        assert stats["cores_visited"] + stats["cores_skipped"] == stats["cores"] and stats["pairs"] >= stats["cores_visited"]
        seen[name] = stats
    if kind == "scattered":                                # the absent label keeps every core in play, whatever the order
        assert all(s["cores_visited"] == s["cores"] for s in seen.values())
    print(kind, chunk_shape, {k: (s["cores_visited"], s["cores"], s["pairs"]) for k, s in seen.items()})


@pytest.mark.parametrize("chunk_shape", S.CHUNKS[:2])
def test_every_cut_tie_spans_two_cores(chunk_shape):
    from kimimaro_amd import plan
    lab = S.dataset()
    synapses = S.cut_ties(lab, chunk_shape)
    sets = S.nearest_sets(lab, synapses)
    assert len(sets) == 3 * len(S.cut_planes(lab.shape, chunk_shape)) == {S.CHUNKS[0]: 18, S.CHUNKS[1]: 27}[chunk_shape]
    for voxels in sets:
        assert len(set(plan.core_of(voxels, lab.shape, chunk_shape).tolist())) > 1


@pytest.mark.parametrize("chunk_shape", S.CHUNKS[:2])
def test_the_culling_bites(chunk_shape):
    lab = S.dataset()
    label = int(np.unique(lab)[2])
    stats = {}
    one = S.clustered(lab, labels={label})
    assert list(S.host_driver(lab, one, chunk_shape, stats=stats).items()) == list(points_ref.synapses_to_targets(lab, one).items())
    print("one label:", stats["cores_visited"], "of", stats["cores"])
    assert 0 < 2 * stats["cores_visited"] < stats["cores"]
    every = S.clustered(lab)
    S.host_driver(lab, every, chunk_shape, stats=stats)
    print("all labels:", stats["cores_visited"], "of", stats["cores"], "pairs", stats["pairs"])
    assert stats["cores_visited"] < stats["cores"]
    assert stats["pairs"] < stats["cores"] * sum(len(p) for p in every.values())
    every[S.ABSENT] = [((1.0, 2.0, 3.0), 0)]
    S.host_driver(lab, every, chunk_shape, stats=stats)
    assert stats["cores_visited"] == stats["cores"]


@pytest.mark.parametrize("scale", (1.0, 1.0 / 3.0, 1e-3, 1e3))
def test_the_bound_never_exceeds_a_computed_distance(scale):
    from kimimaro_amd import plan
    rng = np.random.default_rng(int(scale * 3000) + 1)
    for _ in range(750):
        lo = rng.integers(0, 40, size=3)
        hi = lo + rng.integers(1, 6, size=3)
        centroids = rng.integers(-200, 600, size=(4, 3)).astype(np.float64) * (scale / 10.0)
        voxels = np.stack(np.meshgrid(*[np.arange(a, b) for a, b in zip(lo, hi)], indexing="ij"), axis=-1).reshape(-1, 3)
        bounds = plan.box_distance_bounds(lo[None], hi[None], centroids)
        assert bounds.shape == (1, 4) and bounds.dtype == np.float64
        for q in range(4):
            assert bounds[0, q] <= S.distance_bits(voxels, centroids[q]).view(np.float64).min()


def test_the_bound_of_a_centroid_inside_the_box_is_zero():
    from kimimaro_amd import plan
    lo, hi = np.array([[0, 0, 0], [4, 5, 6]]), np.array([[4, 5, 6], [9, 9, 9]])
    bounds = plan.box_distance_bounds(lo, hi, [(1.3, 4.0, 0.1), (4.0, 5.5, 8.0), (3.5, 2.0, 2.0)])
    np.testing.assert_array_equal(bounds == 0, [[True, False, False], [False, True, False]])
    assert bounds[0, 2] == 0.5 and bounds[1, 2] == np.sqrt((0.5 * 0.5 + 3.0 * 3.0) + 4.0 * 4.0)
    np.testing.assert_array_equal(plan.nearest_first(bounds), [0, 1])
    np.testing.assert_array_equal(plan.nearest_first(np.array([[2.0, 1.0], [0.5, 3.0], [4.0, 0.5]])), [1, 2, 0])      # stable


class SlicingOnly:
    """what h5py and zarr offer: a shape and cuts over a tuple of slices"""

    def __init__(self, array):
        self._array, self.shape = array, array.shape

    def __getitem__(self, key):
        assert isinstance(key, tuple) and all(isinstance(s, slice) for s in key)
        return self._array[key]


def test_dataset_forms():
    lab = S.dataset()
    synapses = S.clustered(lab)
    want = list(points_ref.synapses_to_targets(lab, synapses).items())
    for form in (np.ascontiguousarray(lab), np.asfortranarray(lab), SlicingOnly(lab), lab.astype(np.int64), lab.astype(np.uint16)):
        assert list(S.host_driver(form, synapses, S.CHUNKS[0]).items()) == want
    small = (lab % 251).astype(np.int8)                        # signed labels, negative ones among them
    assert small.min() < 0
    synapses = S.clustered(small)
    assert list(S.host_driver(small, synapses, S.CHUNKS[0]).items()) == list(points_ref.synapses_to_targets(small, synapses).items())


def test_labels_the_dtype_cannot_hold_and_repeated_words():
    lab = S.dataset().astype(np.uint16)
    label = int(lab[20, 10, 10])
    synapses = {70000: [((1.0, 1.0, 1.0), 1)], -1: [((2.0, 2.0, 2.0), 2)], label: [((5.0, 5.0, 5.0), 0)],
                label + 0.5: [((3.0, 3.0, 3.0), 1)], "x": [((3.0, 3.0, 3.0), 1)], 7: []}
    got = S.host_driver(lab, synapses, S.CHUNKS[0])
    assert list(got.items()) == list(points_ref.synapses_to_targets(lab, {label: synapses[label]}).items()) and len(got) == 1
    assert S.host_driver(lab, {70000: [((1.0, 1.0, 1.0), 1)]}, S.CHUNKS[0]) == {}


def test_refusals_and_early_exits(monkeypatch):
    import kimimaro_amd
    from kimimaro_amd import ops

    def no_engine():
        raise AssertionError("the GPU was asked for")
    monkeypatch.setattr(ops, "engine", no_engine)
    lab = S.dataset()
    one = {int(lab[5, 5, 5]): [((1.0, 2.0, 3.0), 0)]}
    for wrong in (lab[:, :, 0], lab[..., None]):
        with pytest.raises(kimimaro_amd.DimensionError):
            S.host_driver(wrong, one, S.CHUNKS[0])
        with pytest.raises(kimimaro_amd.DimensionError):
            kimimaro_amd.synapses_to_targets_chunked(wrong, {})
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError, match="finite"):
            S.host_driver(lab, {int(lab[5, 5, 5]): [((1.0, bad, 3.0), 0)]}, S.CHUNKS[0])

    class Huge:
        shape = (2 ** 21, 2 ** 21, 2 ** 21)
    with pytest.raises(ValueError, match="2\\^63"):
        kimimaro_amd.synapses_to_targets_chunked(Huge(), {})
    assert kimimaro_amd.synapses_to_targets_chunked(lab, {}) == {}
    assert kimimaro_amd.synapses_to_targets_chunked(lab, {}, chunk_shape=(8, 8, 8), progress=True, stats={}) == {}
    with pytest.raises(AssertionError, match="the GPU was asked for"):          # no CPU fallback: the engine is the first thing asked for
        kimimaro_amd.synapses_to_targets_chunked(lab, one)


def test_public_signatures():
    import kimimaro_amd
    from kimimaro_amd import plan, points, post
    assert kimimaro_amd.synapses_to_targets_chunked is post.synapses_to_targets_chunked
    empty = inspect.Parameter.empty
    params = inspect.signature(kimimaro_amd.synapses_to_targets_chunked).parameters.values()
    assert [(p.name, p.default) for p in params] == [("dataset", empty), ("synapses", empty), ("chunk_shape", (512, 512, 512)),
                                                     ("progress", False), ("stats", None), ("_visit", None), ("_order", None)]
    assert list(inspect.signature(points.nearest_label_voxels_box).parameters) == [
        "eng", "d_lab", "label_bytes", "extent", "lo", "dataset_shape", "words", "query_start", "centroids", "query_index", "d_best",
        "d_vox"]
    assert list(inspect.signature(plan.box_distance_bounds).parameters) == ["core_lo", "core_hi", "centroids"]
    chunked = inspect.signature(post.skeletonize_chunked).parameters
    assert list(chunked)[-3:] == ["_fill", "synapses", "_synapse_targets"]
    assert chunked["synapses"].default is None and chunked["_synapse_targets"].default is None


def oracle_run(labels, **kwargs):
    from oracle import pipeline as P
    return P.skeletonize(labels, **kwargs)


def host_postprocess(skeletons, dust_threshold, tick_threshold):
    from kimimaro_amd import post
    return [post.postprocess(s, dust_threshold, tick_threshold) for s in skeletons]


def test_skeletonize_chunked_takes_synapses():
    from kimimaro_amd import post
    lab = S.dataset()
    chunk_shape = (20, 29, 23)                              # two boxes
    synapses = S.clustered(lab, per_label=2)
    asked = []

    def targets(dataset, syn, chunk):
        asked.append((dataset, syn, chunk))
        return S.host_driver(dataset, syn, chunk)

    kw = dict(teasar_params=chunked_ref.TP, anisotropy=chunked_ref.AN, dust_threshold=50, post_dust_threshold=0, tick_threshold=0,
              _skeletonize=oracle_run, _postprocess=host_postprocess)
    want_targets = list(points_ref.synapses_to_targets(lab, synapses))
    assert len(want_targets) >= 8
    want = post.skeletonize_chunked(lab, chunk_shape, extra_targets_after=want_targets, **kw)
    got = post.skeletonize_chunked(lab, chunk_shape, synapses=synapses, _synapse_targets=targets, **kw)
    assert len(asked) == 1 and asked[0][0] is lab and asked[0][1] is synapses and asked[0][2] == chunk_shape
    chunked_ref.assert_same(got, want)
    # the targets add to the caller's own, and they matter: some become vertices that the plain call does not have
    plain = post.skeletonize_chunked(lab, chunk_shape, **kw)
    an = np.array(chunked_ref.AN, dtype=np.float32)
    rows = lambda skels: {tuple(v) for s in skels.values() for v in s.vertices.tolist()}
    at = {tuple((np.array(t, dtype=np.float32) * an).tolist()) for t in want_targets}
    assert at & rows(got) and (at & rows(got)) - rows(plain)
    both = post.skeletonize_chunked(lab, chunk_shape, extra_targets_after=want_targets[:1], synapses=synapses, _synapse_targets=targets, **kw)
    chunked_ref.assert_same(both, want)
