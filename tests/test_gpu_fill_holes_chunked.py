"""fill_all_holes_chunked on the MI355X: kh_region_apply_box against numpy, its guard against ids outside the
core's range, its argument checks; the driver against intake.fill_all_holes of the whole dataset and against fill_ref.static; and
skeletonize_chunked(fill_holes_global=True) against the composition of tests/chunked_ref.py on the filled dataset.  Every comparison
is exact."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chunked_ref as R  # noqa: E402
import fill_chunked_ref as F  # noqa: E402
import fill_ref  # noqa: E402
import join_ref as J  # noqa: E402
import section_filled_chunked_ref as H  # noqa: E402

pytestmark = pytest.mark.gpu

NREG, PAD = 37, 16


@pytest.fixture(scope="module")
def eng():
    from kimimaro_amd import ops
    return ops.engine()


# ---- kh_region_apply_box ------------------------------------------------------------------------------------------------------------

def apply_call(eng, region, base, nregions, owner, labels):
    """one call of kh_region_apply_box on copies -> (the labels afterwards, state u64 [2]); state starts as garbage: the entry sets it"""
    from kimimaro_amd import _abi
    t = eng.torch
    d_region = t.from_numpy(region.view(np.int32)).to(eng.device)
    d_owner = t.from_numpy(owner.view(np.int64)).to(eng.device)
    d_lab = eng.to_device(labels)
    d_state = t.full((2,), 99, dtype=t.int64, device=eng.device)
    _abi.check(eng.lib.kh_region_apply_box(eng.ptr(d_region), int(base), int(nregions), eng.ptr(d_owner), eng.ptr(d_lab),
                                           labels.dtype.itemsize, region.size, eng.ptr(d_state), eng.stream()))
    return d_lab.cpu().numpy().view(labels.dtype), d_state.cpu().numpy().view(np.uint64)


def owners(rng, dtype, nregions, extra=0):
    """u64 [nregions + 1 + extra]: about half of the regions have an owner, a value the dtype holds; entry 0 is 0"""
    top = int(np.iinfo(dtype).max)
    own = rng.integers(1, min(top, 2 ** 62), size=nregions + 1 + extra, dtype=np.uint64)
    own[rng.random(own.size) < 0.5] = 0
    own[0] = 0
    if dtype == np.uint64:
        own[1], own[2] = 2 ** 63 + 11, 2 ** 64 - 1                        # owners with the top bit set
    return own


def painted_by_numpy(region, base, nregions, owner, labels):
    r = (region.astype(np.int64) - int(base)) % 2 ** 32                   # u32 arithmetic
    known = (r >= 1) & (r <= nregions)
    own = np.where(known, owner[np.where(known, r, 0)], 0).astype(np.uint64)
    out = labels.copy()
    out[own != 0] = own[own != 0].astype(labels.dtype)
    return out, int(np.count_nonzero(own)), int(np.count_nonzero(~known))


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.uint32, np.uint64])
@pytest.mark.parametrize("nvox", [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4099, 524_288, 524_289, 2 * 524_288 + 77])
def test_apply_box_against_numpy(eng, nvox, dtype):
    rng = np.random.default_rng(nvox)
    for base in (0, 1, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1 - NREG):
        region = (rng.integers(1, NREG + 1, size=nvox) + base).astype(np.uint32)
        if nvox >= 64:
            region[5], region[-1] = base + 1, base + NREG               # both ends of the range
        labels = rng.integers(0, 200, size=nvox).astype(dtype)
        owner = owners(rng, dtype, NREG)
        want, n_painted, n_outside = painted_by_numpy(region, base, NREG, owner, labels)
        got, state = apply_call(eng, region, base, NREG, owner, labels)
        assert n_outside == 0 and np.array_equal(got, want), base
        assert state.tolist() == [n_painted, 0] and (n_painted > 0 or nvox < 63)
        got, state = apply_call(eng, region, base, NREG, np.zeros(NREG + 1, dtype=np.uint64), labels)
        assert np.array_equal(got, labels) and state.tolist() == [0, 0]   # nobody owns anything: nothing is written


def test_apply_box_paints_owners_above_2_63(eng):
    rng = np.random.default_rng(7)
    region = rng.integers(1, 4, size=300).astype(np.uint32)
    labels = np.zeros(300, dtype=np.uint64)
    owner = np.array([0, 2 ** 63 + 11, 2 ** 64 - 1, 0], dtype=np.uint64)
    got, state = apply_call(eng, region, 0, 3, owner, labels)
    assert np.array_equal(got, owner[region]) and state[0] == np.count_nonzero(region != 3) and got.max() == 2 ** 64 - 1


@pytest.mark.parametrize("dtype", [np.uint8, np.uint64])
@pytest.mark.parametrize("base", [0, 1, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1 - NREG - PAD])
def test_apply_box_leaves_ids_outside_the_range_alone(eng, base, dtype, nvox=2000):
    """The owner buffer is longer than the table and holds non-zero sentinels in entry 0 and behind entry NREG; the ids outside the
    range are `base` itself and base + NREG + 1 .. base + NREG + PAD.  Without the guard such a voxel would be painted with a
    sentinel read inside the allocation; no id below `base` is used."""
    rng = np.random.default_rng(3)
    owner = owners(rng, dtype, NREG, extra=PAD)
    owner[0] = 0x55
    owner[NREG + 1:] = 0x66
    region = (rng.integers(1, NREG + 1, size=nvox) + base).astype(np.uint32)
    stray = rng.random(nvox) < 0.3
    region[stray] = (base + np.where(rng.random(nvox) < 0.4, 0, rng.integers(NREG + 1, NREG + PAD + 1, size=nvox)))[stray].astype(np.uint32)
    region[0], region[1], region[2] = base, base + NREG + 1, base + NREG + PAD
    stray[:3] = True
    labels = rng.integers(0, 50, size=nvox).astype(dtype)
    got, state = apply_call(eng, region, base, NREG, owner, labels)
    want, n_painted, n_outside = painted_by_numpy(region, base, NREG, owner, labels)
    assert n_outside == int(stray.sum()) >= 500 and n_painted > 300
    assert np.array_equal(got[stray], labels[stray])                       # no sentinel was painted
    assert np.array_equal(got, want) and state.tolist() == [n_painted, n_outside]


@pytest.mark.parametrize("dtype", [np.uint8, np.uint64])
@pytest.mark.parametrize("base", [0, 1, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1 - NREG - PAD])
def test_apply_box_leaves_ids_outside_the_range_alone_on_later_trips(eng, base, dtype):
    """the same with more voxels than two trips of the capped grid cover (2048 blocks of 256)"""
    test_apply_box_leaves_ids_outside_the_range_alone(eng, base, dtype, nvox=2 * 524_288 + 77)


def test_apply_box_bad_arguments(eng):
    from kimimaro_amd import _abi
    t = eng.torch
    d_region, d_owner = eng.empty(64, t.int32), eng.empty(8, t.int64)
    d_lab, d_state = eng.empty(64, t.int32), t.full((2,), 99, dtype=t.int64, device=eng.device)
    p = eng.ptr
    good = dict(region=p(d_region), base=0, nregions=7, owner=p(d_owner), labels=p(d_lab), label_bytes=4, nvox=64, state=p(d_state))
    for change in (dict(region=None), dict(owner=None), dict(labels=None), dict(state=None), dict(nvox=0), dict(nvox=2 ** 32 - 1),
                   dict(nregions=0), dict(nregions=-1), dict(base=2 ** 32 - 7), dict(base=2 ** 32 - 1, nregions=1), dict(label_bytes=3),
                   dict(label_bytes=0), dict(label_bytes=16)):
        a = dict(good, **change)
        rc = eng.lib.kh_region_apply_box(a["region"], a["base"], a["nregions"], a["owner"], a["labels"], a["label_bytes"], a["nvox"],
                                         a["state"], None)
        assert rc == 1 and "kh_region_apply_box" in _abi.last_error(), change
    assert d_state.cpu().numpy().tolist() == [99, 99]                      # a refused call writes nothing


# ---- the driver ---------------------------------------------------------------------------------------------------------------------

DATASETS = {
    "random2": lambda: H.random_dataset(2), "random4": lambda: H.random_dataset(4), "random10": lambda: H.random_dataset(10),
    "corner": lambda: H.straddling_shells()["corner"], "nested": H.nested_shells, "swapped": F.swapped_nested_shells,
    "bool": F.bool_dataset, "uint64": F.uint64_dataset, "ring2d": F.ring_2d,
}


@pytest.mark.parametrize("name", sorted(DATASETS))
def test_driver_equals_fill_all_holes_of_the_whole(name):
    from kimimaro_amd import intake, post
    dataset = DATASETS[name]()
    chunk = H.CORES[:dataset.ndim]
    mine, stats = dataset.copy(order="F"), {}
    got, count = post.fill_all_holes_chunked(mine, chunk, return_fill_count=True, stats=stats)
    print({k: v for k, v in stats.items() if k not in ("label_value", "label_state")})
    assert got is mine
    want = F.assert_same_fill(got, count, stats, dataset)
    whole, whole_count = intake.fill_all_holes(dataset.copy(order="F"), return_fill_count=True)
    assert np.array_equal(got, whole) and count == whole_count
    assert stats["cores"] == (9 if dataset.ndim == 2 else 27) and stats["cores_painted"] >= 1 and stats["apply_s"] > 0
    if name == "corner":
        assert stats["cores_painted"] == 8 < stats["cores"]
    if name == "swapped":
        assert (count, int(np.count_nonzero(got != dataset))) == (466, 396)
    if name in ("random2", "corner", "nested"):
        assert not np.array_equal(F.by_cores(dataset), want[0])          # filling box by box gives something else


def test_driver_on_a_gpu_tensor(eng):
    from kimimaro_amd import post
    dataset = H.random_dataset(4).astype(np.int32)
    want = fill_ref.static(dataset)
    assert want[1] > 0
    tensor = eng.torch.from_numpy(np.ascontiguousarray(dataset)).to(eng.device)
    out = np.zeros(dataset.shape, dtype=np.int32)
    got, count = post.fill_all_holes_chunked(tensor, H.CORES, out=out, return_fill_count=True)
    assert got is out and count == want[1] and np.array_equal(out, want[0])
    assert np.array_equal(tensor.cpu().numpy(), dataset)                   # with out= the dataset is left alone
    assert post.fill_all_holes_chunked(tensor, H.CORES) is tensor and np.array_equal(tensor.cpu().numpy(), want[0])
    with pytest.raises(ValueError, match="out"):
        post.fill_all_holes_chunked(tensor, H.CORES, out=np.zeros(dataset.shape, dtype=np.uint16))


class StaleStore:
    """a region store that loses what is written to it and hands back the ids it was made with"""

    def __init__(self, ids):
        self.ids, self.shape, self.dtype = ids, ids.shape, ids.dtype

    def __getitem__(self, key):
        return self.ids[key]

    def __setitem__(self, key, value):
        pass


def test_a_stale_region_store_is_an_error(eng, monkeypatch):
    """One core (no seam is read back in the first sweep), and a store that keeps the ids of an earlier sweep numbered from another
    base: PAD - 3 higher.  The owner table goes to the kernel inside the sentinel layout of the guard test, so that without the
    guard the stray ids would paint a sentinel and not read outside an allocation."""
    from kimimaro_amd import _abi, post
    dataset = H.straddling_shells()["corner"]
    fresh = post.region_graph_chunked(dataset, H.SHAPE)
    regions = int(fresh.bases[-1])
    stale = StaleStore(np.asfortranarray(fresh.store + np.uint32(PAD - 3)))
    assert stale.ids.min() > 0 and stale.ids.max() == regions + PAD - 3
    seen = []

    def padded(d_region, base, d_owner, d_lab, label_bytes):
        t = eng.torch
        n = int(d_owner.numel()) - 1
        buf = t.full((n + 1 + PAD,), 0x66, dtype=t.int64, device=eng.device)
        buf[1:n + 1] = d_owner[1:]
        d_state = eng.empty(2, t.int64)
        _abi.check(eng.lib.kh_region_apply_box(eng.ptr(d_region), int(base), n, eng.ptr(buf), eng.ptr(d_lab), int(label_bytes),
                                               int(d_region.numel()), eng.ptr(d_state), eng.stream()))
        state = d_state.cpu().numpy().view(np.uint64)
        seen.append((int(base), n, int(state[0]), int(state[1])))
        return int(state[0]), int(state[1])

    monkeypatch.setattr(eng, "region_apply_box", padded)
    mine = dataset.copy(order="F")
    with pytest.raises(_abi.KimiHipError, match="core 0 .*outside the core's range"):
        post.fill_all_holes_chunked(mine, H.SHAPE, region_store=stale)
    assert seen == [(0, regions, seen[0][2], int(np.count_nonzero(stale.ids > regions)))] and seen[0][3] > 0
    assert np.array_equal(mine, dataset)                                   # nothing was written back
    monkeypatch.undo()
    assert post.fill_all_holes_chunked(mine, H.SHAPE, return_fill_count=True)[1] == fill_ref.static(dataset)[1]


# ---- skeletonize_chunked(fill_holes_global=True) ------------------------------------------------------------------------------------

def test_skeletonize_chunked_fills_the_dataset_first(eng):
    """dataset 1 of tests/chunked_ref.py (the smaller one) with a block of label 2000 whose cavity lies across the cut x = 48 and holds
    a blob of label 2001, large enough for a skeleton in either box"""
    import kimimaro_amd
    from kimimaro_amd import post
    k = 1
    chunk_shape = R.DATASETS[k][3]
    dataset = np.array(R.dataset(k), copy=True, order="F")
    dataset[39:59, 19:41, 9:31] = 2000
    dataset[43:55, 23:37, 13:27] = 0
    dataset[44:54, 26:34, 16:24] = 2001
    before = dataset.copy()
    filled_volume, filled_count, _ = fill_ref.static(dataset)
    assert np.all(filled_volume[43:55, 23:37, 13:27] == 2000) and filled_count >= 12 * 14 * 14
    hip_run = lambda labels, **kwargs: kimimaro_amd.skeletonize(labels, _engine=eng, progress=False, **kwargs)
    frags = R.fragments(filled_volume, chunk_shape, hip_run, fill_holes=False)
    for label, skel in R.fused(frags).items():                             # as tests/test_gpu_chunked.py: no join hangs on a tie
        cleaned = post.remove_loops(post.remove_dust(skel.consolidate(remove_disconnected_vertices=True), R.POST_DUST))
        assert not J.join(cleaned, restrict_by_radius=True)[1], "label %d: a tree_tie decides a join" % label
    want = R.compose(frags, post.postprocess)
    timings = {}
    got = kimimaro_amd.skeletonize_chunked(dataset, chunk_shape, teasar_params=R.TP, anisotropy=R.AN, dust_threshold=R.CHUNK_DUST,
                                           post_dust_threshold=R.POST_DUST, tick_threshold=R.TICK, width=2, fill_holes=True,
                                           fill_holes_global=True, timings=timings)
    print(timings)
    R.assert_same(got, want)
    assert 2000 in frags and 2001 not in frags and 2001 not in got and np.array_equal(dataset, before)
    assert timings["filled"] == filled_count and timings["fill_s"] > 0 and timings["chunks"] == R.DATASETS[k][4]
