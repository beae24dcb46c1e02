"""GPU: kh_nearest_label_voxels_box and synapses_to_targets_chunked.  The kernel, one visit at a time, against the
numpy statement of tests/synapses_chunked_ref.py -- distances as bit patterns, indices as integers of the dataset --, its carry
rule from box to box, and the driver against tests/points_ref.py::synapses_to_targets of the whole dataset, item for item in
insertion order.  Every comparison is exact."""
import functools

import numpy as np
import pytest

import chunked_ref
import points_ref
import synapses_chunked_ref as S

pytestmark = pytest.mark.gpu

U32 = (0, 2 ** 32 - 1)


@pytest.fixture(scope="module")
def eng():
    from kimimaro_amd import ops
    return ops.engine()


def running(eng, a):
    """u64 host words -> int64 device tensor"""
    return eng.torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64).copy()).to(eng.device)


def kernel_visit(eng, box, lo, shape, words, query_start, centroids, query_index, best_distance, best_voxel):
    """tests/synapses_chunked_ref.py::visit, by the kernel: the running arrays go up, one call, and come back (changed in place)"""
    from kimimaro_amd import points
    box = np.asfortranarray(box)
    d_best, d_vox = running(eng, best_distance), running(eng, best_voxel)
    points.nearest_label_voxels_box(eng, eng.to_device(box.view("u%d" % box.dtype.itemsize)), box.dtype.itemsize, box.shape, lo, shape,
                                    words, query_start, centroids, query_index, d_best, d_vox)
    best_distance[:] = d_best.cpu().numpy().view(np.uint64)
    best_voxel[:] = d_vox.cpu().numpy().view(np.uint64)


def fresh(n):
    return np.full(n, S.NONE64, dtype=np.uint64), np.full(n, S.NONE64, dtype=np.uint64)


def queries_of(synapses, span=U32, itemsize=4):
    from kimimaro_amd import intake
    _, words, query_start, centroids = intake.synapse_queries(synapses, span, itemsize)
    return words, query_start, centroids, np.arange(centroids.shape[0], dtype=np.uint32)


def assert_visits_agree(eng, box, lo, shape, queries, incoming=None):
    """one visit by the kernel and by the statement, from the same incoming state -> the (distance, voxel) arrays"""
    n = int(queries[3].max()) + 1
    got = fresh(n) if incoming is None else tuple(a.copy() for a in incoming)
    want = tuple(a.copy() for a in got)
    kernel_visit(eng, box, lo, shape, *queries, *got)
    S.visit(box, lo, shape, *queries, *want)
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])
    return got


# ---------------------------------------------------------------------------------------------------------------- the kernel
def test_the_whole_volume_as_one_box(eng):
    from kimimaro_amd import points
    lab = S.dataset()
    queries = queries_of(S.scattered(lab))
    dist, vox = assert_visits_agree(eng, lab, (0, 0, 0), lab.shape, queries)
    winners = points.nearest_label_voxels(eng, eng.to_device(lab), 4, lab.shape, *queries[:3])
    np.testing.assert_array_equal(vox, winners)
    absent = vox == S.NONE64
    assert absent.sum() == 2 and (dist[absent] == S.NONE64).all() and np.isfinite(dist[~absent].view(np.float64)).all()


def test_a_box_at_its_offset(eng):
    lab = S.dataset()
    lo, hi = (5, 3, 2), (21, 16, 13)
    box = lab[5:21, 3:16, 2:13]
    dist, vox = assert_visits_agree(eng, box, lo, lab.shape, queries_of(S.scattered(lab)))
    found = vox[vox != S.NONE64].astype(np.int64)
    assert found.size >= 18                 # at least three labels of the dataset occur in the box
    x, y, z = found // (lab.shape[1] * lab.shape[2]), (found // lab.shape[2]) % lab.shape[1], found % lab.shape[2]
    assert ((x >= lo[0]) & (x < hi[0]) & (y >= lo[1]) & (y < hi[1]) & (z >= lo[2]) & (z < hi[2])).all()      # dataset coordinates


def tie_cases():
    """[(label, centroid, the two cores (lo, hi) its tie spans)] of the cut ties at (16, 13, 11)"""
    from kimimaro_amd import plan
    lab, chunk = S.dataset(), S.CHUNKS[0]
    grid = plan.chunk_grid(lab.shape, chunk, overlap=0)
    synapses = S.cut_ties(lab, chunk)
    cases = []
    for (label, centroid), voxels in zip(((L, c) for L, pairs in synapses.items() for c, _ in pairs), S.nearest_sets(lab, synapses)):
        cores = sorted(set(plan.core_of(voxels, lab.shape, chunk).tolist()))
        assert len(cores) == 2
        cases.append((label, centroid, [(grid.core_lo[k], grid.core_hi[k]) for k in cores]))
    return cases


def test_the_two_cores_of_a_tie_in_both_orders(eng):
    lab = S.dataset()
    cases = tie_cases()
    assert len(cases) == 18
    for label, centroid, cores in cases:
        queries = queries_of({label: [(centroid, 0)]})
        ends = []
        for order in (cores, cores[::-1]):
            state = None
            for lo, hi in order:
                box = lab[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]]
                state = assert_visits_agree(eng, box, lo, lab.shape, queries, state)
            ends.append((int(state[0][0]), int(state[1][0])))
        lower = min(S.c_index(np.floor(centroid), lab.shape), S.c_index(np.ceil(centroid), lab.shape))
        assert ends[0] == ends[1] == (int(np.float64(0.5).view(np.uint64)), lower)


def test_the_four_incoming_states(eng):
    """the same query four times, on four rows, against the SECOND core of its tie: the box holds (0.5, own) and nothing nearer"""
    lab = S.dataset()
    label, centroid, cores = tie_cases()[0]
    lo, hi = cores[1]
    box = lab[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]]
    own = S.c_index(np.ceil(centroid), lab.shape)
    bits = lambda d: int(np.float64(d).view(np.uint64))
    queries = queries_of({label: [(centroid, 0)] * 4})
    incoming = (np.array([bits(0.25), bits(0.5), bits(0.5), bits(0.75)], dtype=np.uint64),
                np.array([12345, own - 1, own + 1, 3], dtype=np.uint64))
    dist, vox = assert_visits_agree(eng, box, lo, lab.shape, queries, incoming)
    assert list(zip(dist.tolist(), vox.tolist())) == [
        (bits(0.25), 12345),          # nearer incoming: unchanged
        (bits(0.5), own - 1),         # equal distance, lower incoming index: unchanged
        (bits(0.5), own),             # equal distance, higher incoming index: the index is replaced
        (bits(0.5), own)]             # farther incoming: both replaced -- the stale index 3, although lower, is not kept


def test_unlisted_rows_are_not_touched(eng):
    lab = S.dataset()
    words, query_start, centroids, _ = queries_of(S.clustered(lab, per_label=1))
    assert centroids.shape[0] == 7
    rows = np.array([9, 2, 11, 5, 0, 7, 4], dtype=np.uint32)              # a permuted strict subset of 12 rows
    sentinel = (np.arange(12, dtype=np.uint64) * np.uint64(0x0123456789ABCDEF)) | np.uint64(1 << 63)
    incoming = (sentinel.copy(), sentinel[::-1].copy())
    incoming[0][rows], incoming[1][rows] = S.NONE64, S.NONE64
    dist, vox = assert_visits_agree(eng, lab[5:21, 3:16, 2:13], (5, 3, 2), lab.shape, (words, query_start, centroids, rows), incoming)
    unlisted = np.setdiff1d(np.arange(12), rows)
    np.testing.assert_array_equal(dist[unlisted], sentinel[unlisted])
    np.testing.assert_array_equal(vox[unlisted], sentinel[::-1][unlisted])
    assert (dist[rows] != S.NONE64).sum() >= 3


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.uint32, np.uint64], ids=lambda d: np.dtype(d).name)
def test_lane_boundaries_and_label_widths(eng, dtype):
    """a box of two x tiles whose labels change between lanes 63 | 64 and tiles 255 | 256"""
    base = {1: 3, 2: 300, 4: 70000, 8: 2 ** 32 + 5}[np.dtype(dtype).itemsize]
    box = np.empty((300, 3, 2), dtype=dtype, order="F")
    box[:64], box[64:256], box[256:] = base, base + 1, base + 2
    box[60:70, 1, 1] = base + 2
    box[250:260, 2, 0] = base
    lo, shape = (3, 4, 5), (400, 20, 20)
    rng = np.random.default_rng(17)
    info = np.iinfo(dtype)
    synapses = {base + k: [(tuple((rng.integers(0, 8 * 320, 3) / 8.0 * [1, 0.03, 0.03]).tolist()), 0) for _ in range(5)] for k in range(4)}
    synapses[base + 1] += [((63.5 + 3, 5.0, 6.0), 0), ((255.5 + 3, 4.0, 5.0), 0), ((258.0, 6.5, 5.5), 0)]       # ties across the changes
    dist, vox = assert_visits_agree(eng, box, lo, shape, queries_of(synapses, (int(info.min), int(info.max)), np.dtype(dtype).itemsize))
    assert (vox == S.NONE64).sum() == 5                                    # base + 3 does not occur


def test_blocks_of_several_tiles_by_both_entry_points(eng):
    """a box of 2 x 65 x 64 = 8 320 x tiles: the launch is capped at 4 096 blocks, so a block walks 3 tiles (2 774 blocks, the last one
    short) and carries its looked-up label from tile to tile; the second tile of every row has one lane inside the box (x = 256).
    The whole-volume entry and the box entry at lo = 0 with an identity query_index run the one sweep and must agree"""
    from kimimaro_amd import points
    shape = (257, 65, 64)
    assert -(-shape[0] // 256) * shape[1] * shape[2] == 8320 and -(-8320 // 4096) == 3 and -(-8320 // 3) == 2774
    box = np.empty(shape, dtype=np.uint16, order="F")
    box[:, :20], box[:, 20:45], box[:, 45:] = 500, 501, 502                # slabs along y: a row's label is its neighbour's, mostly
    box[100:140, 18:24, 30:] = 503                                         # an island across a slab boundary
    box[256, 7:60, 3:50] = 504                                             # a label confined to x >= 256, the lone lane of its tile
    rng = np.random.default_rng(23)
    synapses = {label: [(tuple((rng.integers(-8 * 6, 8 * (np.array(shape) + 6)) / 8.0).tolist()), 0) for _ in range(5)]
                for label in (500, 501, 502, 503, 504, 505)}               # 505 occurs nowhere
    queries = queries_of(synapses, (0, 65535), 2)
    want = fresh(30)
    S.visit(box, (0, 0, 0), shape, *queries, *want)
    assert (want[1] == S.NONE64).sum() == 5 and (want[1][20:25] // (shape[1] * shape[2]) == 256).all()
    dist, vox = fresh(30)
    kernel_visit(eng, box, (0, 0, 0), shape, *queries, dist, vox)
    winners = points.nearest_label_voxels(eng, eng.to_device(box), 2, shape, *queries[:3])
    np.testing.assert_array_equal(dist, want[0])
    np.testing.assert_array_equal(vox, want[1])
    np.testing.assert_array_equal(winners, want[1])
    np.testing.assert_array_equal(winners, vox)


def test_indices_beyond_2_to_the_32(eng):
    shape = (2 ** 21 + 8, 2 ** 20, 2 ** 20)
    lo = (2 ** 21, 2 ** 20 - 8, 2 ** 20 - 8)
    box = np.asfortranarray(np.random.default_rng(3).integers(1, 4, size=(8, 8, 8)).astype(np.uint16))
    near = np.array(lo, dtype=np.float64)
    synapses = {k: [(tuple((near + off).tolist()), 0) for off in ((3.5, 3.5, 3.5), (-2.0, 9.0, 4.25), (100.0, -50.0, 7.0))] for k in (1, 2, 3)}
    dist, vox = assert_visits_agree(eng, box, lo, shape, queries_of(synapses, (0, 65535), 2))
    for k, v in enumerate(int(v) for v in vox):
        x, y, z = v // (shape[1] * shape[2]), (v // shape[2]) % shape[1], v % shape[2]
        assert v > 2 ** 60 and all(a <= c < a + 8 for a, c in zip(lo, (x, y, z))), (k, v)
        assert int(box[x - lo[0], y - lo[1], z - lo[2]]) == 1 + k // 3


# ---------------------------------------------------------------------------------------------------------------- the driver
@functools.lru_cache(maxsize=None)
def case(kind, chunk_shape):
    """(synapses, the items of points_ref on the whole dataset, the stats of the host run)"""
    lab = S.dataset()
    synapses = {"scattered": S.scattered, "clustered": S.clustered}[kind](lab) if kind != "cut_ties" else S.cut_ties(lab, chunk_shape)
    stats = {}
    host = S.host_driver(lab, synapses, chunk_shape, stats=stats)
    want = list(points_ref.synapses_to_targets(lab, synapses).items())
    assert list(host.items()) == want and want
    return synapses, want, stats


@pytest.mark.parametrize("kind,chunk_shape", [("scattered", S.CHUNKS[0]), ("clustered", S.CHUNKS[0]), ("cut_ties", S.CHUNKS[0]),
                                              ("cut_ties", S.CHUNKS[1])], ids=str)
def test_driver_equals_the_whole_dataset(kind, chunk_shape):
    import kimimaro_amd
    synapses, want, host = case(kind, chunk_shape)
    stats = {}
    got = kimimaro_amd.synapses_to_targets_chunked(S.dataset(), synapses, chunk_shape, stats=stats)
    assert list(got.items()) == want
    assert all(type(v) is int for key in got for v in key)
    # the culling decisions are exact: the same cores and the same queries as the host run of the same input
    assert (stats["cores"], stats["cores_visited"], stats["pairs"]) == (host["cores"], host["cores_visited"], host["pairs"])
    assert stats["cores_skipped"] == stats["cores"] - stats["cores_visited"] and stats["load_s"] > 0 and stats["visit_s"] > 0


def test_driver_dataset_forms(eng, tmp_path):
    import kimimaro_amd
    lab = S.dataset()
    synapses, want, host = case("clustered", S.CHUNKS[0])
    mm = np.lib.format.open_memmap(str(tmp_path / "labels.npy"), mode="w+", dtype=lab.dtype, shape=lab.shape)
    mm[:] = lab
    mm.flush()
    tensor = eng.torch.from_numpy(np.ascontiguousarray(lab).astype(np.int32)).to(eng.device)
    for form in (np.ascontiguousarray(lab), tensor, np.load(str(tmp_path / "labels.npy"), mmap_mode="r")):
        stats = {}
        assert list(kimimaro_amd.synapses_to_targets_chunked(form, synapses, S.CHUNKS[0], stats=stats).items()) == want
        assert (stats["cores_visited"], stats["pairs"]) == (host["cores_visited"], host["pairs"])


def test_skeletonize_chunked_takes_synapses():
    import kimimaro_amd
    from kimimaro_amd import plan
    k = 1                                                   # the smaller dataset of tests/chunked_ref.py: six boxes
    lab, chunk_shape = chunked_ref.dataset(k), chunked_ref.DATASETS[k][3]
    rng = np.random.default_rng(8)
    synapses = {int(label): [(tuple(rng.uniform(0, lab.shape).tolist()), int(rng.integers(0, 3))) for _ in range(2)]
                for label in np.unique(lab)[:5].tolist()}
    targets = points_ref.synapses_to_targets(lab, synapses)
    assert len(targets) >= 8
    # a target in another core than its centroid: what a call per box cannot find
    apart = 0
    for label, pairs in synapses.items():
        for centroid, swc in pairs:
            (voxel, _), = points_ref.synapses_to_targets(lab, {label: [(centroid, swc)]}).items()
            cores = plan.core_of([voxel, np.floor(centroid).astype(np.int64)], lab.shape, chunk_shape)
            apart += int(cores[0] != cores[1])
    assert apart >= 1
    kw = dict(teasar_params=chunked_ref.TP, anisotropy=chunked_ref.AN, dust_threshold=chunked_ref.CHUNK_DUST,
              post_dust_threshold=chunked_ref.POST_DUST, tick_threshold=0, width=2)
    want = kimimaro_amd.skeletonize_chunked(lab, chunk_shape, extra_targets_after=list(targets), **kw)
    got = kimimaro_amd.skeletonize_chunked(lab, chunk_shape, synapses=synapses, **kw)
    chunked_ref.assert_same(got, want)
    an = np.array(chunked_ref.AN, dtype=np.float32)
    rows = {tuple(v) for s in got.values() for v in s.vertices.tolist()}
    assert sum(tuple((np.array(t, dtype=np.float32) * an).tolist()) in rows for t in targets) >= 1
