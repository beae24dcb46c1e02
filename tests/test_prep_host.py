"""tests/prep_ref.py held against independent definitions on small volumes (no GPU): np.bincount, scipy.ndimage, the oracle (itself
pinned to the reference's vectors in tests/golden/pdrf.npz), Python loops and hand-written tables -- so that tests/test_gpu_prep.py
does not compare the kernels with a mistake of the restatement's own."""
import itertools

import numpy as np
import pytest
import scipy.ndimage as ndi

import prep_ref

SHAPES = [(1, 1, 1), (7, 9, 5), (13, 11, 3), (65, 4, 3), (1, 70, 3), (5, 3, 1)]
bits = lambda a: np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)

# direction index -> (step, cc3d bit): the neighbour order of include/kimi_hip.h (dijkstra_invalidation.hpp:60-124) and the word the
# reference tests for it (:152-190), written out by hand
DIRECTION_TABLE = [
    ((-1, 0, 0), 1), ((1, 0, 0), 0), ((0, -1, 0), 3), ((0, 1, 0), 2), ((0, 0, -1), 5), ((0, 0, 1), 4),
    ((-1, -1, 0), 9), ((-1, 1, 0), 7), ((1, -1, 0), 8), ((1, 1, 0), 6),
    ((0, -1, -1), 17), ((0, -1, 1), 13), ((0, 1, -1), 16), ((0, 1, 1), 12),
    ((-1, 0, -1), 15), ((-1, 0, 1), 11), ((1, 0, -1), 14), ((1, 0, 1), 10),
    ((-1, -1, -1), 25), ((1, -1, -1), 24), ((-1, 1, -1), 23), ((-1, -1, 1), 21),
    ((1, 1, -1), 22), ((1, -1, 1), 20), ((-1, 1, 1), 19), ((1, 1, 1), 18),
]


def volume(shape, pattern, seed=0):
    lab = prep_ref.pattern_labels(shape, pattern, seed)
    rng = np.random.default_rng(seed + 1)
    dbf = (rng.random(shape, dtype=np.float32) * np.float32(9) + np.float32(0.5)).astype(np.float32)
    flat = dbf.reshape(-1, order="F")
    flat[rng.integers(flat.size)] = np.inf
    flat[rng.integers(flat.size)] = 0.0
    return lab, np.asfortranarray(flat.reshape(shape, order="F"))


@pytest.mark.parametrize("pattern", prep_ref.PATTERNS)
@pytest.mark.parametrize("shape", SHAPES)
def test_label_stats_against_bincount_ndimage_and_the_oracle(shape, pattern):
    import oracle
    lab, dbf = volume(shape, pattern, seed=sum(shape))
    nlabels = int(lab.max()) + 3                                  # ids without a voxel, the largest among them
    counts, dmax, first, xmin, xmax, yz = prep_ref.label_stats(lab, dbf, nlabels)
    n1 = nlabels + 1
    for out in (counts, dmax, first, xmin, xmax):
        assert out.shape == (n1,)
    assert yz.shape == (n1, 4) and dmax.dtype == np.float32 and all(o.dtype == np.uint32 for o in (counts, first, xmin, xmax, yz))
    want = np.bincount(lab.ravel(), minlength=n1)
    want[0] = 0
    np.testing.assert_array_equal(counts, want)
    present = [int(v) for v in np.unique(lab) if v != 0]
    assert present
    np.testing.assert_array_equal(bits(dmax[present]), bits(ndi.maximum(dbf, lab, present)))
    boxes = ndi.find_objects(lab.astype(np.int32), max_label=nlabels)
    for label in range(1, n1):
        if label not in present:
            assert boxes[label - 1] is None
            continue
        bx, by, bz = boxes[label - 1]
        assert (int(xmin[label]), int(xmax[label]) + 1) == (bx.start, bx.stop)
        assert [int(v) for v in yz[label]] == [by.start, by.stop - 1, bz.start, bz.stop - 1]
        pt = oracle.first_label(np.asfortranarray((lab == label).astype(np.uint8)))
        assert int(first[label]) == oracle.loc_of(pt, shape)
    for label in [0] + [v for v in range(1, n1) if v not in present]:          # the identities the header promises
        assert (int(counts[label]), bits(dmax[label:label + 1])[0], int(first[label]), int(xmin[label]), int(xmax[label])) == \
            (0, 0, 0xFFFFFFFF, 0xFFFFFFFF, 0)
        assert [int(v) for v in yz[label]] == [0xFFFFFFFF, 0, 0xFFFFFFFF, 0]


@pytest.mark.parametrize("pattern", prep_ref.PATTERNS)
@pytest.mark.parametrize("shape", SHAPES)
def test_voxel_lists_and_alive(shape, pattern):
    lab, _ = volume(shape, pattern, seed=3)
    nlabels = int(lab.max()) + 2
    present = [int(v) for v in np.unique(lab) if v != 0]
    chosen = present[::2]
    slot = np.full(nlabels + 1, -1, dtype=np.int32)
    slot[chosen[::-1]] = np.arange(len(chosen))                    # descending labels get ascending slots
    lists = prep_ref.voxel_lists(lab, slot)
    assert len(lists) == len(chosen)
    seen = np.zeros(lab.size, dtype=np.uint8)
    for label in chosen:
        got = lists[slot[label]]
        assert got.dtype == np.uint32 and (np.diff(got.astype(np.int64)) > 0).all()
        x, y, z = np.nonzero(lab == label)
        np.testing.assert_array_equal(np.sort(x + shape[0] * (y + shape[1] * z)), got)
        seen[got] = 1
    np.testing.assert_array_equal(prep_ref.alive(lab, slot), seen)
    np.testing.assert_array_equal(prep_ref.alive(lab, slot), np.isin(lab, chosen).reshape(-1, order="F").astype(np.uint8))


def loop_neighbor_mask(lab):
    sx, sy, sz = lab.shape
    out = np.zeros(lab.size, dtype=np.uint32)
    for z in range(sz):
        for y in range(sy):
            for x in range(sx):
                word = 0
                for k, ((dx, dy, dz), _) in enumerate(DIRECTION_TABLE):
                    nx, ny, nz = x + dx, y + dy, z + dz
                    if 0 <= nx < sx and 0 <= ny < sy and 0 <= nz < sz and lab[x, y, z] != 0 and lab[nx, ny, nz] == lab[x, y, z]:
                        word |= 1 << k
                out[x + sx * (y + sy * z)] = word
    return out


@pytest.mark.parametrize("pattern", ["solid", "alternating", "voronoi"])
@pytest.mark.parametrize("shape", [(1, 1, 1), (6, 5, 4), (1, 5, 4), (6, 1, 4), (6, 5, 1), (2, 2, 2)])
def test_neighbor_mask_against_a_triple_loop(shape, pattern):
    lab, _ = volume(shape, pattern, seed=5)
    got = prep_ref.neighbor_mask(lab)
    assert got.dtype == np.uint32 and not (got >> 26).any()
    np.testing.assert_array_equal(got, loop_neighbor_mask(lab))
    assert not got[lab.reshape(-1, order="F") == 0].any()
    if pattern == "solid" and min(shape) >= 3:
        assert got[1 + shape[0] * (1 + shape[1] * 1)] == (1 << 26) - 1       # an interior voxel has all 26


def test_direction_and_graph_tables():
    """prep_ref composes its two tables from the reference's rules; here they are written out one by one, and the oracle's own copies
    (the tables its searches honour a voxel graph with) say the same"""
    import oracle
    assert [step for step, _ in DIRECTION_TABLE] == list(prep_ref.DIRECTIONS)
    assert sorted(bit for _, bit in DIRECTION_TABLE) == list(range(26))
    for k, (step, bit) in enumerate(DIRECTION_TABLE):
        assert prep_ref.CC3D_STEP_OF_BIT[bit] == step
        assert int(prep_ref.allowed_directions(np.uint32(1 << bit))) == 1 << k
    assert list(oracle._DIRS) == [step for step, _ in DIRECTION_TABLE]
    assert list(oracle._GRAPH_BIT) == [bit for _, bit in DIRECTION_TABLE]
    assert int(prep_ref.allowed_directions(np.uint32(0xFFFFFFFF))) == (1 << 26) - 1
    assert int(prep_ref.allowed_directions(np.uint32(0xFC000000))) == 0


def test_apply_voxel_graph_against_the_table():
    rng = np.random.default_rng(11)
    lab, _ = volume((6, 5, 4), "voronoi", seed=2)
    nbr = prep_ref.neighbor_mask(lab)
    graph = rng.integers(0, 1 << 32, nbr.size, dtype=np.uint64).astype(np.uint32)
    graph[0], graph[1] = 0xFFFFFFFF, 0
    got, gate = prep_ref.apply_voxel_graph(nbr, graph)
    assert got.dtype == np.uint32 and gate.dtype == np.uint8
    for v in range(nbr.size):
        word = 0
        for k, (_, bit) in enumerate(DIRECTION_TABLE):
            if (int(nbr[v]) >> k) & 1 and (int(graph[v]) >> bit) & 1:
                word |= 1 << k
        assert int(got[v]) == word
        want_gate = 0
        for j in range(8):
            (_, dy, dz), bit = DIRECTION_TABLE[18 + j]
            diagonal = [step for step, _ in DIRECTION_TABLE].index((0, dy, dz))
            if (int(nbr[v]) >> diagonal) & 1 and (int(graph[v]) >> bit) & 1:
                want_gate |= 1 << j
        assert int(gate[v]) == want_gate
    np.testing.assert_array_equal(prep_ref.apply_voxel_graph(nbr, np.full(nbr.size, 0xFFFFFFFF, np.uint32))[0], nbr)
    assert not prep_ref.apply_voxel_graph(nbr, np.zeros(nbr.size, np.uint32))[0].any()
    assert gate.any() and (gate != prep_ref.apply_voxel_graph(nbr, np.full(nbr.size, 0xFFFFFFFF, np.uint32))[1]).any()


def pdrf_case(seed=4, shape=(12, 7, 5)):
    """labels 1..4 as blobs and a one-voxel label 6, with a DBF and a DAF per voxel; tasks as plan.py fills them"""
    rng = np.random.default_rng(seed)
    lab = prep_ref.pattern_labels(shape, "voronoi", seed)
    lab[lab == 5] = 4
    lab[3, 2, 1] = 6
    dbf = np.asfortranarray((rng.random(shape) * 6 + 0.25).astype(np.float32))
    daf = np.asfortranarray((rng.random(shape) * 300).astype(np.float32))
    daf.reshape(-1, order="F")[rng.choice(lab.size, 12, replace=False)] = np.inf
    daf[3, 2, 1] = np.inf
    labels = [1, 2, 3, 4, 6]
    slot = np.full(9, -1, dtype=np.int32)
    slot[labels] = rng.permutation(len(labels))
    tasks = np.zeros(len(labels), dtype=[("M", "<f4"), ("max_val", "<f4")])
    f = np.float32
    for label in labels:
        inside = lab == label
        tasks["M"][slot[label]] = f(1 / (f(dbf[inside].max()) ** 1.01))
        finite = daf[inside][np.isfinite(daf[inside])]
        tasks["max_val"][slot[label]] = finite.max() if finite.size else 0
    assert tasks["max_val"][slot[6]] == 0
    return lab, dbf, daf, labels, slot, tasks


@pytest.mark.parametrize("exponent", [1, 4, 16, 2 ** 15, 3])
def test_pdrf_per_label_against_the_oracle(exponent):
    import oracle
    lab, dbf, daf, labels, slot, tasks = pdrf_case()
    scale = 5000.0
    if exponent & (exponent - 1) == 0:
        got, got_daf = prep_ref.pdrf(lab, slot, tasks, dbf, daf, int(np.log2(exponent)), scale)
    else:                                                          # the two halves around the host's np.power
        base, same_daf = prep_ref.pdrf(lab, slot, tasks, dbf, daf, prep_ref.PDRF_BASE, scale)
        np.testing.assert_array_equal(bits(same_daf), bits(daf.reshape(-1, order="F")))
        np.power(base, exponent, out=base)
        got, got_daf = prep_ref.pdrf(lab, slot, tasks, dbf, daf, prep_ref.PDRF_FINISH, scale, pdrf_in=base)
    background = (lab == 0).reshape(-1, order="F")
    assert background.any() and np.isposinf(got[background]).all()
    np.testing.assert_array_equal(bits(got_daf[background]), bits(daf.reshape(-1, order="F")[background]))
    for label in labels:
        inside = lab == label
        own_dbf = oracle.zero2inf(np.asfortranarray(np.where(inside, dbf, np.float32(0)).astype(np.float32)))
        own_daf = oracle.inf2zero(np.asfortranarray(np.where(inside, daf, np.float32(np.inf)).astype(np.float32)))
        want = oracle.compute_pdrf(dbf[inside].max(), scale, exponent, own_dbf, own_daf, tasks["max_val"][slot[label]])
        flat = inside.reshape(-1, order="F")
        np.testing.assert_array_equal(bits(got[flat]), bits(want.reshape(-1, order="F")[flat]))
        np.testing.assert_array_equal(bits(got_daf[flat]), bits(own_daf.reshape(-1, order="F")[flat]))


def test_pdrf_keep_others_and_partial_selection():
    lab, dbf, daf, labels, slot, tasks = pdrf_case()
    full, full_daf = prep_ref.pdrf(lab, slot, tasks, dbf, daf, 2, 100.0)
    part = slot.copy()
    part[[2, 3, 6]] = -1                                            # labels 1 and 4 stay, with the slots (and tasks) they had
    before = np.arange(lab.size, dtype=np.uint32).view(np.float32)  # distinct bit patterns
    kept, kept_daf = prep_ref.pdrf(lab, part, tasks, dbf, daf, 2, 100.0, keep=True, pdrf_in=before)
    plain, plain_daf = prep_ref.pdrf(lab, part, tasks, dbf, daf, 2, 100.0, pdrf_in=before)
    mine = np.isin(lab, [1, 4]).reshape(-1, order="F")
    for out, out_daf in ((kept, kept_daf), (plain, plain_daf)):
        np.testing.assert_array_equal(bits(out[mine]), bits(full[mine]))
        np.testing.assert_array_equal(bits(out_daf[mine]), bits(full_daf[mine]))
        np.testing.assert_array_equal(bits(out_daf[~mine]), bits(daf.reshape(-1, order="F")[~mine]))
    np.testing.assert_array_equal(bits(kept[~mine]), bits(before[~mine]))
    assert np.isposinf(plain[~mine]).all()


def test_level_keys_against_float64():
    """every float32 operation of the key, redone in float64 and rounded: products and sums of float32 numbers are exact in float64
    before the rounding, and the square root of a float32 rounds the same way from float64 (53 >= 2 * 24 + 2 bits)"""
    f, d = np.float32, np.float64
    dims, w = (9, 6, 5), (3.7, 1.3, 2.2)
    got = prep_ref.level_keys(dims, w)
    assert got.shape == dims and got.dtype == np.float32
    for a, b, c in itertools.product(*[range(n) for n in dims]):
        fa, fb, fc = [f(d(f(wi)) * d(n)) for wi, n in zip(w, (a, b, c))]
        qa, qb, qc = [f(d(v) * d(v)) for v in (fa, fb, fc)]
        s = f(d(f(d(qa) + d(qb))) + d(qc))
        assert got[a, b, c].view(np.uint32) == f(np.sqrt(d(s))).view(np.uint32)
