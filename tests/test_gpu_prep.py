"""The streaming kernels of csrc/prep.hip and kh_level_keys, each called through the C ABI and compared with its numpy restatement
(tests/prep_ref.py, pinned by tests/test_prep_host.py) -- integers exactly, float32 as bit patterns, no tolerance anywhere.  The
shapes are the smallest at which the wave-run logic, the 256-voxel chunks and the grid-stride loops can go wrong; every output
lies between guard words that must come back untouched."""
import ctypes as C
import functools

import numpy as np
import pytest

import prep_ref

pytestmark = pytest.mark.gpu

DTYPES = [np.uint8, np.uint16, np.uint32]
# several rows share a wave / rows cross the 256-voxel chunks / tails and degenerate sizes
STAT_SHAPES = [(7, 9, 5), (13, 11, 3), (63, 5, 2), (64, 4, 2), (65, 4, 3),
               (255, 3, 2), (256, 2, 2), (257, 3, 1), (300, 5, 1),
               (1, 1, 1), (5, 3, 1), (1, 70, 3)]
MASK_SHAPES = [(1, 1, 1), (1, 9, 7), (9, 1, 7), (9, 7, 1), (2, 2, 2), (255, 3, 3), (256, 3, 2), (257, 2, 3), (513, 2, 2)]
GUARD = 16                      # words (bytes for a u8 output) on either side of every output
WORD, BYTE = 0xA5A5A5A5, 0xA5   # what they hold
ONE_PASS = 8192 * 256           # voxels the capped grid of the element-wise kernels covers in one pass
EINVAL = 1


@pytest.fixture(scope="module")
def eng():
    from kimimaro_amd.engine import Engine
    return Engine()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


class Out:
    """a device buffer of n u32 (or u8) elements between two guards; the library gets the address of the body"""

    def __init__(self, eng, n, dtype=np.uint32, init=None):
        self.n, self.dtype = int(n), np.dtype(dtype)
        self.sentinel = WORD if self.dtype.itemsize == 4 else BYTE
        host = np.full(self.n + 2 * GUARD, self.sentinel, dtype=self.dtype)
        if init is not None:
            host[GUARD:GUARD + self.n] = np.asarray(init).view(self.dtype) if np.asarray(init).dtype.itemsize == self.dtype.itemsize \
                else np.asarray(init, dtype=self.dtype)
        self.dev = eng.to_device(host)
        self.ptr = C.c_void_p(self.dev.data_ptr() + GUARD * self.dtype.itemsize)

    def read(self):
        """the body, after checking that no word outside it changed"""
        host = self.dev.cpu().numpy().view(self.dtype)
        assert (host[:GUARD] == self.sentinel).all(), "the words in front of the output were written"
        assert (host[GUARD + self.n:] == self.sentinel).all(), "the words behind the output were written"
        return host[GUARD:GUARD + self.n].copy()


@functools.lru_cache(maxsize=None)
def pattern(shape, name):
    return prep_ref.pattern_labels(shape, name, seed=sum(shape))


def run_starts(flat, sx):
    """where a wave of 64 consecutive voxels starts a new run of equal labels: at its first lane, at x == 0, at a change of label"""
    i = np.arange(flat.size)
    start = (i % 64 == 0) | (i % sx == 0)
    start[1:] |= flat[1:] != flat[:-1]
    return np.flatnonzero(start)


def planted_dbf(lab, salt):
    """random positive float32 with, per label, its maximum at the first, the last or a middle lane of one of its runs (+inf for one
    label), and one label that is 0.0 everywhere but for a subnormal"""
    rng = np.random.default_rng(salt)
    flat = lab.reshape(-1, order="F")
    dbf = (rng.random(flat.size, dtype=np.float32) * np.float32(9) + np.float32(0.5)).astype(np.float32)
    starts = run_starts(flat, lab.shape[0])
    ends = np.append(starts[1:], flat.size) - 1
    present = [int(v) for v in np.unique(flat) if v != 0]
    for n, label in enumerate(present):
        own = np.flatnonzero(flat[starts] == label)
        if n == 1:                                                  # this one's maximum is a subnormal among zeros
            dbf[flat == label] = 0.0
            dbf[starts[own[len(own) // 2]]] = np.float32(1e-42)
            continue
        length = ends[own] - starts[own] + 1
        run = own[np.argmax(length >= 2)] if (length >= 2).any() else own[0]         # the first run of two or more voxels
        lane = [starts[run], ends[run], (starts[run] + ends[run] + 1) // 2][(n + salt) % 3]
        dbf[lane] = np.inf if (n + salt) % 4 == 0 else np.float32(1000 + label)
    background = np.flatnonzero(flat == 0)
    if background.size:
        dbf[background[0]] = np.inf                                 # not a voxel of any label: must not reach a maximum
    return dbf


def stats_call(eng, flat, dtype, dbf, shape, nlabels, with_yz=True, label_bytes=None):
    n1 = nlabels + 1
    d_lab, d_dbf = eng.to_device(flat.astype(dtype)), eng.to_device(dbf)
    outs = [Out(eng, n1) for _ in range(5)] + [Out(eng, 4 * n1)]
    rc = eng.lib.kh_label_stats(eng.ptr(d_lab), label_bytes or np.dtype(dtype).itemsize, eng.ptr(d_dbf), flat.size, shape[0], shape[1],
                                nlabels, *[o.ptr for o in outs[:5]], outs[5].ptr if with_yz else C.c_void_p(0), eng.stream())
    eng.sync()
    return rc, outs


def check_stats(eng, flat, dtype, dbf, shape, nlabels):
    from kimimaro_amd import _abi
    want = prep_ref.label_stats(flat.reshape(shape, order="F"), dbf.reshape(shape, order="F"), nlabels)
    for with_yz in (True, False):
        rc, outs = stats_call(eng, flat, dtype, dbf, shape, nlabels, with_yz)
        _abi.check(rc)
        got = [o.read() for o in outs]
        for name, g, w in zip(("counts", "dbf_max", "first_index", "xmin", "xmax"), got, want):
            np.testing.assert_array_equal(g, bits(w) if name == "dbf_max" else w, err_msg=name)
        if with_yz:
            np.testing.assert_array_equal(got[5].reshape(-1, 4), want[5], err_msg="yz_extent")
        else:
            assert (got[5] == WORD).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("name", prep_ref.PATTERNS)
@pytest.mark.parametrize("shape", STAT_SHAPES, ids=str)
def test_label_stats(eng, shape, name, dtype):
    flat = pattern(shape, name).reshape(-1, order="F")
    salt = STAT_SHAPES.index(shape) + DTYPES.index(dtype)
    dbf = planted_dbf(pattern(shape, name), salt)
    check_stats(eng, flat, dtype, dbf, shape, int(flat.max()) + 3)
    if dtype is np.uint8:                                           # the largest id a byte holds, present, as the last table entry
        top = flat.copy()
        top[top == top.max()] = 255
        check_stats(eng, top, dtype, dbf, shape, 255)


@functools.lru_cache(maxsize=None)
def big_volume():
    """(160, 128, 128): more voxels than one pass of the capped grid covers; blocks of labels, some only behind the first pass"""
    shape = (160, 128, 128)
    assert np.prod(shape) > ONE_PASS
    rng = np.random.default_rng(7)
    x, y, z = np.meshgrid(*[np.arange(n) for n in shape], indexing="ij")
    lab = 1 + x // 40 + 4 * (y // 50) + 12 * (z // 35)
    lab[rng.random(shape) < 0.05] = 0
    flat = np.ascontiguousarray(lab.reshape(-1, order="F"))
    assert set(np.unique(flat[ONE_PASS:])) - set(np.unique(flat[:ONE_PASS]))
    dbf = (rng.random(flat.size, dtype=np.float32) * np.float32(50)).astype(np.float32)
    return shape, flat, dbf


def test_label_stats_grid_stride(eng):
    shape, flat, dbf = big_volume()
    check_stats(eng, flat, np.uint16, dbf, shape, int(flat.max()) + 2)


def scatter_case(flat, nlabels, salt):
    """about half the labels, slots in shuffled order, lists laid out in another shuffled order with a gap after each"""
    rng = np.random.default_rng(100 + salt)
    present = np.array([v for v in np.unique(flat) if v != 0])
    chosen = rng.permutation(present)[:max(1, present.size // 2)]
    slot = np.full(nlabels + 1, -1, dtype=np.int32)
    slot[chosen] = np.arange(chosen.size)
    counts = np.array([(flat == label).sum() for label in chosen])
    offsets = np.zeros(chosen.size, dtype=np.uint32)
    at = GUARD
    for s in rng.permutation(chosen.size):
        offsets[s] = at
        at += int(counts[s]) + GUARD
    return slot, counts, offsets, at


def check_scatter(eng, flat, dtype, shape, slot, counts, offsets, total):
    from kimimaro_amd import _abi
    nslots = counts.size
    d_lab, d_slot, d_off = eng.to_device(flat.astype(dtype)), eng.to_device(slot), eng.to_device(offsets)
    cursors, lists = Out(eng, nslots), Out(eng, total)
    _abi.check(eng.lib.kh_scatter_lists(eng.ptr(d_lab), np.dtype(dtype).itemsize, flat.size, eng.ptr(d_slot), nslots, eng.ptr(d_off),
                                        cursors.ptr, lists.ptr, eng.stream()))
    eng.sync()
    want = prep_ref.voxel_lists(flat.reshape(shape, order="F"), slot)
    np.testing.assert_array_equal(cursors.read(), counts.astype(np.uint32))
    got = lists.read()
    inside = np.zeros(total, dtype=bool)
    for s in range(nslots):
        inside[offsets[s]:offsets[s] + counts[s]] = True
        np.testing.assert_array_equal(np.sort(got[offsets[s]:offsets[s] + counts[s]]), want[s])
    assert (got[~inside] == WORD).all(), "a guard word between the lists was written"
    assert (slot[flat[got[inside]]] >= 0).all()                    # no entry belongs to an unselected label


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("name", prep_ref.PATTERNS)
@pytest.mark.parametrize("shape", STAT_SHAPES, ids=str)
def test_scatter_lists(eng, shape, name, dtype):
    flat = pattern(shape, name).reshape(-1, order="F")
    nlabels = int(flat.max()) + 3
    check_scatter(eng, flat, dtype, shape, *scatter_case(flat, nlabels, STAT_SHAPES.index(shape)))


def test_scatter_lists_grid_stride(eng):
    shape, flat, _ = big_volume()
    check_scatter(eng, flat, np.uint16, shape, *scatter_case(flat, int(flat.max()) + 2, 0))


def test_scatter_lists_single_object(eng):
    """as Engine.single_object calls it: a 0 / 1 volume of 4-byte labels, one slot, the table [-1, 0]"""
    shape = (65, 4, 3)
    flat = (pattern(shape, "voronoi").reshape(-1, order="F") > 2).astype(np.int64)
    count = int(flat.sum())
    assert 0 < count < flat.size
    check_scatter(eng, flat, np.uint32, shape, np.array([-1, 0], dtype=np.int32), np.array([count]), np.array([GUARD], dtype=np.uint32),
                  GUARD + count + GUARD)


def mask_labels(shape, name):
    if name == "checkerboard":
        x, y, z = np.meshgrid(*[np.arange(n) for n in shape], indexing="ij")
        return 1 + (x + y + z) % 2                                  # face neighbours differ, edge neighbours agree
    return pattern(shape, name)


def neighbor_mask_call(eng, lab, dtype):
    from kimimaro_amd import _abi
    flat = lab.reshape(-1, order="F")
    d_lab = eng.to_device(flat.astype(dtype))
    out = Out(eng, flat.size)
    _abi.check(eng.lib.kh_neighbor_mask(eng.ptr(d_lab), np.dtype(dtype).itemsize, lab.shape[0], lab.shape[1], lab.shape[2], out.ptr,
                                        eng.stream()))
    eng.sync()
    return out.read()


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("name", ["solid", "checkerboard", "voronoi"])
@pytest.mark.parametrize("shape", MASK_SHAPES, ids=str)
def test_neighbor_mask(eng, shape, name, dtype):
    lab = mask_labels(shape, name)
    np.testing.assert_array_equal(neighbor_mask_call(eng, lab, dtype), prep_ref.neighbor_mask(lab))


def test_neighbor_mask_beyond_the_tile_cap(eng):
    """(2, 1100, 1000): one row tile per (y, z), more of them than the 2^20 blocks the launch is capped at"""
    shape = (2, 1100, 1000)
    assert shape[1] * shape[2] > 1 << 20
    x, y, z = np.meshgrid(*[np.arange(n) for n in shape], indexing="ij")
    lab = 1 + (y // 7 + 3 * (z // 5) + x) % 250                     # bands, thinner than the neighbourhood in places
    lab[(y * 31 + z * 17) % 23 == 0] = 0
    np.testing.assert_array_equal(neighbor_mask_call(eng, lab, np.uint8), prep_ref.neighbor_mask(lab))


@pytest.mark.parametrize("with_gate", [True, False])
@pytest.mark.parametrize("shape,name", [((257, 2, 3), "voronoi"), ((513, 2, 2), "solid"), ((9, 7, 1), "checkerboard")], ids=str)
def test_apply_voxel_graph(eng, shape, name, with_gate):
    from kimimaro_amd import _abi
    nbr = prep_ref.neighbor_mask(mask_labels(shape, name))
    assert nbr.size % 256 != 0
    rng = np.random.default_rng(nbr.size)
    graph = rng.integers(0, 1 << 32, nbr.size, dtype=np.uint64).astype(np.uint32)
    graph[::5] |= np.uint32(0xFC000000)                             # bits above 25 mean nothing
    graph[1], graph[2] = 0xFFFFFFFF, 0
    want, want_gate = prep_ref.apply_voxel_graph(nbr, graph)
    assert want_gate.any() or name != "solid"
    d_graph = eng.to_device(graph)
    word, gate = Out(eng, nbr.size, init=nbr), Out(eng, nbr.size, dtype=np.uint8)
    _abi.check(eng.lib.kh_apply_voxel_graph(word.ptr, eng.ptr(d_graph), nbr.size, gate.ptr if with_gate else C.c_void_p(0), eng.stream()))
    eng.sync()
    np.testing.assert_array_equal(word.read(), want)
    np.testing.assert_array_equal(gate.read(), want_gate if with_gate else np.full(nbr.size, BYTE, dtype=np.uint8))


def test_apply_voxel_graph_arguments(eng):
    from kimimaro_amd import _abi
    word, d_graph = Out(eng, 8, init=np.arange(8, dtype=np.uint32)), eng.to_device(np.zeros(8, dtype=np.uint32))
    assert eng.lib.kh_apply_voxel_graph(word.ptr, eng.ptr(d_graph), 0, C.c_void_p(0), eng.stream()) == 0
    for args in ((C.c_void_p(0), eng.ptr(d_graph), 8), (word.ptr, C.c_void_p(0), 8), (word.ptr, eng.ptr(d_graph), -1)):
        assert eng.lib.kh_apply_voxel_graph(args[0], args[1], args[2], C.c_void_p(0), eng.stream()) == EINVAL
        assert "kh_apply_voxel_graph" in _abi.last_error()
    eng.sync()
    np.testing.assert_array_equal(word.read(), np.arange(8, dtype=np.uint32))


LENGTHS = [1, 255, 256, 257, ONE_PASS + 3]


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("n", LENGTHS)
def test_init_alive(eng, n, dtype):
    from kimimaro_amd import _abi
    rng = np.random.default_rng(n)
    nlabels = 200
    flat = rng.integers(0, nlabels + 1, n)
    flat[-1] = nlabels
    slot = np.where(rng.random(nlabels + 1) < 0.5, rng.permutation(nlabels + 1), -1).astype(np.int32)
    slot[0] = 5                                                     # background is never alive, whatever the table says at 0
    slot[nlabels] = 0
    d_lab, d_slot = eng.to_device(flat.astype(dtype)), eng.to_device(slot)
    out = Out(eng, n, dtype=np.uint8)
    _abi.check(eng.lib.kh_init_alive(eng.ptr(d_lab), np.dtype(dtype).itemsize, n, eng.ptr(d_slot), out.ptr, eng.stream()))
    eng.sync()
    np.testing.assert_array_equal(out.read(), prep_ref.alive(flat, slot))


@pytest.mark.parametrize("n", LENGTHS)
def test_fill_and_gather(eng, n):
    from kimimaro_amd import _abi
    rng = np.random.default_rng(n)
    for value in (np.float32(np.inf), np.float32(-1.25), np.float32(1e-42)):
        out = Out(eng, n)
        _abi.check(eng.lib.kh_fill_f32(out.ptr, n, float(value), eng.stream()))
        eng.sync()
        np.testing.assert_array_equal(out.read(), np.full(n, bits(value)[0], dtype=np.uint32))
    for value in (1, 0, 0xA7):
        out = Out(eng, n, dtype=np.uint8)
        _abi.check(eng.lib.kh_fill_u8(out.ptr, n, value, eng.stream()))
        eng.sync()
        np.testing.assert_array_equal(out.read(), np.full(n, value, dtype=np.uint8))
    nsrc = 1000
    src = rng.integers(0, 1 << 32, nsrc, dtype=np.uint64).astype(np.uint32)       # any bit pattern, NaNs included: a gather copies
    for idx in (rng.integers(0, nsrc, n), np.arange(n)[::-1] % nsrc, np.full(n, nsrc - 1)):   # repeated, descending, all the same
        idx = idx.astype(np.uint32)
        d_src, d_idx = eng.to_device(src), eng.to_device(idx)
        out = Out(eng, n)
        _abi.check(eng.lib.kh_gather_f32(eng.ptr(d_src), eng.ptr(d_idx), n, out.ptr, eng.stream()))
        eng.sync()
        np.testing.assert_array_equal(out.read(), src[idx])


# ---- kh_pdrf ------------------------------------------------------------------------------------------------------------------
PDRF_SHAPE = (40, 9, 6)
PDRF_LABELS = [1, 2, 4, 5, 7]       # 7 is a single voxel; 3, 6, 8, 9 have none


@functools.lru_cache(maxsize=None)
def pdrf_volume():
    from kimimaro_amd import _abi
    f = np.float32
    rng = np.random.default_rng(42)
    lab = pattern(PDRF_SHAPE, "voronoi").copy()
    lab[lab == 3] = 4
    lab[17, 4, 3] = 7
    flat = lab.reshape(-1, order="F")
    assert sorted(set(np.unique(flat)) - {0}) == PDRF_LABELS and (flat == 0).any()
    dbf = (rng.random(flat.size) * 7 + 0.5).astype(f)
    daf = (rng.random(flat.size) * 400).astype(f)
    daf[rng.choice(flat.size, 40, replace=False)] = np.inf
    daf[flat == 7] = np.inf
    slot = np.full(10, -1, dtype=np.int32)
    slot[PDRF_LABELS] = [3, 0, 4, 1, 2]
    tasks = np.zeros(len(PDRF_LABELS), dtype=_abi.LABEL_T)
    for label in PDRF_LABELS:
        own = np.flatnonzero(flat == label)
        dbf_max = f(dbf[own].max())
        tasks["segid"][slot[label]] = label
        tasks["M"][slot[label]] = f(1 / (f(dbf_max) ** 1.01))        # kimimaro/trace.py:336, as kimimaro_amd.plan computes it
        finite = daf[own][np.isfinite(daf[own])]
        tasks["max_val"][slot[label]] = finite.max() if finite.size else 0
        if own.size > 30:
            # voxels whose 2^15-th power lies in the subnormal range and survives to the result (DAF 0 or +inf: nothing is added):
            # (1 - x)^32768 ~ exp(-32768 x) is subnormal for x = DBF * M in 0.00267 .. 0.00314
            probe = own[5:17]
            dbf[probe] = (np.linspace(0.0026, 0.0032, probe.size) * float(dbf_max) ** 1.01).astype(f)
            daf[probe[::2]] = 0
            daf[probe[1::2]] = np.inf
    assert tasks["max_val"][slot[7]] == 0 and np.isinf(daf[flat != 0]).sum() > 10
    return flat, dbf, daf, slot, tasks


def pdrf_call(eng, dtype, slot, stage, scale, pdrf_in, daf_in, label_bytes=None):
    flat, dbf, _, _, tasks = pdrf_volume()
    t = eng.torch
    d_lab, d_slot, d_dbf = eng.to_device(flat.astype(dtype)), eng.to_device(slot), eng.to_device(dbf)
    d_tasks = t.from_numpy(tasks.view(np.uint8).copy()).to(eng.device)
    out, daf = Out(eng, flat.size, init=pdrf_in), Out(eng, flat.size, init=daf_in)
    rc = eng.lib.kh_pdrf(eng.ptr(d_lab), label_bytes or np.dtype(dtype).itemsize, flat.size, eng.ptr(d_slot), eng.ptr(d_tasks),
                         eng.ptr(d_dbf), daf.ptr, stage, scale, out.ptr, eng.stream())
    eng.sync()
    return rc, out, daf


def garbage(n, base):
    """n distinct bit patterns that no result holds (NaNs with a payload for base 0x7FC00000)"""
    return (np.uint32(base) + np.arange(n, dtype=np.uint32)).view(np.float32)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("log2e", [0, 2, 4, 15])
def test_pdrf_stages(eng, log2e, dtype):
    from kimimaro_amd import _abi
    flat, dbf, daf, slot, tasks = pdrf_volume()
    scale = 1.0 if log2e == 15 else 100000.0
    before = garbage(flat.size, 0x7FC00000)
    want, want_daf = prep_ref.pdrf(flat, slot, tasks, dbf, daf, log2e, scale)
    if log2e == 15:
        tiny = want[(want != 0) & (np.abs(want) < np.finfo(np.float32).tiny)]
        assert tiny.size >= 8, "the case must carry subnormal results"
    rc, out, d_daf = pdrf_call(eng, dtype, slot, log2e, scale, before, daf)
    _abi.check(rc)
    np.testing.assert_array_equal(out.read(), bits(want))
    np.testing.assert_array_equal(d_daf.read(), bits(want_daf))


def test_pdrf_base_power_finish(eng):
    """an exponent that is no power of two: KH_PDRF_BASE, the host's own np.power on the buffer, KH_PDRF_FINISH"""
    from kimimaro_amd import _abi
    flat, dbf, daf, slot, tasks = pdrf_volume()
    scale = 5000.0
    want_base, same = prep_ref.pdrf(flat, slot, tasks, dbf, daf, prep_ref.PDRF_BASE, scale)
    rc, out, d_daf = pdrf_call(eng, np.uint16, slot, _abi.PDRF_BASE, scale, garbage(flat.size, 0x7FC00000), daf)
    _abi.check(rc)
    base = out.read()
    np.testing.assert_array_equal(base, bits(want_base))
    np.testing.assert_array_equal(d_daf.read(), bits(daf))
    np.testing.assert_array_equal(bits(same), bits(daf))
    cubed = base.view(np.float32).copy()
    with np.errstate(all="ignore"):
        np.power(cubed, 3, out=cubed)
    want, want_daf = prep_ref.pdrf(flat, slot, tasks, dbf, daf, prep_ref.PDRF_FINISH, scale, pdrf_in=cubed)
    rc, out, d_daf = pdrf_call(eng, np.uint16, slot, _abi.PDRF_FINISH, scale, cubed, daf)
    _abi.check(rc)
    np.testing.assert_array_equal(out.read(), bits(want))
    np.testing.assert_array_equal(d_daf.read(), bits(want_daf))


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_pdrf_keep_others(eng, dtype):
    """two of the five labels selected: with KH_PDRF_KEEP_OTHERS every other voxel of both volumes keeps its bits; without it the
    other voxels become +inf in pdrf and keep their bits in daf"""
    from kimimaro_amd import _abi
    flat, dbf, daf, slot, tasks = pdrf_volume()
    part = slot.copy()
    part[[1, 5, 7]] = -1
    mine = np.isin(flat, [2, 4])
    pdrf_before = garbage(flat.size, 0x7FC00000)
    daf_before = np.where(mine, daf, garbage(flat.size, 0x12340000))
    for keep in (True, False):
        want, want_daf = prep_ref.pdrf(flat, part, tasks, dbf, daf_before, 2, 100000.0, keep=keep, pdrf_in=pdrf_before)
        np.testing.assert_array_equal(bits(want_daf[~mine]), bits(daf_before[~mine]))
        if keep:
            np.testing.assert_array_equal(bits(want[~mine]), bits(pdrf_before[~mine]))
        else:
            assert np.isposinf(want[~mine]).all()
        rc, out, d_daf = pdrf_call(eng, dtype, part, 2 | (_abi.PDRF_KEEP_OTHERS if keep else 0), 100000.0, pdrf_before, daf_before)
        _abi.check(rc)
        np.testing.assert_array_equal(out.read(), bits(want))
        np.testing.assert_array_equal(d_daf.read(), bits(want_daf))


def test_pdrf_bad_exponents(eng):
    """16, -3, and KH_PDRF_KEEP_OTHERS on a stage that is not 0..15.  In two's complement `KH_PDRF_BASE | KH_PDRF_KEEP_OTHERS` IS
    KH_PDRF_BASE (bit 8 of -1 and of -2 is set already), so no call can tell that combination from the plain stage; what can be
    told apart is refused: the flag on -3, on 16, and a negative stage with the flag's bit taken OUT (-1 ^ 0x100)."""
    from kimimaro_amd import _abi
    flat, dbf, daf, slot, tasks = pdrf_volume()
    keep = _abi.PDRF_KEEP_OTHERS
    assert (_abi.PDRF_BASE | keep, _abi.PDRF_FINISH | keep) == (_abi.PDRF_BASE, _abi.PDRF_FINISH)
    before = garbage(flat.size, 0x7FC00000)
    for stage in (16, -3, -3 | keep, 16 | keep, _abi.PDRF_BASE ^ keep, _abi.PDRF_FINISH ^ keep, 0x200, keep << 1 | 2):
        rc, out, d_daf = pdrf_call(eng, np.uint32, slot, stage, 1.0, before, daf)
        assert rc == EINVAL, stage
        assert "kh_pdrf" in _abi.last_error()
        np.testing.assert_array_equal(out.read(), bits(before))    # and nothing ran
        np.testing.assert_array_equal(d_daf.read(), bits(daf))


def test_eight_byte_labels_are_refused(eng):
    """KH_DISPATCH_LT: label_bytes 1, 2 or 4"""
    from kimimaro_amd import _abi
    flat, dbf, daf, slot, tasks = pdrf_volume()
    lab8 = eng.to_device(flat.astype(np.uint64))
    d_slot = eng.to_device(slot)
    n = flat.size

    def refused(rc):
        eng.sync()
        assert rc == EINVAL
        assert "label_bytes" in _abi.last_error()

    rc, outs = stats_call(eng, flat, np.uint64, dbf, PDRF_SHAPE, 9, label_bytes=8)
    refused(rc)
    assert all((o.read() != WORD).all() for o in outs)              # the outputs were initialised, their guards hold
    cursors, lists, d_off = Out(eng, 5), Out(eng, n), eng.to_device(np.zeros(5, dtype=np.uint32))
    refused(eng.lib.kh_scatter_lists(eng.ptr(lab8), 8, n, eng.ptr(d_slot), 5, eng.ptr(d_off), cursors.ptr, lists.ptr, eng.stream()))
    assert (lists.read() == WORD).all()
    nbr = Out(eng, n)
    refused(eng.lib.kh_neighbor_mask(eng.ptr(lab8), 8, PDRF_SHAPE[0], PDRF_SHAPE[1], PDRF_SHAPE[2], nbr.ptr, eng.stream()))
    assert (nbr.read() == WORD).all()
    rc, out, d_daf = pdrf_call(eng, np.uint64, slot, 2, 1.0, garbage(n, 0x7FC00000), daf, label_bytes=8)
    refused(rc)
    np.testing.assert_array_equal(d_daf.read(), bits(daf))
    alive = Out(eng, n, dtype=np.uint8)
    refused(eng.lib.kh_init_alive(eng.ptr(lab8), 8, n, eng.ptr(d_slot), alive.ptr, eng.stream()))
    assert (alive.read() == BYTE).all()


# ---- kh_level_keys ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [(16, 16, 40), (1, 1, 1), (3.7, 1.3, 2.2)], ids=str)
@pytest.mark.parametrize("dims", [(1, 1, 1), (45, 45, 19), (257, 3, 2)], ids=str)
def test_level_keys(eng, dims, w):
    """bit-equal to the statement the host tier trusts (tests/test_host.py builds its key table from the same function); with the
    non-integer weights a fused multiply-add or a square root that is not correctly rounded changes bits"""
    from kimimaro_amd import _abi
    n = dims[0] * dims[1] * dims[2]
    wf = [float(np.float32(v)) for v in w]
    out = Out(eng, n)
    _abi.check(eng.lib.kh_level_keys(dims[0], dims[1], dims[2], wf[0], wf[1], wf[2], out.ptr, eng.stream()))
    eng.sync()
    np.testing.assert_array_equal(out.read(), bits(prep_ref.level_keys(dims, w).reshape(-1, order="F")))


def test_level_keys_bad_sizes(eng):
    from kimimaro_amd import _abi
    out = Out(eng, 8)
    for dims in ((0, 2, 2), (2, -1, 2), (2, 2, 0), (1 << 16, 1 << 15, 1), (1 << 11, 1 << 10, 1 << 10), (1 << 20, 1 << 20, 1)):
        assert eng.lib.kh_level_keys(dims[0], dims[1], dims[2], 1.0, 1.0, 1.0, out.ptr, eng.stream()) == EINVAL, dims
        assert "kh_level_keys" in _abi.last_error()
    eng.sync()
    assert (out.read() == WORD).all()
