"""fill_all_holes in one pass over the volume on the MI355X: kimimaro_amd.intake.fill_all_holes against the
restated loop of the reference (tests/fill_ref.py), volume and count exactly; on component volumes also against the per-label loop
intake.fill_all_holes_device, which skeletonize(fill_holes=True) runs."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fill_ref  # noqa: E402
from shapes import voronoi_labels  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from kimimaro_amd.engine import Engine
    return Engine()


def _product(cc):
    """the public function on a copy -> (volume, count)"""
    from kimimaro_amd import intake
    mine = cc.copy(order="K")
    out, n = intake.fill_all_holes(mine, return_fill_count=True)
    assert out is mine
    return out, n


def _both_routes(eng, cc):
    """the components of `cc` (kh_ccl26) filled by the loop and by the new route, each on its own copy -> the host volume filled by
    the reference restatement, which both must equal"""
    from kimimaro_amd import intake
    shape = tuple(cc.shape)
    d_cc, ncomp, _ = eng.ccl(np.asfortranarray(cc))
    host = eng.to_host_volume(d_cc, shape).copy()
    want, want_n, _ = fill_ref.sequential(host)
    d_old, d_new = d_cc.clone(), d_cc.clone()
    n_new = eng.fill_all_holes(d_new, 4, shape)
    assert n_new == want_n
    assert np.array_equal(eng.to_host_volume(d_new, shape), want)
    if ncomp:                                             # (the loop has nothing to go through in an all-zero volume)
        n_old = intake.fill_all_holes_device(eng, d_old, shape, ncomp)
        assert n_old == want_n
        assert np.array_equal(eng.to_host_volume(d_old, shape), want)
    return want_n


def _check(eng, cc, components=True):
    """product == reference on `cc` as it is; with components=True also loop == new route == reference on cc's components.
    -> (reference volume, count, states)"""
    want, want_n, state = fill_ref.sequential(cc)
    got, n = _product(cc)
    assert got.dtype == cc.dtype and got.shape == cc.shape
    assert np.array_equal(got, want)
    assert n == want_n
    if components and cc.ndim == 3:
        _both_routes(eng, cc)
    return want, want_n, state


def _box_wall(cc, lo, hi, label):
    """the one-voxel wall of the box [lo, hi] (inclusive corners)"""
    sl = tuple(slice(a, b + 1) for a, b in zip(lo, hi))
    inner = tuple(slice(a + 1, b) for a, b in zip(lo, hi))
    keep = cc[inner].copy()
    cc[sl] = label
    cc[inner] = keep


def _nested(outer, inner):
    cc = np.zeros((12, 12, 12), dtype=np.uint32)
    _box_wall(cc, (1, 1, 1), (10, 10, 10), outer)         # outer shell, interior 8^3 = 512
    _box_wall(cc, (3, 3, 3), (8, 8, 8), inner)            # inner shell (6^3 - 4^3 = 152 voxels), interior 4^3 = 64 background:
    return cc                                             # the pocket; between the shells 512 - 216 = 296 background voxels


def test_nested_shells_in_both_id_orders(eng):
    _, n_out_first, state = _check(eng, _nested(1, 2))
    assert n_out_first == 512 and state == {1: fill_ref.PROCESSED | fill_ref.FILLED, 2: fill_ref.KILLED}
    _, n_in_first, state = _check(eng, _nested(2, 1))
    assert n_in_first == 64 + 512                         # the pocket is filled by the inner label, then again by the outer one
    assert state[1] == fill_ref.PROCESSED | fill_ref.FILLED | fill_ref.KILLED and state[2] == fill_ref.PROCESSED | fill_ref.FILLED


def test_shell_gaps(eng):
    cc = np.zeros((12, 11, 10), dtype=np.uint32)
    _box_wall(cc, (2, 2, 2), (8, 8, 8), 3)
    gap = cc.copy()
    gap[8, 5, 5] = 0                                      # one voxel of a face is missing: the inside is open
    _, n, _ = _check(eng, gap)
    assert n == 0
    edge = cc.copy()
    edge[8, 8, 5] = 0                                     # one voxel of an EDGE is missing: only a diagonal step leads inside
    want, n, _ = _check(eng, edge)
    assert n == 125 and want[8, 8, 5] == 0


@pytest.mark.parametrize("shell_id,thread_id", [(1, 2), (2, 1)])
def test_thread_crossing_a_shell_diagonally(eng, shell_id, thread_id):
    cc = np.zeros((16, 16, 12), dtype=np.uint32)
    _box_wall(cc, (2, 2, 2), (8, 8, 8), shell_id)
    for k in range(5, 11):
        cc[k, k, 5] = thread_id                           # (8, 8, 5) replaces a voxel of the shell's edge: no 6-connected way in
    cc[10:13, 10:13, 4:7] = thread_id                     # the thread ends in a block ...
    cc[11, 11, 5] = 0                                     # ... with a hole of its own
    want, n, state = _check(eng, cc)
    assert want[5, 5, 5] == shell_id and want[7, 7, 5] == shell_id            # the part inside is painted over
    assert want[8, 8, 5] == thread_id and want[9, 9, 5] == thread_id          # the part outside keeps its id
    if shell_id < thread_id:
        assert state[thread_id] == fill_ref.KILLED and want[11, 11, 5] == 0 and n == 125    # killed whole: its own hole stays open
    else:
        assert want[11, 11, 5] == thread_id and n == 1 + 125


def test_face_contacts(eng):
    cc = np.zeros((12, 12, 12), dtype=np.uint32)
    _box_wall(cc, (0, 3, 3), (6, 9, 9), 4)
    cc[0, 4:9, 4:9] = 0                                   # the box has no wall at x = 0: its inside touches the volume's face
    _, n, _ = _check(eng, cc)
    assert n == 0
    cut = np.zeros((14, 14, 14), dtype=np.uint32)
    cut[fill_ref.shell(cut.shape, (1.0, 7.0, 7.0), 5.0, 1.5)] = 6         # a sphere shell cut by the face x = 0
    _, n, _ = _check(eng, cut)
    assert n == 0
    closed = np.zeros((14, 14, 14), dtype=np.uint32)
    _box_wall(closed, (0, 3, 3), (6, 9, 9), 4)            # the same box with its wall ON the face: closed
    _, n, _ = _check(eng, closed)
    assert n == 125


def test_concentric_unconnected_labels(eng):
    cc = np.zeros((17, 17, 17), dtype=np.uint32)
    for k, label in enumerate((1, 2, 1, 2)):              # L1, L2, L1, L2 from the outside in, the innermost a solid block
        _box_wall(cc, (1 + 2 * k,) * 3, (15 - 2 * k,) * 3, label)
    cc[8, 8, 8] = 2
    _, n, _ = _check(eng, cc)
    assert n > 0


def test_long_rows_and_a_hole_across_the_tile_boundary(eng):
    cc = np.zeros((300, 5, 4), dtype=np.uint32)
    cc[250:263, 1:4, 0:3] = 9
    cc[251:262, 2, 1] = 0                                 # a tube of background along x, from 251 to 261: across x = 255 | 256
    want, n, _ = _check(eng, cc)
    assert n == 11 and (want[251:262, 2, 1] == 9).all()


@pytest.mark.parametrize("shape", [(12, 10, 1), (12, 1, 10), (1, 1, 1), (7, 1, 1), (1, 9, 1)])
def test_extent_one_axes(eng, shape):
    """an axis of extent 1 puts every voxel on a face: nothing is ever filled (and nothing goes wrong)"""
    rng = np.random.default_rng(sum(shape))
    cc = rng.integers(0, 4, shape).astype(np.uint32)
    if shape[0] > 1 and max(shape[1:]) > 1:
        ring = [slice(2, 7) if s > 1 else slice(None) for s in shape]
        hole = [slice(3, 6) if s > 1 else slice(None) for s in shape]
        cc[tuple(ring)] = 5
        cc[tuple(hole)] = 0                               # a ring with a hole in the plane
    _, n, _ = _check(eng, cc)
    assert n == 0


def test_all_zero_and_one_label(eng):
    _, n, _ = _check(eng, np.zeros((9, 8, 7), dtype=np.uint32), components=False)
    assert n == 0
    _, n, state = _check(eng, np.full((9, 8, 7), 3, dtype=np.uint32))
    assert n == 0 and state == {3: fill_ref.PROCESSED}


def _random_case(seed):
    cc = voronoi_labels((48, 48, 48), 40, seed).astype(np.uint32)
    rng = np.random.default_rng(1000 + seed)
    for k in range(10):
        centre = [float(rng.integers(4, 44)) for _ in range(3)]
        radius = float(rng.integers(3, 9))
        cc[fill_ref.shell(cc.shape, centre, radius, float(rng.integers(1, 3)), cube=rng.random() < 0.5)] = 41 + k
        if k % 3 == 0:                                    # something of another label inside, to be swallowed
            cc[fill_ref.shell(cc.shape, centre, 1.0, 2.0)] = 60 + k
    noise = rng.random(cc.shape)
    cc[noise < 0.002] = 0
    cc[noise > 0.998] = 77
    return cc


@pytest.mark.parametrize("seed", range(5))
def test_random_volumes(eng, seed):
    _, n, _ = _check(eng, _random_case(seed))
    assert n > 0                                          # (a condition on the input, asserted on the reference's count)


def test_random_volumes_swallow_a_label():
    """a condition on the inputs of test_random_volumes, on the reference alone"""
    assert any(any(bits & fill_ref.KILLED for bits in fill_ref.sequential(_random_case(seed))[2].values()) for seed in range(5))


def test_pair_table_overflow_is_retried(eng):
    """a pair table that is too small is reported and tried again larger; the result is the same"""
    cc = np.asfortranarray(_random_case(0))
    want, want_n, _ = fill_ref.sequential(cc)
    d = eng.to_device(cc)
    stats = {}
    eng.holes_table_capacity = 64
    try:
        n = eng.fill_all_holes(d, 4, cc.shape, stats=stats)
    finally:
        eng.holes_table_capacity = None
    assert stats["table_tries"] > 1 and stats["pairs"] > 64 and stats["table_capacity"] >= stats["pairs"]
    assert n == want_n and np.array_equal(eng.to_host_volume(d, cc.shape), want)
    for key in ("regions_ms", "table_ms", "pairs_ms", "apply_ms", "resolve_ms"):
        assert stats[key] >= 0


def assert_region_graph(eng, cc, ndim=3):
    """the device's regions, table and pairs of `cc` (three axes; ndim < 3: the trailing ones have extent 1 and are no axes) equal
    numpy's up to the numbering of the regions; the device numbers them by first appearance in the raster"""
    value, count, face, pairs, region = fill_ref.region_graph(cc.reshape(cc.shape[:ndim]))
    region = region.reshape(cc.shape)
    d_region, g_value, g_count, g_face, g_pairs, info = eng.region_graph(eng.to_device(cc), cc.dtype.itemsize, cc.shape, ndim)
    got = eng.to_host_volume(d_region, cc.shape).astype(np.int64)
    nreg = len(value) - 1
    assert info["regions"] == nreg and got.min() == 1 and got.max() == nreg
    flat = got.reshape(-1, order="F")
    firsts = np.unique(flat, return_index=True)[1]
    assert (np.diff(firsts) > 0).all()                    # ids ascend with the first voxel of the region in the raster
    to_ref = np.zeros(nreg + 1, dtype=np.int64)
    to_ref[got.reshape(-1)] = region.reshape(-1)
    assert np.array_equal(to_ref[got], region) and len(np.unique(to_ref[1:])) == nreg      # the same partition
    assert np.array_equal(g_value[1:], value[to_ref[1:]])
    assert np.array_equal(g_count[1:], count[to_ref[1:]])
    assert np.array_equal(g_face[1:], face[to_ref[1:]])
    lo, hi = to_ref[(g_pairs >> np.uint64(32)).astype(np.int64)], to_ref[(g_pairs & np.uint64(0xFFFFFFFF)).astype(np.int64)]
    mapped = (np.minimum(lo, hi).astype(np.uint64) << np.uint64(32)) | np.maximum(lo, hi).astype(np.uint64)
    assert len(np.unique(g_pairs)) == len(g_pairs)
    assert np.array_equal(np.sort(mapped), pairs)
    return nreg


@pytest.mark.parametrize("shape,dtype", [((70, 33, 21), np.uint16), ((130, 9, 5), np.uint64), ((5, 6, 7), np.uint8)])
def test_region_graph_against_numpy(eng, shape, dtype):
    rng = np.random.default_rng(shape[0])
    cc = np.asfortranarray(rng.integers(0, 3, shape).astype(dtype) * dtype(41))
    cc[2:-1, 2:-1, 2:-1] = np.where(rng.random(cc[2:-1, 2:-1, 2:-1].shape) < 0.6, dtype(7), cc[2:-1, 2:-1, 2:-1])
    assert_region_graph(eng, cc)


@pytest.mark.parametrize("dtype,scale", [(np.uint8, 1), (np.uint16, 1000), (np.uint32, 1), (np.uint32, (1 << 31) + 5), (np.uint64, (1 << 40) + 3),
                                         (np.int32, 3), (np.bool_, 1)])
def test_label_dtypes_and_sparse_values(eng, dtype, scale):
    base = _nested(2, 1)
    base[0, 0, 0] = 3
    if dtype == np.bool_:
        cc = base == 2
    elif scale == 1000:
        cc = (base * 1000 + (base > 0) * 5).astype(dtype)
    elif scale > 1000:
        cc = (base.astype(np.uint64) + np.uint64(scale) * (base > 0)).astype(dtype)       # 2^31 + 6, 2^31 + 7, 2^31 + 8
    else:
        cc = (base * scale).astype(dtype)
    _, n, _ = _check(eng, cc, components=False)
    assert n > 0


def test_memory_orders_axes_and_return_forms(eng):
    from kimimaro_amd import intake
    base = np.zeros((12, 11, 10), dtype=np.uint32)
    _box_wall(base, (1, 1, 1), (10, 9, 8), 1)
    _box_wall(base, (3, 3, 3), (7, 6, 5), 2)
    want, want_n, _ = fill_ref.sequential(base)
    assert want_n > 0
    for order in ("C", "F"):
        cc = np.array(base, order=order)
        out = intake.fill_all_holes(cc)                   # without the count: the array alone
        assert out is cc and np.array_equal(cc, want)
        cc = np.array(base, order=order)
        out, n = intake.fill_all_holes(cc, progress=True, return_fill_count=True)
        assert out is cc and n == want_n and np.array_equal(cc, want)
    view = np.zeros((14, 13, 12), dtype=np.uint32)[1:13, 1:12, 1:11]       # not contiguous at all
    view[...] = base
    assert intake.fill_all_holes(view) is view and np.array_equal(view, want)
    plane = np.zeros((12, 10), dtype=np.uint16)           # a 2-D array: its border is its outline
    plane[2:9, 2:8] = 5
    plane[4:6, 3:6] = 0
    want2, n2, _ = fill_ref.sequential(plane)
    out, n = intake.fill_all_holes(plane.copy(), return_fill_count=True)
    assert n2 == 6 and n == n2 and np.array_equal(out, want2)
    line, n = intake.fill_all_holes(np.array([1, 0, 1, 2, 0], dtype=np.uint8), return_fill_count=True)
    assert n == 1 and line.tolist() == [1, 1, 1, 2, 0]    # 1-D: a gap between two voxels of a label is a hole
    four = base.reshape(base.shape + (1,)).copy()
    assert np.array_equal(intake.fill_all_holes(four)[..., 0], want)
    empty = np.zeros((0, 4, 4), dtype=np.uint32)
    assert intake.fill_all_holes(empty, return_fill_count=True)[1] == 0
    with pytest.raises(TypeError):
        intake.fill_all_holes(base.astype(np.float32))


def test_tensor_in_tensor_out(eng):
    import torch
    from kimimaro_amd import intake
    base = _nested(2, 1)
    want, want_n, _ = fill_ref.sequential(base)
    for dtype in (torch.int32, torch.int64, torch.uint8, torch.int16):
        ten = torch.from_numpy(base.astype(np.int64)).to(dtype).to(eng.device)            # indexed [x, y, z], C order: copied inside
        out, n = intake.fill_all_holes(ten, return_fill_count=True)
        assert out is ten and n == want_n
        assert np.array_equal(ten.cpu().numpy().astype(np.uint32), want)
    zyx = torch.from_numpy(np.ascontiguousarray(base.astype(np.int32).transpose(2, 1, 0))).to(eng.device)
    ten = zyx.permute(2, 1, 0)                            # a Fortran-ordered view: edited where it lies
    assert intake.fill_all_holes(ten) is ten
    assert np.array_equal(zyx.cpu().numpy().transpose(2, 1, 0).astype(np.uint32), want)
    mask = torch.from_numpy(base == 2).to(eng.device)
    want_mask, n_mask, _ = fill_ref.sequential(base == 2)
    out, n = intake.fill_all_holes(mask, return_fill_count=True)
    assert out is mask and out.dtype == torch.bool and n == n_mask and np.array_equal(mask.cpu().numpy(), want_mask)


def test_both_routes_on_a_96_cubed_volume(eng):
    """skeletonize(fill_holes=True): the component volume after the new route equals the one after the per-label loop"""
    cc = voronoi_labels((96, 96, 96), 60, 7).astype(np.uint32)
    rng = np.random.default_rng(7)
    for k in range(12):
        centre = [float(rng.integers(8, 88)) for _ in range(3)]
        cc[fill_ref.shell(cc.shape, centre, float(rng.integers(4, 12)), 2.0, cube=k % 2 == 0)] = 100 + k
        cc[fill_ref.shell(cc.shape, centre, 2.0, 3.0)] = 0 if k % 3 else 200 + k
    assert _both_routes(eng, cc) > 0
