"""kimimaro_amd.boxes on numbers, without a GPU: the plumbing the dataset-in-boxes drivers share, each piece against plain numpy.  The
grid arithmetic the drivers take from kimimaro_amd.plan (core_index, neighbor_cores) is checked here beside it."""
import numpy as np
import pytest

from kimimaro_amd import boxes, plan
from kimimaro_amd.segment_boxes import DIRECTIONS


class SlicesOnly:
    """a dataset in the h5py / zarr form: .shape and __getitem__ over a tuple of slices, nothing else"""

    def __init__(self, array, cut=None):
        self.array, self.shape, self.cut = array, array.shape, cut

    def __getitem__(self, at):
        assert isinstance(at, tuple) and len(at) == len(self.shape) and all(isinstance(s, slice) for s in at), at
        return self.array[at] if self.cut is None else self.array[at][self.cut]


VOLUME = np.arange(6 * 5 * 4, dtype=np.uint16).reshape(6, 5, 4)


@pytest.mark.parametrize("dataset", [VOLUME, np.asfortranarray(VOLUME), SlicesOnly(VOLUME)], ids=["c", "fortran", "slices_only"])
def test_load_box_is_plain_indexing(dataset):
    for lo, hi in (((0, 0, 0), (6, 5, 4)), ((1, 2, 0), (4, 5, 3)), (np.array([5, 4, 3]), np.array([6, 5, 4]))):
        got = boxes._load_box(dataset, lo, hi, "driver")
        assert isinstance(got, np.ndarray) and got.dtype == VOLUME.dtype
        assert np.array_equal(got, VOLUME[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]])


def test_load_box_gives_two_axes_a_unit_z_axis():
    flat = VOLUME[:, :, 0]
    got = boxes._load_box(flat, (1, 0, 0), (5, 3, 1), "driver")
    assert got.shape == (4, 3, 1) and np.array_equal(got[:, :, 0], flat[1:5, 0:3])


def test_load_box_checks_the_shape_when_it_has_a_name():
    short = SlicesOnly(VOLUME, cut=(slice(0, 2),))
    assert boxes._load_box(short, (1, 0, 0), (5, 3, 2)).shape == (2, 3, 2)               # unnamed: the cut as it comes
    with pytest.raises(ValueError, match=r"driver: dataset\[\[1, 0, 0\]:\[5, 3, 2\]\] has shape \(2, 3, 2\)"):
        boxes._load_box(short, np.array([1, 0, 0]), np.array([5, 3, 2]), "driver")


def test_store_like():
    given = np.zeros((6, 5, 4), dtype=np.float32)
    assert boxes.store_like(given, (6, 5, 4), np.float32, "distance_store") is given
    with pytest.raises(ValueError, match="distance_store: float32 of shape"):
        boxes.store_like(np.zeros((6, 5), dtype=np.float32), (6, 5, 4), np.float32, "distance_store")
    with pytest.raises(ValueError, match="region_store: u32 of shape"):
        boxes.store_like(np.zeros((6, 5, 4), dtype=np.int32), (6, 5, 4), np.uint32, "region_store", "u32")
    made = boxes.store_like(None, (6, 5, 4), np.uint32, "feature_store")
    assert made.shape == (6, 5, 4) and made.dtype == np.uint32 and made.flags.f_contiguous
    zeroed = boxes.store_like(None, (6, 5, 4), np.uint32, "region_store", "u32", zeros=True)
    assert zeroed.flags.f_contiguous and not zeroed.any()


def test_group_by_core():
    grid = plan.chunk_grid((8, 6, 3), (4, 3, 3), overlap=0)
    assert grid.grid == (2, 2, 1)
    cores = np.array([3, 0, 3, 1, 0, 3, 1, 0, 0, 3, 1, 3], dtype=np.int64)               # core 2 holds nothing; given out of order
    items = np.arange(100, 112, dtype=np.int64)
    want = {}
    for core, item in zip(cores.tolist(), items.tolist()):
        want.setdefault(core, []).append(item)
    got = boxes.group_by_core(cores, items)
    assert list(got) == sorted(want) == [0, 1, 3]
    assert {k: v.tolist() for k, v in got.items()} == want
    assert boxes.group_by_core(cores[:0], items[:0]) == {}


def test_core_index_and_neighbor_cores():
    shape, chunk = (9, 7, 5), (3, 4, 3)
    grid = plan.chunk_grid(shape, chunk, overlap=0)
    assert grid.grid == (3, 2, 2)
    assert np.array_equal(plan.core_index(grid.grid, grid.grid_index), np.arange(12))     # position -> index -> position
    near = plan.neighbor_cores(grid, DIRECTIONS)
    assert near.shape == (12, 26)
    for k in range(12):
        for bit, step in enumerate(DIRECTIONS):
            step = np.array(step)
            # the core's voxel nearest that face, edge or corner, stepped across it
            voxel = np.where(step < 0, grid.core_lo[k], np.where(step > 0, grid.core_hi[k] - 1, grid.core_lo[k])) + step
            assert near[k, bit] == plan.core_of([voxel], shape, chunk)[0]
            outside = np.any((grid.grid_index[k] + step < 0) | (grid.grid_index[k] + step >= grid.grid))
            assert (near[k, bit] == -1) == outside


def test_count_core():
    rng = np.random.default_rng(3)
    volume = rng.choice(np.array([0, 4, 9, 17], dtype=np.uint32), size=(6, 5, 4))
    place = {4: 1, 17: 0, 23: 2}                                                          # 9 is no skeleton's label, 23 no voxel's
    counts = np.array([10, 20, 30], dtype=np.int64)
    boxes.count_core(volume, place, counts)
    found = dict(zip(*(a.tolist() for a in np.unique(volume, return_counts=True))))
    assert counts.tolist() == [10 + found[17], 20 + found[4], 30]
