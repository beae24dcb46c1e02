"""What the host tests of cross_sectional_area_filled_chunked put in place of the GPU, on the statements of
tests/fill_ref.py, tests/section_filled_ref.py and tests/section_box_ref.py: numpy and scipy only, independent of the product.

  regions_on_host   Engine.region_graph's contract on a host array: fill_ref.region_graph on the core, the face flag taken on the
                    faces of the core that the mask names (kh_region_table_box's meaning).
  FakeFilledSections  section.cross_sections_filled_box's signature: the section of the CROPPED box of the mask "carries the label,
                    or its id in the region box is listed", contact and clip read off the voxel list.
Also the datasets the tests share."""
import numpy as np

import fill_ref
import section_box_ref as B
import section_ref

SHAPE, CORES = (24, 20, 18), (10, 8, 7)          # cuts at x = 10, 20, y = 8, 16, z = 7, 14: cores of unequal size


def regions_on_host(core, label_bytes, shape, ndim, mark, faces):
    core = np.asarray(core)
    assert core.shape == tuple(shape) and core.dtype.itemsize == label_bytes and ndim == 3
    value, count, _, pairs, region = fill_ref.region_graph(core)
    face = np.zeros(value.size, dtype=np.uint8)
    for axis in range(3):
        for bit, index in ((1 << (2 * axis), 0), (2 << (2 * axis), -1)):
            if faces & bit:
                face[np.unique(np.take(region, index, axis=axis))] = 1
    return region, value, count, face, pairs, {}


class FakeFilledSections:
    """`calls` records (box_lo, box_shape, the seeds in dataset coordinates, the list handed over, hole_begin, hole_count) per launch"""

    def __init__(self):
        self.calls = []

    def __call__(self, eng, d_lab, label_bytes, box_lo, box_shape, dataset_shape, anisotropy, seed_lin, want_label, normals, filled,
                 stats=None):
        regions, begin, count, ids = filled
        ext = tuple(int(v) for v in box_shape)
        assert eng is None and tuple(d_lab.shape) == ext and d_lab.dtype.itemsize == label_bytes
        assert tuple(regions.shape) == ext and regions.dtype == np.uint32 and np.all(regions != 0)
        lo = np.array([int(v) for v in box_lo], dtype=np.int64)
        n = len(seed_lin)
        area, contact, clip = np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
        voxels = np.zeros(n, dtype=np.uint32)
        seeds, masks = [], {}
        for i in range(n):
            lin = int(seed_lin[i])
            if lin == B.OUTSIDE:
                seeds.append(None)
                continue
            seed = (lin % ext[0], (lin // ext[0]) % ext[1], lin // (ext[0] * ext[1]))
            seeds.append(tuple(int(v) for v in lo + seed))
            key = (int(want_label[i]), int(begin[i]), int(count[i]))
            if key not in masks:
                mine = ids[key[1]:key[1] + key[2]]
                assert np.all(np.diff(mine.astype(np.int64)) > 0)                      # ascending
                masks[key] = (np.asarray(d_lab) == key[0]) | np.isin(regions, mine)
            vox, a, _ = section_ref.section(masks[key], seed, normals[i], anisotropy, True)
            if len(vox):
                contact[i], clip[i] = B.face_bits(vox, lo, ext, dataset_shape)
                area[i], voxels[i] = np.float32(a), len(vox)
        self.calls.append((tuple(lo.tolist()), ext, seeds, np.array(ids, copy=True), np.array(begin, copy=True), np.array(count, copy=True)))
        return area, contact, clip, voxels


def box_walls(shape, lo, hi):
    """a mask: the walls, one voxel thick, of the box [lo, hi] (both ends included)"""
    walls = np.zeros(shape, dtype=bool)
    inside = tuple(slice(a, b + 1) for a, b in zip(lo, hi))
    walls[inside] = True
    walls[tuple(slice(a + 1, b) for a, b in zip(lo, hi))] = False
    return walls


def random_dataset(seed):
    """fill_ref.random_volume, repeated and cut to SHAPE (the repeats make every label disconnected)"""
    v = fill_ref.random_volume(seed)
    reps = [-(-s // n) for s, n in zip(SHAPE, v.shape)]
    return np.asfortranarray(np.tile(v, reps)[:SHAPE[0], :SHAPE[1], :SHAPE[2]])


def straddling_shells():
    """{name: dataset}: a shell of label 5 whose cavity lies across the cut x = 10, y = 8, z = 7, and the corner where eight cores meet"""
    out = {}
    for name, lo, hi in (("x", (7, 1, 1), (13, 6, 5)), ("y", (2, 5, 1), (8, 11, 5)), ("z", (2, 1, 4), (8, 6, 10)),
                         ("corner", (7, 5, 4), (13, 11, 10))):
        lab = np.zeros(SHAPE, dtype=np.uint16, order="F")
        lab[box_walls(SHAPE, lo, hi)] = 5
        out[name] = lab
    return out


def nested_shells():
    """shell 3 around shell 4 around a core of label 6, across the cut x = 10 (and y = 8)"""
    lab = np.zeros(SHAPE, dtype=np.uint16, order="F")
    lab[box_walls(SHAPE, (4, 3, 1), (16, 13, 6))] = 3
    lab[box_walls(SHAPE, (6, 5, 2), (14, 11, 5))] = 4
    lab[9:12, 7:9, 3:5] = 6
    return lab


def open_tube():
    """label 7: a square tube along x, capped at x = 2 and open at the face x = 23 of the dataset.  Inside the first core (x < 10)
    its bore touches no face of the dataset: closed in that core's view, open in the dataset"""
    lab = np.zeros(SHAPE, dtype=np.uint16, order="F")
    lab[2:, 2:7, 1:6] = 7
    lab[3:, 3:6, 2:5] = 0
    return lab


def room():
    """(labels, skeletons): label 5 is the wall of a room [1, 22] x [1, 18] x [1, 16] that fills the dataset but for a margin; the box
    of the middle core at halo 1 lies inside the room and holds no voxel of 5.  Label 9 is a blob in the room.  Skeleton 5 runs
    from the wall at x = 1 through the room; skeleton 9 sits in its blob; 77 names no voxel."""
    from kimimaro_amd import Skeleton
    lab = np.zeros(SHAPE, dtype=np.uint16, order="F")
    lab[box_walls(SHAPE, (1, 1, 1), (22, 18, 16))] = 5
    lab[13:16, 10:13, 9:12] = 9
    line = np.array([[x, 11, 10] for x in range(1, 20)])
    edges = np.array([[i, i + 1] for i in range(len(line) - 1)])
    skels = {5: Skeleton(line, edges, segid=5, space="voxel"),
             9: Skeleton(np.array([[13, 11, 10], [14, 11, 10], [15, 11, 10]]), np.array([[0, 1], [1, 2]]), segid=9, space="voxel"),
             77: Skeleton(np.array([[3, 3, 3], [4, 3, 3]]), np.array([[0, 1]]), segid=77, space="voxel")}
    return lab, skels
