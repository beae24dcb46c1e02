"""What the dataset-in-boxes drivers share (region_boxes, section_boxes, segment_boxes, point_boxes; post.skeletonize_chunked
composes them): a dataset that is never resident as a whole is read box by box, and every driver needs the same plumbing around
that.  Each piece has its one owner here:

    axes, label_type                   what a driver knows about its dataset: shape as given, with three axes, extent; dtype, span
    _slices, _load_box                 a box of a dataset or a store as a host array, optionally checked against the shape asked for
    _store_box                         its writing counterpart: a host box into a dataset or a store
    store_like                         a store of the dataset's shape and one dtype: the caller's, checked, or a Fortran numpy array
    clip_graph, GRAPH_STEP_OF_BIT      a box of a voxel connectivity graph without the bits that leave it; the word's layout
    label_table                        the skeletons' labels, their sorted table and each label's place in it
    upload_labels                      a host box of labels -> the device labels the kernels read, and the word of every table entry
    count_core, count_core_device      voxels per label of the table in a core, on the host and on the device
    group_by_core                      items grouped by the core they fall into
    up, down                           Fortran host box of 32-bit words <-> flat device tensor; the core of a device box -> host
    route_targets, count_labels        on a plan.chunk_grid: the extra targets of every box; voxels per label over the cores

The grid arithmetic (which core holds a voxel, a core's neighbours) is plan's: core_of, core_index, neighbor_cores.  Nothing here
decides an order of checks or names a driver: the drivers call these in their own order and pass their name where a message has one.
"""
from collections import defaultdict

import numpy as np

from . import utility
from .volume import DimensionError, _device_labels


def axes(dataset, name):
    """-> (the dataset's shape as given, its shape with three axes -- two axes get a unit z axis --, that as an int64 array);
    DimensionError, naming the driver, for a dataset that has not two or three axes"""
    shape0 = tuple(int(v) for v in dataset.shape)
    if len(shape0) not in (2, 3):
        raise DimensionError("{} needs a dataset of two or three axes. Got: {}".format(name, shape0))
    shape = (shape0 + (1,))[:3]
    return shape0, shape, np.array(shape, dtype=np.int64)


def label_type(dataset):
    """-> (dtype, is_bool, span: the smallest and largest label it holds) of a dataset or a loaded box, from its first voxel;
    TypeError unless integers or bool"""
    dtype = _load_box(dataset, (0, 0, 0), (1, 1, 1)).dtype
    if dtype != np.bool_ and dtype.kind not in "ui":
        raise TypeError("labels must be integers or bool")
    is_bool = dtype == np.bool_
    return dtype, is_bool, (0, 1) if is_bool else (int(np.iinfo(dtype).min), int(np.iinfo(dtype).max))


def _slices(lo, hi):
    return tuple(slice(int(a), int(b)) for a, b in zip(lo, hi))


def _load_box(dataset, lo, hi, name=None):
    """dataset[lo:hi] as a host array with three axes: numpy arrays of any order and memmaps, a tensor (copied from where it lives),
    anything that takes a tuple of slices (the h5py / zarr form).  With `name` (the driver's) a cut of another shape than hi - lo is
    a ValueError"""
    cut = dataset[_slices(lo, hi)[:len(dataset.shape)]]
    if hasattr(cut, "cpu") and hasattr(cut, "numpy"):
        cut = cut.cpu().numpy()
    cut = np.asarray(cut)
    cut = cut.reshape(cut.shape + (1,) * (3 - cut.ndim))
    if name is not None and cut.shape != tuple(int(b) - int(a) for a, b in zip(lo, hi)):
        raise ValueError("{}: dataset[{}:{}] has shape {}".format(name, [int(v) for v in lo], [int(v) for v in hi], cut.shape))
    return cut


def _store_box(target, lo, hi, box):
    """target[lo:hi] = box (a host array with three axes), for what _load_box reads: arrays and memmaps of two or three axes, a tensor
    (the box goes to where it lives), anything that takes a tuple of slices"""
    ndim = len(target.shape)
    box = box.reshape(box.shape[:ndim])
    if hasattr(target, "cpu") and hasattr(target, "numpy"):
        import torch
        signed = {"uint16": np.int16, "uint32": np.int32, "uint64": np.int64}.get(box.dtype.name)   # (as Engine.to_device moves words)
        piece = torch.from_numpy(np.ascontiguousarray(box if signed is None else box.view(signed))).to(target.device)
        target[_slices(lo, hi)[:ndim]] = piece if piece.dtype == target.dtype else piece.view(target.dtype)
    else:
        target[_slices(lo, hi)[:ndim]] = box


def store_like(given, shape, dtype, name, spelled=None, zeros=False):
    """A store of the dataset's `shape` (three axes) and `dtype`: `given` as it is when it is one, ValueError naming it otherwise;
    default a Fortran-ordered numpy array in host memory, uninitialised unless `zeros` (the drivers write every core before they
    read it).  `spelled`: the dtype's name in the message (default: numpy's)"""
    store = (np.zeros if zeros else np.empty)(shape, dtype=dtype, order="F") if given is None else given
    if tuple(int(v) for v in store.shape) != tuple(shape) or np.dtype(store.dtype) != np.dtype(dtype):
        raise ValueError("{}: {} of shape {}. Got: {} of shape {}".format(name, spelled or np.dtype(dtype).name, shape, store.dtype,
                                                                          tuple(store.shape)))
    return store


# cc3d's voxel-connectivity word listed by bit (the layout csrc/common.h reads: graph_to_directions / graph_bit_direction): bit b of a
# voxel's word allows the step GRAPH_STEP_OF_BIT[b] away from it
GRAPH_STEP_OF_BIT = (
    (1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1),
    (1, 1, 0), (-1, 1, 0), (1, -1, 0), (-1, -1, 0),
    (1, 0, 1), (-1, 0, 1), (0, 1, 1), (0, -1, 1),
    (1, 0, -1), (-1, 0, -1), (0, 1, -1), (0, -1, -1),
    (1, 1, 1), (-1, 1, 1), (1, -1, 1), (-1, -1, 1),
    (1, 1, -1), (-1, 1, -1), (1, -1, -1), (-1, -1, -1),
)


def graph_side_bits(axis, sign):
    """the bits of a voxel-connectivity word whose step goes towards `sign` (-1 / +1) along `axis`"""
    return sum(1 << b for b, step in enumerate(GRAPH_STEP_OF_BIT) if step[axis] == sign)


def clip_graph(box):
    """a box cut out of a dataset's voxel connectivity graph (three axes, _load_box) -> a Fortran-ordered uint32 copy with every bit
    that leaves the box cleared, on its six face planes: the graph of the box ALONE.  skeletonize reads such bits:
    the transform of a box that holds one value everywhere (black_border) asks the last voxel of an axis for its +x / +y / +z bit."""
    out = np.array(box, dtype=np.uint32, order="F")
    for axis in range(3):
        low, high = [slice(None)] * 3, [slice(None)] * 3
        low[axis], high[axis] = slice(0, 1), slice(out.shape[axis] - 1, out.shape[axis])
        out[tuple(low)] &= np.uint32(~graph_side_bits(axis, -1) & 0xFFFFFFFF)
        out[tuple(high)] &= np.uint32(~graph_side_bits(axis, 1) & 0xFFFFFFFF)
    return out


def label_table(skeletons, is_bool, span=None):
    """a dict, a list or one Skeleton -> (the skeletons as a list; per skeleton the label it names or None: utility._label_of; `table`:
    the distinct labels, sorted; `place`: {label: its index in table}).  With `span` the table leaves out a label the dataset's dtype
    cannot hold; without, whoever uses it filters"""
    skels = utility._skeleton_list(skeletons)
    labels_of = [utility._label_of(s, is_bool) for s in skels]
    table = sorted({L for L in labels_of if L is not None and (span is None or span[0] <= L <= span[1])})
    return skels, labels_of, table, {L: k for k, L in enumerate(table)}


def upload_labels(eng, host, span, table):
    """a host box of labels, uploaded as it is and narrowed to at most four bytes per label (utility._narrow_labels)
    -> (device labels, bytes per label, {label of `table` the box can hold: its word on the device})"""
    d_flat, itemsize, _, _, _, _ = _device_labels(eng, host)
    return utility._narrow_labels(eng, d_flat, itemsize, span, table)


def count_core(core, place, counts):
    """counts[place[L]] += the voxels of label L in the host array `core`, for every L in `place`"""
    values, found = np.unique(core, return_counts=True)
    for v, c in zip(values.tolist(), found.tolist()):
        if int(v) in place:
            counts[place[int(v)]] += c


def _device_core(d_box, ext, inner):
    """the slices `inner` ([x, y, z]) of a flat device box of extent `ext` (Fortran ordered: [z, y, x] as a view)"""
    return d_box.view(ext[2], ext[1], ext[0])[inner[2], inner[1], inner[0]]


def count_core_device(eng, d_lab, ext, inner, device_word, place, counts):
    """count_core on the device labels of a box (upload_labels), `inner` its core"""
    if device_word:
        found = utility._label_voxel_counts(eng, _device_core(d_lab, ext, inner).reshape(-1), device_word.values())
        for L, w in device_word.items():
            counts[place[L]] += found[w]


def group_by_core(cores, items):
    """{core: the entries of `items` whose entry of `cores` it is, in the order given}, cores ascending; both int64 [n]"""
    order = np.argsort(cores, kind="stable")
    ks, first = np.unique(cores[order], return_index=True)
    return dict(zip(ks.tolist(), np.split(items[order], first[1:])))


def up(eng, box):
    """a host box [x, y, z] of 32-bit words (or a flat table) -> flat device tensor in Fortran order, float32 as it is, u32 as int32
    words"""
    flat = np.asfortranarray(box).reshape(-1, order="F")
    return eng.torch.from_numpy(flat.view(np.int32) if flat.dtype == np.uint32 else flat).to(eng.device)


def down(d_box, ext, inner=None):
    """a flat device box of extent `ext` -> host [x, y, z] in the tensor's dtype: the whole box, or its slices `inner`"""
    if inner is None:
        return d_box.cpu().numpy().reshape(ext, order="F")
    return _device_core(d_box, ext, inner).contiguous().cpu().numpy().transpose(2, 1, 0)


def route_targets(targets, grid, shape):
    """Extra targets given as voxels of the dataset -> per chunk of `grid` the list of those its box contains, as (x, y, z) tuples
    relative to the box's low corner.  A point on an overlap plane goes to both boxes.  Two coordinates get z = 0.  IndexError, naming
    the point, for one outside a dataset of `shape`."""
    shape = (tuple(int(v) for v in shape) + (1,))[:3]
    out = [[] for _ in range(grid.box_lo.shape[0])]
    for target in targets:
        pt = tuple(int(v) for v in target)
        if len(pt) == 2:
            pt += (0,)
        if len(pt) != 3 or any(not 0 <= v < s for v, s in zip(pt, shape)):
            raise IndexError("point {} is outside a dataset of shape {}".format(tuple(target), shape))
        p = np.asarray(pt, dtype=np.int64)
        for k in np.flatnonzero(((grid.box_lo <= p) & (p < grid.box_hi)).all(axis=1)).tolist():
            out[k].append(tuple(int(v) for v in p - grid.box_lo[k]))
    return out


def count_labels(dataset, grid):
    """{label: voxels in the whole dataset}, zero included, from one pass over the cores of `grid` (they partition the dataset)"""
    total = defaultdict(int)
    for lo, hi in zip(grid.core_lo, grid.core_hi):
        values, counts = np.unique(_load_box(dataset, lo, hi), return_counts=True)
        for value, count in zip(values.tolist(), counts.tolist()):
            total[value] += count
    return dict(total)
