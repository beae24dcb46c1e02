"""The label volume on the host side: how an input becomes a three-axis Fortran-ordered array, the component volume that stays in
HBM (LazyVolume), and the index arithmetic of a Fortran-ordered volume.  numpy only; whatever touches the GPU takes the engine."""
from __future__ import annotations

import numpy as np


class DimensionError(Exception):
    pass


def as_3d(a):
    """the array with trailing axes of extent 1 up to three axes (a view)"""
    a = np.asarray(a)
    while a.ndim < 3:
        a = a[..., np.newaxis]
    return a


def linear_index(pt, shape):
    """x + sx * (y + sy * z) of one point"""
    return int(pt[0]) + shape[0] * (int(pt[1]) + shape[1] * int(pt[2]))


def coords_of(locs, shape):
    """linear indices -> (n, 3) int64 coordinates: the inverse of linear_index"""
    locs = np.asarray(locs, dtype=np.int64)
    return np.stack([locs % shape[0], (locs // shape[0]) % shape[1], locs // (shape[0] * shape[1])], axis=1)


def ranges(starts, counts):
    """concatenation of starts[i] + arange(counts[i]) over i, without a Python loop"""
    counts = np.asarray(counts, dtype=np.int64)
    total = int(counts.sum())
    before = np.cumsum(counts) - counts
    return np.repeat(np.asarray(starts, dtype=np.int64) - before, counts) + np.arange(total, dtype=np.int64)


def last_run_starts(t, ids, n):
    """skeletontricks.get_mapping's choice of voxel (skeletontricks.pyx:490-525) on the device: the raster (x fastest) is walked
    once and an id is (re)named wherever it differs from the PREVIOUS voxel's -- the last such place wins.  ids: int64 device tensor
    of the flat component volume, values 0..n.  Returns an int64 device tensor [n + 1]: per id the linear index of its last run
    start, -1 for an id that does not occur."""
    nvox = ids.numel()
    starts = t.ones(nvox, dtype=t.bool, device=ids.device)
    starts[1:] = ids[1:] != ids[:-1]
    sidx = t.nonzero(starts).reshape(-1)
    return t.full((n + 1,), -1, dtype=t.int64, device=ids.device).scatter_reduce(0, ids[sidx], sidx, reduce="amax")


def format_labels(labels, in_place=False):
    """The input as a Fortran-ordered array with exactly three axes, as kimimaro/intake.py:315-342 prepares it: bool
    volumes are reinterpreted as uint8, 1-D / 2-D inputs get trailing axes of extent 1, trailing singleton axes
    beyond the third are dropped, and a fourth non-trivial axis is a DimensionError (same message).  in_place avoids
    the copy when the array already is Fortran ordered."""
    vol = np.asfortranarray(labels) if in_place else np.array(labels, order="F", copy=True)
    if vol.dtype == np.bool_:
        vol = vol.view(np.uint8)
    given = vol.shape
    if vol.ndim > 3 and any(extent != 1 for extent in given[3:]):
        raise DimensionError(
            "Input labels may be no more than three non-trivial dimensions. Got: {}".format(given))
    return vol.reshape((given + (1, 1, 1))[:3], order="F")


def apply_object_mask(all_labels, object_ids):
    """kimimaro/intake.py:519-535."""
    if object_ids is None:
        return all_labels
    keep = np.isin(all_labels, np.asarray(list(object_ids), dtype=all_labels.dtype))
    all_labels[~keep] = 0
    return all_labels


def _device_labels(eng, all_labels):
    """-> (1-D device tensor in Fortran order, bytes per label, bool volume?, (sx, sy, sz), shape to return, (smallest, largest) label
    the dtype can hold).  numpy input goes through format_labels like skeletonize's; a torch tensor on the engine's device, indexed
    [x, y, z], is taken as it is (a view that is Fortran ordered already -- a contiguous (z, y, x) tensor permuted -- is not copied)."""
    t = eng.torch
    if isinstance(all_labels, t.Tensor):
        if all_labels.device != eng.device:
            raise ValueError("a label tensor must live on the engine's device (%s)" % eng.device)
        if all_labels.ndim > 3:
            raise ValueError("a label tensor has at most three axes")
        if all_labels.dtype.is_floating_point or all_labels.dtype.is_complex:
            raise TypeError("labels must be integers or bool")
        shape0 = tuple(int(v) for v in all_labels.shape)
        vol = all_labels
        while vol.ndim < 3:
            vol = vol.unsqueeze(-1)
        shape = tuple(int(v) for v in vol.shape)
        is_bool = vol.dtype == t.bool
        flat = vol.permute(2, 1, 0).contiguous().reshape(-1)
        size = flat.element_size()
        span = (-(1 << (8 * size - 1)), (1 << (8 * size - 1)) - 1) if vol.dtype.is_signed else (0, (1 << (8 * size)) - 1)
        return flat.view({1: t.uint8, 2: t.int16, 4: t.int32, 8: t.int64}[size]), size, is_bool, shape, shape0, span
    arr = np.asarray(all_labels)
    if arr.dtype != np.bool_ and arr.dtype.kind not in "ui":
        raise TypeError("labels must be integers or bool")
    is_bool = arr.dtype == np.bool_
    vol = format_labels(arr, in_place=True)          # (no copy of a Fortran-ordered volume: nothing here writes to it)
    info = np.iinfo(vol.dtype)
    return (eng.to_device(vol.view("u%d" % vol.dtype.itemsize)), vol.dtype.itemsize, is_bool, tuple(int(v) for v in vol.shape),
            arr.shape, (int(info.min), int(info.max)))


class LazyVolume:
    """The component volume lives in HBM; the few host-side consumers (border faces, extra-target lookups,
    soma crops) pull what they need, the whole array only if a soma label asks for its crop."""

    def __init__(self, eng, d_cc, shape, host=None):
        self.eng, self.d, self.shape, self._host = eng, d_cc, tuple(shape), host

    def host(self):
        if self._host is None:
            self._host = self.eng.to_host_volume(self.d, self.shape)
        return self._host

    def faces(self):
        if self._host is not None:
            c = self._host
            return (c[:, :, 0], c[:, :, -1], c[:, 0, :], c[:, -1, :], c[0, :, :], c[-1, :, :])
        e, d, s = self.eng, self.d, self.shape
        return (e.face(d, s, 2, 0), e.face(d, s, 2, s[2] - 1), e.face(d, s, 1, 0), e.face(d, s, 1, s[1] - 1),
                e.face(d, s, 0, 0), e.face(d, s, 0, s[0] - 1))

    def release_device(self):
        """drop this object's reference to the u32 component volume in HBM (0.5 GB at 512^3): skeletonize_cc calls it once the u16
        copy serves every remaining sweep and no soma label will ask for a crop -- the volumes in flight are bounded by memory.
        Callers that want the memory back must not keep a reference of their own (pass the volume through this object only)."""
        self.d = None

    def __getitem__(self, pt):
        if self._host is not None:
            return self._host[pt]
        x, y, z = (int(v) for v in pt)
        return int(self.d[x + self.shape[0] * (y + self.shape[1] * z)].item()) & 0xFFFFFFFF
