"""Host wrappers of the region-graph C functions (kh_host_resolve_holes, kh_host_enclosed_regions; no GPU needed): who fills what
once the regions of a label volume and their adjacency are known."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _abi


def resolve_holes(value, count, face, pairs):
    """kh_host_resolve_holes (host C, no GPU needed): the reference's loop over the labels (kimimaro/intake.py:763-790) on the region
    adjacency graph.  value (u64), count (u32), face (u8): the table of kh_region_table, [R + 1] with entry 0 unused; pairs (u64):
    every unordered pair of regions that share a voxel face once, as smaller id << 32 | larger id.
    Returns (owner u64 [R + 1]: the label a region is painted with, 0 = none; label_value u64 [nlabels]: the distinct non-zero
    labels ascending; label_state u8 [nlabels]: _abi.HOLES_PROCESSED | HOLES_FILLED | HOLES_KILLED; number of voxels filled)."""
    lib = _abi.lib()
    value = np.ascontiguousarray(value, dtype=np.uint64)
    count = np.ascontiguousarray(count, dtype=np.uint32)
    face = np.ascontiguousarray(face, dtype=np.uint8)
    pairs = np.ascontiguousarray(pairs, dtype=np.uint64)
    if not (value.ndim == count.ndim == face.ndim == pairs.ndim == 1 and value.size == count.size == face.size >= 1):
        raise ValueError("value, count and face are 1-D arrays of one length (regions + 1), pairs is 1-D")
    nreg = value.size - 1
    owner = np.zeros(nreg + 1, dtype=np.uint64)
    label_value = np.zeros(max(nreg, 1), dtype=np.uint64)
    label_state = np.zeros(max(nreg, 1), dtype=np.uint8)
    filled = C.c_int64(0)
    p = _abi.np_ptr
    nlab = lib.kh_host_resolve_holes(nreg, p(value), p(count), p(face), pairs.size, p(pairs), p(owner), p(label_value), p(label_state),
                                     C.byref(filled))
    if nlab == -1:
        raise MemoryError("kh_host_resolve_holes failed")
    if nlab < 0:
        raise ValueError("kh_host_resolve_holes: a pair names a region outside 1..%d, or joins a region with itself" % nreg)
    return owner, label_value[:nlab], label_state[:nlab], int(filled.value)


def enclosed_regions(value, face, pairs, labels):
    """kh_host_enclosed_regions (host C, no GPU needed): hole(L) for each of the wanted label words `labels` (u64, any order,
    duplicates allowed) on the region adjacency graph as given -- no dead set, no order among the labels, a region may be listed for
    several labels.  value (u64), face (u8), pairs (u64): as resolve_holes takes them.
    Returns (offsets u64 [len(labels) + 1], regions u32): label i's hole regions are regions[offsets[i]:offsets[i + 1]], ascending;
    empty for a label that does not occur or has no holes."""
    lib = _abi.lib()
    value = np.ascontiguousarray(value, dtype=np.uint64)
    face = np.ascontiguousarray(face, dtype=np.uint8)
    pairs = np.ascontiguousarray(pairs, dtype=np.uint64)
    labels = np.ascontiguousarray(labels, dtype=np.uint64)
    if not (value.ndim == face.ndim == pairs.ndim == labels.ndim == 1 and value.size == face.size >= 1):
        raise ValueError("value and face are 1-D arrays of one length (regions + 1), pairs and labels are 1-D")
    offsets = np.zeros(labels.size + 1, dtype=np.uint64)
    regions = np.zeros(0, dtype=np.uint32)
    p = lambda a: _abi.np_ptr(a) if a.size else None              # (NULL for an empty array)
    while True:                                      # the first call asks for the size, the second one fills
        total = lib.kh_host_enclosed_regions(value.size - 1, p(value), p(face), pairs.size, p(pairs), labels.size, p(labels), p(offsets),
                                             p(regions), regions.size)
        if total == -1:
            raise MemoryError("kh_host_enclosed_regions failed")
        if total < 0:
            raise ValueError("kh_host_enclosed_regions: a pair names a region outside 1..%d, or joins a region with itself" % (value.size - 1))
        if total <= regions.size:
            return offsets, regions[:total]
        regions = np.zeros(total, dtype=np.uint32)
