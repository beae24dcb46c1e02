"""CPU statement of the oversegment contract, independent of the product and of the oracle: numpy, heapq and
struct only.  Not the kernels' method (whole-volume pull sweeps) but the textbook one:

* distance  d: multi-source heap Dijkstra inside every label (26-connected), every sum rounded to float32 -- fl(d + w) is monotone
               in d, so Dijkstra yields the unique fixpoint of d(v) = min(0 at a seed, min_u fl(d(u) + w(u, v)));
* feature   f: voxels visited in ascending d; a seed voxel takes the smallest number seeded there, every other voxel the smallest
               f(u) among the neighbours u with fl(d(u) + w(u, v)) == d(v) (they all have d(u) < d(v), hence are done already);
* numbering  : kimimaro/utility.py:599-644 restated -- skeletons in container order, skipped when id == 0, label absent or its
               bounding box holds one voxel; vertex j of skeleton k provisionally base_k + j + 1; the composite renumbered 1..K by
               first appearance in the Fortran raster, smallest unsigned dtype that holds K; segments = composite at the vertices.
"""
import copy
import heapq
import struct

import numpy as np

_F32 = struct.Struct("f")
INF = float("inf")


def fl(x):
    """round a Python float to float32 (d + w of two float32 values is exact in double while d / w < 2^29: one rounding)"""
    return _F32.unpack(_F32.pack(x))[0]


def directions():
    return [(dx, dy, dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dx, dy, dz) != (0, 0, 0)]


def step_length(d, anisotropy):
    """float32 length of the step d: sqrt(fl(fl(a^2 + b^2) + c^2)), every operation rounded to float32"""
    f = np.float32
    a, b, c = (f(w) if k else f(0) for k, w in zip(d, np.asarray(anisotropy, dtype=np.float32)))
    return float(np.sqrt(f(f(f(a * a) + f(b * b)) + f(c * c))))


def _padded(ids):
    """dense ids (0 = background) with a one-voxel background frame, as a flat Fortran-ordered Python list"""
    sx, sy, sz = ids.shape
    pad = np.zeros((sx + 2, sy + 2, sz + 2), dtype=np.int64, order="F")
    pad[1:-1, 1:-1, 1:-1] = ids
    return pad.ravel(order="F").tolist(), sx + 2, sy + 2


def geodesic_voronoi(ids, seeds, anisotropy):
    """ids: int array [sx, sy, sz], 0 = background; seeds: iterable of ((x, y, z), number >= 1, id) -- one that is outside the
    array or not on its id seeds nothing.  Returns (dist float32, +inf where no seed reaches; feature int64, 0 there)."""
    ids = np.asarray(ids)
    sx, sy, sz = ids.shape
    lab, px, py = _padded(ids)
    steps = [(dx + px * (dy + py * dz), step_length((dx, dy, dz), anisotropy)) for dx, dy, dz in directions()]
    seed_number = {}
    for (x, y, z), number, want in seeds:
        if not (0 <= x < sx and 0 <= y < sy and 0 <= z < sz) or want == 0:
            continue
        p = (x + 1) + px * ((y + 1) + py * (z + 1))
        if lab[p] != want:
            continue
        seed_number[p] = min(number, seed_number.get(p, number))
    dist = [INF] * len(lab)
    heap = []
    for p in seed_number:
        dist[p] = 0.0
        heap.append((0.0, p))
    heapq.heapify(heap)
    while heap:
        d, p = heapq.heappop(heap)
        if d > dist[p]:
            continue
        L = lab[p]
        for off, w in steps:
            q = p + off
            if lab[q] == L:
                c = fl(d + w)
                if c < dist[q]:
                    dist[q] = c
                    heapq.heappush(heap, (c, q))
    feat = [0] * len(lab)
    reached = sorted((d, p) for p, d in enumerate(dist) if d != INF)
    for d, p in reached:
        if p in seed_number:
            feat[p] = seed_number[p]
            continue
        L = lab[p]
        best = None
        for off, w in steps:
            q = p + off
            if lab[q] == L and fl(dist[q] + w) == d:
                assert dist[q] < d
                if best is None or feat[q] < best:
                    best = feat[q]
        assert best is not None and best > 0, "a reached voxel has an achieving neighbour"
        feat[p] = best
    shape = (sx + 2, sy + 2, sz + 2)
    D = np.array(dist, dtype=np.float32).reshape(shape, order="F")[1:-1, 1:-1, 1:-1]
    F = np.array(feat, dtype=np.int64).reshape(shape, order="F")[1:-1, 1:-1, 1:-1]
    return np.asfortranarray(D), np.asfortranarray(F)


def as_volume(labels):
    a = np.asarray(labels)
    return a.reshape((a.shape + (1, 1, 1))[:3], order="F")


def vertex_voxels(skel, anisotropy):
    return (np.asarray(skel.vertices).reshape(-1, 3) / np.asarray(anisotropy, dtype=np.float32)).round().astype(np.int64)


def skeleton_list(skeletons):
    if hasattr(skeletons, "vertices"):
        return [skeletons]
    if isinstance(skeletons, dict):
        return list(skeletons.values())
    return list(skeletons)


def smallest_unsigned(k):
    for dt in (np.uint8, np.uint16, np.uint32, np.uint64):
        if k <= np.iinfo(dt).max:
            return dt


def renumber_first_appearance(comp):
    """1..K in the order of first appearance in the Fortran raster, 0 stays 0"""
    flat = comp.ravel(order="F")
    values, first = np.unique(flat, return_index=True)
    keep = values != 0
    values, first = values[keep], first[keep]
    values = values[np.argsort(first, kind="stable")]
    lut = {int(v): i + 1 for i, v in enumerate(values)}
    lut[0] = 0
    out = np.array([lut[int(v)] for v in flat], dtype=smallest_unsigned(len(values)))
    return out.reshape(comp.shape, order="F"), len(values)


def oversegment(all_labels, skeletons, anisotropy=(1, 1, 1)):
    """-> (all_features, deep copy of the skeletons with .segments, provisional composite before the renumbering)"""
    vol = as_volume(all_labels)
    is_bool = vol.dtype == np.bool_
    present = np.unique(vol)
    ids = np.searchsorted(present, vol) + 1             # dense ids; the background gets one too ...
    ids[vol == 0] = 0                                   # ... and loses it
    skeletons = copy.deepcopy(skeletons)
    skels = skeleton_list(skeletons)
    seeds, base = [], 0
    for skel in skels:
        label = 1 if is_bool else skel.id
        if label is None or label == 0:
            continue
        where = vol == label
        if not where.any():
            continue
        xs, ys, zs = np.nonzero(where)
        if (xs.max() - xs.min() + 1) * (ys.max() - ys.min() + 1) * (zs.max() - zs.min() + 1) <= 1:
            continue
        want = int(ids[xs[0], ys[0], zs[0]])
        vox = vertex_voxels(skel, anisotropy)
        for j, v in enumerate(vox):
            seeds.append((tuple(int(c) for c in v), base + j + 1, want))
        base += len(vox)
    dist, comp = geodesic_voronoi(ids, seeds, anisotropy)
    features, K = renumber_first_appearance(comp)
    sx, sy, sz = vol.shape
    for skel in skels:
        vox = vertex_voxels(skel, anisotropy)
        seg = np.zeros(len(vox), dtype=np.uint64)
        for j, (x, y, z) in enumerate(vox):
            if 0 <= x < sx and 0 <= y < sy and 0 <= z < sz:
                seg[j] = features[x, y, z]
        skel.segments = seg
        if not any(a["id"] == "segments" for a in skel.extra_attributes):
            skel.extra_attributes.append({"id": "segments", "data_type": "uint64", "num_components": 1})
    return features.reshape(np.asarray(all_labels).shape, order="F"), skeletons, (dist, comp, ids)
