"""kimimaro_amd.skeletonize -- host-side mirror of kimimaro.skeletonize (kimimaro/intake.py:58-221)
driving the HIP kernels.  Same signature, same defaults, same return type ({label: Skeleton}).

What runs where
  host (numpy)         format_labels / object mask / early outs (intake.py:147-160), connected
                       components (row f1, host C++ for now), border targets (row f2), Skeleton assembly.
  MI355X (libkimi_hip) whole-volume EDT (intake.py:174-185), per-label statistics, and for every
                       connected component the complete TEASAR trace (kimimaro/trace.py:36-267):
                       find_root, DAF, PDRF, target finder, railroad, rolling invalidation.

There is no CPU fallback: without libkimi_hip.so + an MI355X this raises HipUnavailableError.
"""
from __future__ import annotations

import os

from collections import defaultdict

import numpy as np

from . import _abi
from .engine import Engine, NONE32
from .plan import LabelSet
from .skeleton import Skeleton

DEFAULT_TEASAR_PARAMS = {  # kimimaro/intake.py:47-56
    "scale": 1.5,
    "const": 300,
    "pdrf_scale": 100000,
    "pdrf_exponent": 4,
    "soma_acceptance_threshold": 3500,
    "soma_detection_threshold": 750,
    "soma_invalidation_const": 300,
    "soma_invalidation_scale": 2,
}

# kimimaro/trace.py:38-43 -- the defaults trace() falls back to for keys missing from teasar_params
TRACE_DEFAULTS = {
    "scale": 10, "const": 10, "soma_detection_threshold": 1100, "soma_acceptance_threshold": 4000,
    "pdrf_scale": 5000, "pdrf_exponent": 16, "soma_invalidation_scale": 0.5, "soma_invalidation_const": 0,
    "max_paths": None,
}


class DimensionError(Exception):
    pass


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


def compute_cc_labels(all_labels):
    """kimimaro/utility.py:58-83 -> (cc_labels uint32 F-order, N, {cc id: original id}).
    Row f1: 26-connected multi-label CCL, host C++ helper in libkimi_hip.so for now."""
    lib = _abi.lib()
    lab = all_labels
    if lab.dtype.kind not in "ui" or lab.dtype.itemsize not in (1, 2, 4, 8):
        lab = lab.astype(np.uint64)
    lab = np.asfortranarray(lab)
    cc = np.zeros(lab.shape, dtype=np.uint32, order="F")
    import ctypes as C
    n = lib.kh_host_ccl26(lab.ctypes.data_as(C.c_void_p), lab.dtype.itemsize, lab.shape[0], lab.shape[1],
                          lab.shape[2], cc.ctypes.data_as(C.c_void_p))
    if n < 0:
        raise MemoryError("kh_host_ccl26 failed")
    flat_cc = cc.reshape(-1, order="F")
    idx = np.flatnonzero(flat_cc)
    uniq, first_idx = np.unique(flat_cc[idx], return_index=True)
    orig = all_labels.reshape(-1, order="F")[idx[first_idx]]
    remap = {int(u): orig[i].item() for i, u in enumerate(uniq)}  # skeletontricks.get_mapping :490-525
    return cc, int(n), remap


def compute_cc_labels_device(eng, all_labels, d_graph=None):
    """kimimaro/utility.py:58-83 on the MI355X (kh_ccl26; with a voxel graph kh_ccl26_graph): (device cc volume, N, {cc id: original id})."""
    d_cc, n, rep = eng.ccl(all_labels, d_graph)
    orig = all_labels.reshape(-1, order="F")[rep[1:].astype(np.int64)] if n else []
    remap = {i + 1: orig[i].item() for i in range(n)}  # skeletontricks.get_mapping :490-525
    return d_cc, n, remap


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


def _points_to_labels(pts, cc_labels):
    mapping = defaultdict(list)
    for pt in pts:
        pt = tuple(int(v) for v in pt)
        mapping[int(cc_labels[pt])].append(pt)
    return mapping


def _loc(pt, shape):
    return int(pt[0]) + shape[0] * (int(pt[1]) + shape[1] * int(pt[2]))


def skeletonize(all_labels, teasar_params=DEFAULT_TEASAR_PARAMS, anisotropy=(1, 1, 1),
                object_ids=None, dust_threshold=1000, progress=True, fix_branching=True,
                in_place=False, fix_borders=True, parallel=1, parallel_chunk_size=100,
                extra_targets_before=[], extra_targets_after=[], fill_holes=False,
                fix_avocados=False, voxel_graph=None, _timings=None, _engine=None):
    """Skeletonize all non-zero labels of a 2D/3D label image on the MI355X.

    Arguments and return value as kimimaro.skeletonize (kimimaro/intake.py:58-141).  `parallel` and
    `parallel_chunk_size` (process pool of the reference, intake.py:344-408) have no meaning here:
    one process drives one GPU; multi-GPU runs shard the connected components round robin over the
    ranks of torch.distributed (see kimimaro_amd.distributed).
    """
    eng = _engine or Engine()  # raises HipUnavailableError without a GPU: no CPU fallback
    anisotropy = np.array(anisotropy, dtype=np.float32)

    all_labels = format_labels(all_labels, in_place=in_place)
    all_labels = apply_object_mask(all_labels, object_ids)
    if all_labels.size <= dust_threshold:
        return {}
    minlabel, maxlabel = all_labels.min(), all_labels.max()
    if minlabel == 0 and maxlabel == 0:
        return {}

    d_graph = None
    if voxel_graph is not None:
        # kimimaro/intake.py:162,174-183,467: the graph decides the components (cc3d.color_connectivity_graph), puts walls into the
        # transform (edt.edt(voxel_graph=)) and goes to every search and to the invalidation of every label (trace(voxel_graph=)).
        # cc3d and edt are absent from the reference tree: kh_ccl26_graph / kh_edt_graph_* restate their published behaviour,
        # PARITY UNPINNED (include/kimi_hip.h).
        if fix_avocados:
            raise NotImplementedError("skeletonize(voxel_graph=, fix_avocados=True): the avocado pass re-labels components, which a "
                                      "graph of the ORIGINAL voxels does not describe")
        vg = np.asarray(voxel_graph)
        vg = vg.reshape((vg.shape + (1, 1, 1))[:3], order="F") if vg.ndim < 3 else vg
        if tuple(vg.shape) != tuple(all_labels.shape):
            raise ValueError("voxel_graph must have the shape of the labels")
        d_graph = eng.to_device(np.asfortranarray(vg.astype(np.uint32)))
    d_cc, nlabels, remapping = compute_cc_labels_device(eng, all_labels, d_graph)  # row f1 on the GPU
    if fill_holes:
        # intake.py:168-169.  The per-label loop until the one-pass route (Engine.fill_all_holes, same result: tests/
        # test_gpu_fill_holes.py) has been timed against it on c3 (tools/fill_holes_time.py; DESIGN.md 3.13, BENCH_NOTES.md)
        fill_all_holes_device(eng, d_cc, all_labels.shape, nlabels)
    avocado = None
    if fix_avocados:
        # kimimaro/intake.py:187-193 run BEFORE everything else that looks at the components: it edits them (and renumbers them)
        d_cc, nlabels, remapping, d_dbf_av = engage_avocado_protection_device(
            eng, d_cc, all_labels.shape, nlabels, remapping, anisotropy, bool(minlabel == maxlabel),
            teasar_params.get("soma_detection_threshold", 0))
        avocado = d_dbf_av
    cc = LazyVolume(eng, d_cc, all_labels.shape)
    del d_cc                   # (the volume is reached through `cc` from here on, which lets go of it as soon as it can)
    before = _points_to_labels(extra_targets_before, cc)
    after = _points_to_labels(extra_targets_after, cc)

    return skeletonize_cc(eng, cc, nlabels, remapping, teasar_params, anisotropy, dust_threshold,
                          fix_branching, fix_borders, before, after, black_border=(minlabel == maxlabel),
                          timings=_timings, d_dbf=avocado, d_graph=d_graph)


def _label_word(label, span, itemsize):
    """the unsigned word a volume whose dtype holds `span` = (smallest, largest) stores for `label`, None when `labels == label`
    is False everywhere whatever the volume holds (a value outside the dtype, a fraction, something that is no number)"""
    try:
        value = int(label)
        if value != label:
            return None
    except (TypeError, ValueError, OverflowError):
        return None
    if not span[0] <= value <= span[1]:
        return None
    return value % (1 << (8 * itemsize))


def synapses_to_targets(labels, synapses, progress=False):
    """kimimaro.synapses_to_targets (kimimaro/intake.py:706-745): turn the output of synapse detection into targets for
    skeletonize(extra_targets_after=...).  synapses: { label: [ (centroid, swc_label), ... ] }, centroid an (x, y, z) float triple in
    voxel coordinates.  For every label that occurs in the volume and every swc label of its pairs, the voxels of the label nearest
    to the centroids become targets.  Returns { (x, y, z): swc_label } with tuples of ints.

    The reference compares the volume with one label at a time and builds a dense cdist matrix per label; here all labels and all
    centroids go to the MI355X in one call (kh_nearest_label_voxels, two passes over the volume).  Distances are scipy's float64
    ones, among equally near voxels the first in C order wins (np.argmin over np.nonzero's enumeration).  Insertion and overwrite
    order are the reference's: labels in the order of `synapses`; within a label the swc labels in first-seen order; within an swc
    label the distinct winners in ascending C order; a later entry overwrites an equal key's value and keeps its place.
    labels: numpy, or a torch tensor on the GPU indexed [x, y, z].  Trailing axes beyond the third are dropped (`labels[..., 0]`,
    as the reference does); what is not 3-D then is a DimensionError.  `progress` is accepted and has no effect."""
    if len(synapses) == 0:
        return {}
    while labels.ndim > 3:
        labels = labels[..., 0]
    if labels.ndim != 3:
        raise DimensionError("synapses_to_targets needs a 3-D label volume. Got: {}".format(tuple(labels.shape)))
    from . import points
    from .ops import engine
    from .utility import _device_labels
    eng = engine()                                   # raises HipUnavailableError without the library or a gfx950 device
    d_flat, itemsize, _, shape, _, span = _device_labels(eng, labels)
    sx, sy, sz = shape

    # per label that the dtype can hold: its swc labels in first-seen order, each with its centroids (intake.py:735-737)
    groups, by_word = [], {}
    for label, pairs in synapses.items():
        word = _label_word(label, span, itemsize)
        swc = {}
        for centroid, swc_label in pairs:
            swc.setdefault(swc_label, []).append(np.asarray(centroid, dtype=np.float64).reshape(3))
        if word is None or not swc or word in by_word:
            groups.append(None)
            continue
        by_word[word] = len(groups)
        groups.append((word, swc))
    if not by_word:
        return {}
    words = np.array(sorted(by_word), dtype=np.uint64)
    counts = [sum(len(c) for c in groups[by_word[int(w)]][1].values()) for w in words]
    query_start = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)
    centroids = np.concatenate([np.stack(c) for w in words for c in groups[by_word[int(w)]][1].values()])
    winners = points.nearest_label_voxels(eng, d_flat, itemsize, shape, words, query_start, centroids)

    targets = {}
    for g in groups:
        if g is None:
            continue
        word, swc = g
        at = int(query_start[int(np.searchsorted(words, np.uint64(word)))])
        for swc_label, cens in swc.items():
            won = winners[at:at + len(cens)]
            at += len(cens)
            if won[0] == points.NONE64:              # the label does not occur (intake.py:732-733)
                break
            for c in np.unique(won).tolist():        # np.unique(np.argmin(...)): ascending C order
                targets[(c // (sy * sz), (c // sz) % sy, c % sz)] = swc_label
    return targets


def connect_points(labels, start, end, anisotropy=(1, 1, 1), fill_holes=False, in_place=False, pdrf_scale=100000, pdrf_exponent=4):
    """kimimaro.connect_points (kimimaro/intake.py:268-313): one centerline between two chosen voxels of a 2-D or 3-D binary image,
    in physical units.  The connected components come from the GPU CCL (kh_ccl26), the path from kimimaro_amd.trace.point_to_point.
    start / end: (x, y, z), or (x, y) for a 2-D image.  ValueError when `start` is background or the two lie in different
    components.  labels: numpy, or a torch tensor indexed [x, y, z].  `fill_holes` is accepted and ignored, as the reference ignores it."""
    anisotropy = np.array(anisotropy, dtype=np.float32)
    start, end = tuple(start), tuple(end)
    if hasattr(labels, "permute") and hasattr(labels, "cpu"):          # a torch tensor: the searches below take host arrays
        labels = labels.cpu().numpy()
    planar = np.ndim(labels) == 2
    labels = format_labels(np.asarray(labels).astype(bool), in_place=in_place)
    pts = []
    for pt in (start, end):
        pt = tuple(int(v) for v in pt)
        if planar and len(pt) == 2:
            pt += (0,)
        if len(pt) != 3 or any(not 0 <= v < s for v, s in zip(pt, labels.shape)):
            raise IndexError("point {} is outside an image of shape {}".format(pt, labels.shape))
        pts.append(pt)
    start, end = pts

    from .ops import engine
    from .trace import point_to_point
    eng = engine()                                   # raises HipUnavailableError without the library or a gfx950 device
    d_cc, _, _ = compute_cc_labels_device(eng, labels)
    cc = LazyVolume(eng, d_cc, labels.shape)
    if cc[start] == 0 or cc[start] != cc[end]:
        raise ValueError("Cannot extract centerline from disconnected components.")
    del cc, d_cc

    skel = point_to_point(labels, start, end, anisotropy=anisotropy, pdrf_scale=pdrf_scale, pdrf_exponent=pdrf_exponent)
    skel.vertices *= anisotropy
    skel.space = "physical"
    return skel


def _avocado_fruit_from_lines(xl, yl, zl, cx, cy, cz, background=0):
    """kimimaro.skeletontricks.find_avocado_fruit (skeletontricks.pyx:905-992) on the three axis-parallel lines of the label volume
    through (cx, cy, cz) (host copies): six rays from the voxel, each ends at the background or at the first other label, which it
    reports; the rays towards smaller coordinates stop BEFORE index 0 (`range(c, 0, -1)`).  Fewer than three reports: (label, label).
    The most frequent report -- the smallest label among equally frequent ones (np.unique order) -- is the fruit if at most one
    report disagrees with it (none when there are exactly three reports)."""
    label = int(xl[cx])
    rays = (xl[cx:], xl[cx:0:-1], yl[cy:], yl[cy:0:-1], zl[cz:], zl[cz:0:-1])
    changes = []
    for ray in rays:
        stop = np.flatnonzero((ray == background) | (ray != label))
        if stop.size and int(ray[stop[0]]) != background:
            changes.append(int(ray[stop[0]]))
    if len(changes) < 3:
        return label, label
    uniq, cts = np.unique(changes, return_counts=True)
    k = int(np.argmax(cts))
    if len(changes) - int(cts[k]) > (1 if len(changes) > 3 else 0):
        return label, label
    return label, int(uniq[k])


def engage_avocado_protection_device(eng, d_cc, shape, nlabels, remapping, anisotropy, black_border, soma_detection_threshold):
    """kimimaro/intake.py:600-704 (fix_avocados=True) on the component volume resident in HBM: a nucleus that carries a label of its
    own inside its cell ("pit" in "fruit") is merged into the cell, holes filled, up to 20 passes for nested ones; then the
    components are renumbered (fastremap.renumber: by first appearance) and mapped back to the original labels
    (skeletontricks.get_mapping, skeletontricks.pyx:490-525).  Device work: the transforms (kh_edt), the bounding boxes
    (kh_label_stats), the 2-D fills of the six faces of a crop and its 3-D fill (kh_fill_voids_nd); selections, arg-max and the
    relabelling are device-side tensor plumbing; the host reads three lines of labels per candidate (find_avocado_fruit's rays)
    and keeps the reference's sets -- INCLUDING their iteration order: the candidates of a pass are a Python set built from the
    sorted unique labels, and the reference edits the volume in that set's order.
    Returns (component volume u32 on the device, number of components, {component: original label}, its EDT)."""
    t = eng.torch
    sx, sy, sz = (int(v) for v in shape)
    nvox = sx * sy * sz
    d_cc = d_cc.clone()                      # (the caller's volume may be shared)
    orig = d_cc.clone()
    v = d_cc.view(sz, sy, sx)                # torch C order (z, y, x) == Fortran order (x, y, z)
    d_dbf = eng.edt(d_cc, 4, shape, anisotropy, black_border)
    thr = float(np.float32(soma_detection_threshold / 2.5))     # numpy compares the f32 field with the scalar in float32
    unchanged = set()
    for _ in range(20):
        vals = t.unique(d_cc[d_dbf > thr]).cpu().numpy().view(np.uint32)       # sorted, like fastremap.unique
        candidates = set([0] + [int(x) for x in vals]) if bool((d_dbf <= thr).any()) else set(int(x) for x in vals)
        candidates -= unchanged
        candidates.discard(0)
        order = [label for label in candidates if label != 0]
        changed, unchanged_now = set(), set()          # (the sets of ONE pass, intake.py:650-651)
        if order:
            stats = eng.label_stats(d_cc, 4, d_dbf, shape, nlabels)
            for label in order:
                lo, hi = stats.bbox(label)
                sub = eng.box(d_cc, shape, lo, hi)
                binimg = (sub == label)
                # paint_walls (:655-666): a 2-D fill on each of the six faces, in the reference's order
                for face in ((-1, 0), (-1, -1), (1, 0), (1, -1), (2, 0), (2, -1)):      # (torch axis, index): z, z, y, y, x, x
                    ax = 0 if face[0] == -1 else face[0]
                    plane = binimg.select(ax, face[1])
                    p2 = plane.to(t.uint8).contiguous()
                    filled, nfill = eng.fill_voids(p2.view(-1), (p2.shape[1], p2.shape[0], 1), ndim=2)
                    if nfill:
                        plane.copy_(filled.view(p2.shape).bool())
                prod = binimg * eng.box(d_dbf, shape, lo, hi)
                k = int(t.argmax(prod.reshape(-1)).item())            # first maximum in the raster (x fastest), like argmax(arr.T)
                nx, ny = hi[0] - lo[0], hi[1] - lo[1]
                cx, cy, cz = lo[0] + k % nx, lo[1] + (k // nx) % ny, lo[2] + k // (nx * ny)
                lines = [a.cpu().numpy().view(np.uint32) for a in (v[cz, cy, :], v[cz, :, cx].contiguous(), v[:, cy, cx].contiguous())]
                pit, fruit = _avocado_fruit_from_lines(lines[0], lines[1], lines[2], cx, cy, cz)
                if pit == fruit and pit not in changed:
                    unchanged_now.add(pit)
                else:
                    unchanged_now.discard(pit)
                    unchanged_now.discard(fruit)
                    changed.add(pit)
                    changed.add(fruit)
                    binimg |= (sub == fruit)
                cshape = (hi[0] - lo[0], hi[1] - lo[1], hi[2] - lo[2])
                filled, _ = eng.fill_voids(binimg.to(t.uint8).contiguous().view(-1), cshape)
                fb = filled.view(cshape[2], cshape[1], cshape[0]).bool()
                sub[fb] = fruit                               # cc_labels[slc] *= ~binimg; cc_labels[slc] += fruit * binimg
        unchanged |= unchanged_now
        if len(changed) == 0:
            break
        d_dbf = eng.edt(d_cc, 4, shape, anisotropy, black_border)
    # fastremap.renumber: 1..N by first appearance in memory; get_mapping: the LAST run start of a component in the raster names it
    flat = d_cc.to(t.int64) & 0xFFFFFFFF
    idx = t.arange(nvox, device=eng.device, dtype=t.int64)
    top = int(flat.max().item()) + 1
    first = t.full((top,), nvox, dtype=t.int64, device=eng.device).scatter_reduce(0, flat, idx, reduce="amin")
    present = t.nonzero(first < nvox).reshape(-1)
    present = present[present != 0]
    by_first = present[t.argsort(first[present], stable=True)]
    lut = t.zeros(top, dtype=t.int64, device=eng.device)
    lut[by_first] = t.arange(1, by_first.numel() + 1, device=eng.device, dtype=t.int64)
    new = lut[flat]
    starts = t.ones(nvox, dtype=t.bool, device=eng.device)
    starts[1:] = new[1:] != new[:-1]
    sidx = t.nonzero(starts).reshape(-1)
    n_new = int(by_first.numel())
    last = t.full((n_new + 1,), -1, dtype=t.int64, device=eng.device).scatter_reduce(0, new[sidx], sidx, reduce="amax")
    last_h = last.cpu().numpy()
    src = (orig.to(t.int64) & 0xFFFFFFFF)[last.clamp(min=0)].cpu().numpy()
    adjusted = {}
    for new_cc in range(0, n_new + 1):
        if last_h[new_cc] >= 0 and int(src[new_cc]) in remapping:
            adjusted[new_cc] = remapping[int(src[new_cc])]
    return new.to(t.int32), n_new, adjusted, d_dbf       # (renumbering does not move a voxel: the last transform stands)


def fill_all_holes_device(eng, d_cc, shape, nlabels):
    """kimimaro/intake.py:747-795 on the component volume resident in HBM (modified in place): the holes of every
    component are filled with kh_fill_voids on the component's bounding box, in ascending label order; a component
    that gets swallowed is not processed itself any more.  Bounding boxes are those before any filling, as in the
    reference (find_objects is called once, intake.py:767).  Returns the number of voxels filled."""
    eng.edited(d_cc)
    t = eng.torch
    nvox = int(shape[0]) * int(shape[1]) * int(shape[2])
    stats = eng.label_stats(d_cc, 4, t.zeros(nvox, dtype=t.float32, device=eng.device), shape, nlabels)
    in_set = np.ones(nlabels + 1, dtype=bool)
    in_set[0] = False
    filled_total = 0
    for label in range(1, nlabels + 1):
        if not in_set[label] or stats.counts[label] == 0:
            continue
        lo, hi = stats.bbox(label)
        cshape = (hi[0] - lo[0], hi[1] - lo[1], hi[2] - lo[2])
        sub = eng.box(d_cc, shape, lo, hi)
        d_filled, n = eng.fill_voids((sub == label).to(t.uint8).contiguous().view(-1), cshape)
        if n == 0:
            continue
        filled_total += n
        fb = d_filled.view(cshape[2], cshape[1], cshape[0]).bool()
        for other in t.unique(sub[fb]).cpu().numpy():
            if other != label and other > 0:
                in_set[int(other)] = False
        sub[fb] = label
    return filled_total


def resolve_holes(value, count, face, pairs):
    """kh_host_resolve_holes (host C, no GPU needed): the reference's loop over the labels (kimimaro/intake.py:763-790) on the region
    adjacency graph.  value (u64), count (u32), face (u8): the table of kh_region_table, [R + 1] with entry 0 unused; pairs (u64):
    every unordered pair of regions that share a voxel face once, as smaller id << 32 | larger id.
    Returns (owner u64 [R + 1]: the label a region is painted with, 0 = none; label_value u64 [nlabels]: the distinct non-zero
    labels ascending; label_state u8 [nlabels]: _abi.HOLES_PROCESSED | HOLES_FILLED | HOLES_KILLED; number of voxels filled)."""
    import ctypes as C
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
    p = lambda a: a.ctypes.data_as(C.c_void_p)
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
    import ctypes as C
    lib = _abi.lib()
    value = np.ascontiguousarray(value, dtype=np.uint64)
    face = np.ascontiguousarray(face, dtype=np.uint8)
    pairs = np.ascontiguousarray(pairs, dtype=np.uint64)
    labels = np.ascontiguousarray(labels, dtype=np.uint64)
    if not (value.ndim == face.ndim == pairs.ndim == labels.ndim == 1 and value.size == face.size >= 1):
        raise ValueError("value and face are 1-D arrays of one length (regions + 1), pairs and labels are 1-D")
    offsets = np.zeros(labels.size + 1, dtype=np.uint64)
    regions = np.zeros(0, dtype=np.uint32)
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a.size else None
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


def fill_all_holes(cc_labels, progress=False, return_fill_count=False):
    """kimimaro.intake.fill_all_holes (kimimaro/intake.py:747-795): fills the holes of every label and removes the labels that get
    filled in.  A hole of L is what fill_voids.fill paints on L's bounding box: the voxels that no 6-connected path outside L joins
    to a face of the array.  The labels take their turn in ascending order; a label that lay (even partly) in a hole that was
    filled does not get its own turn.

    cc_labels: numpy array (any memory order, at most three non-trivial axes, integers or bool), or a torch tensor on the GPU
      indexed [x, y(, z)].  It is modified in place and returned.  Values need not be dense, nor need a value be connected
      (the reference asks for values below the number of voxels because it indexes find_objects' list); they are ordered as
      the unsigned words the array holds.
    progress: accepted, no effect.
    return_fill_count: return (cc_labels, N), N = the number of voxels filled (a voxel filled twice counts twice, as there).

    One pass over the volume on the MI355X (Engine.fill_all_holes); HipUnavailableError without one."""
    from .ops import engine
    from .utility import _device_labels
    eng = engine()                                   # raises HipUnavailableError without the library or a gfx950 device
    t = eng.torch
    is_tensor = isinstance(cc_labels, t.Tensor)
    if not is_tensor and not isinstance(cc_labels, np.ndarray):
        raise TypeError("cc_labels must be a numpy array or a torch tensor (it is modified in place)")
    if cc_labels.ndim < 1:
        raise DimensionError("fill_all_holes needs an array with at least one axis")
    filled = 0
    if (cc_labels.numel() if is_tensor else cc_labels.size) > 0:
        d_flat, itemsize, _, shape, shape0, _ = _device_labels(eng, cc_labels)
        filled = eng.fill_all_holes(d_flat, itemsize, shape, ndim=min(cc_labels.ndim, 3))
        if filled:
            if is_tensor:
                if d_flat.data_ptr() != cc_labels.data_ptr():          # (a Fortran-ordered view was edited where it lies)
                    like = cc_labels.dtype if cc_labels.dtype == t.bool else d_flat.dtype
                    cc_labels.view(like).copy_(d_flat.view(like).view(shape[2], shape[1], shape[0]).permute(2, 1, 0).reshape(shape0))
            else:
                word = np.dtype("u%d" % itemsize)
                host = d_flat.cpu().numpy().view(word).reshape(shape, order="F")
                cc_labels[...] = host.view(np.bool_ if cc_labels.dtype == np.bool_ else cc_labels.dtype).reshape(cc_labels.shape, order="F")
    return (cc_labels, filled) if return_fill_count else cc_labels


def shard_components(cc_segids, counts, rank, world):
    """The components rank `rank` of `world` traces.  The reference deals them round robin (kimimaro/intake.py:388-389:
    cc_segids[i::parallel]); the cost of a component grows with its voxel count and the tail of the size distribution is
    heavy, so here they are dealt largest first to the rank with the least voxels so far (LPT; ties -> lowest rank).
    Deterministic: every rank computes the same assignment from the same counts."""
    order = sorted(cc_segids, key=lambda s: (-int(counts[s]), s))
    load = [0] * world
    mine = []
    for s in order:
        r = min(range(world), key=lambda k: (load[k], k))
        load[r] += int(counts[s])
        if r == rank:
            mine.append(s)
    return sorted(mine)


def skeletonize_cc(eng, cc_labels, nlabels, remapping, teasar_params, anisotropy, dust_threshold,
                   fix_branching, fix_borders, before, after, black_border, timings=None,
                   rank=0, world=1, d_cc=None, d_dbf=None, d_graph=None):
    """Everything after the connected components (intake.py:174-221 + skeletonize_subset :434-517)."""
    import time as _time

    def _mark(name):
        if timings is not None:
            eng.sync_stream()
            timings.append((name, _time.perf_counter()))

    _mark("start")
    if not isinstance(cc_labels, LazyVolume):
        cc_labels = LazyVolume(eng, d_cc, cc_labels.shape, host=cc_labels)
    shape = cc_labels.shape
    label_bytes = 4
    if d_cc is None:
        d_cc = cc_labels.d
    if d_cc is None:
        d_cc = eng.to_device(cc_labels.host())
        cc_labels.d = d_cc
    d_lab, label_bytes = eng.narrow(d_cc)          # u16 ids when there are < 65536 components (utility.py:79 refit)
    if d_dbf is None and d_graph is not None:
        d_dbf = eng.edt_graph(d_lab, label_bytes, d_graph, shape, anisotropy, black_border)  # intake.py:174-185 with voxel_graph
    if d_dbf is None:         # (fix_avocados hands over the transform of the components it left behind)
        d_dbf = eng.edt(d_lab, label_bytes, shape, anisotropy, black_border)  # intake.py:174-185
    stats = eng.label_stats(d_lab, label_bytes, d_dbf, shape, nlabels)
    counts, dbf_max = stats.counts, stats.dbf_max
    _mark("edt+stats")

    # intake.py:198-201
    cc_segids = [sid for sid in range(1, nlabels + 1) if counts[sid] > dust_threshold]
    border_targets = defaultdict(list)
    if fix_borders:
        from .border import compute_border_targets
        border_targets = compute_border_targets(None, anisotropy, eng=eng, faces=cc_labels.faces(), shape=shape)  # intake.py:207

    _mark("border_targets")
    params = dict(TRACE_DEFAULTS)
    params.update(teasar_params)
    if world > 1:
        cc_segids = shard_components(cc_segids, counts, rank, world)

    soma_jobs = []
    segids, roots, tb, ta = [], [], [], []
    for segid in cc_segids:
        # intake.py:454-456: bounding boxes of volume <= 1 are skipped (never true above dust_threshold >= 1)
        if counts[segid] <= 1 and dust_threshold < 1:
            continue
        mtb, mta, root = [], [], NONE32
        if len(border_targets[segid]) > 0:                      # intake.py:486-488
            mtb = [_loc(p, shape) for p in border_targets[segid]]
            root = mtb.pop()
        if segid in before and len(before[segid]) > 0:
            mtb.extend(_loc(p, shape) for p in before[segid])
        if segid in after and len(after[segid]) > 0:
            mta.extend(_loc(p, shape) for p in after[segid])
        if dbf_max[segid] > params["soma_detection_threshold"] and _needs_soma_path(
                eng, d_cc, shape, stats.bbox(segid), segid, float(dbf_max[segid]), params):
            soma_jobs.append((segid, root, mtb, mta))  # traced one by one on their crop, below
            continue
        segids.append(segid)
        roots.append(root)
        tb.append(mtb)
        ta.append(mta)

    if not soma_jobs and label_bytes == 2 and d_lab is not d_cc and os.environ.get("KH_KEEP_CC", "0") != "1":
        # nothing reads the u32 ids any more (the faces are taken, no soma crop will be asked for): the u16 copy, which d_lab holds,
        # serves from here on
        d_cc = None
        cc_labels.release_device()
    sel = np.asarray(segids, dtype=np.int64)
    asm = Assembler(shape, anisotropy, remapping)
    labels = LabelSet(sel, counts[sel], dbf_max[sel], stats.first_index[sel], stats.xmin[sel], stats.xmax[sel], roots, tb, ta)
    eng.run_labels(d_lab, label_bytes, d_dbf, shape, anisotropy, nlabels, labels, params, fix_branching=fix_branching,
                   max_paths=params.get("max_paths"), timings=timings, consume=asm.add, voxel_graph=d_graph)
    out = asm.finish()
    _mark("assemble")
    if soma_jobs:
        _trace_soma_labels(eng, soma_jobs, d_cc, d_dbf, shape, anisotropy, remapping, params, fix_branching, stats.bbox, out, d_graph)
        _mark("soma_labels")
    return out


def _trace_soma_labels(eng, jobs, d_cc, d_dbf, shape, anisotropy, remapping, params, fix_branching, bbox, out, d_graph=None):
    """Labels that enter the soma branch of kimimaro/trace.py:108-134 (internal voids to fill, or DBF max above
    soma_acceptance_threshold) leave the shared-volume batch -- filling voids changes which voxels belong to
    the label -- and are traced on their bounding-box crop, exactly like intake.py:450-517.  The reference gives every
    label a process of its pool (intake.py:344-408); here several somas of one volume run side by side, each on a host
    thread with an Engine and a HIP stream of its own (`Engine.soma_lanes`, kimimaro_amd.lanes.Lanes); the skeletons are
    merged in the order of the labels either way."""
    from .trace import trace as trace_one
    sx, sy = shape[0], shape[1]
    an = np.asarray(anisotropy, dtype=np.float32)
    unloc = lambda l: (l % sx, (l // sx) % sy, l // (sx * sy))
    kw = {k: params[k] for k in ("scale", "const", "pdrf_scale", "pdrf_exponent", "soma_detection_threshold",
                                 "soma_acceptance_threshold", "soma_invalidation_scale", "soma_invalidation_const")}

    def one(e, i):
        segid, root, mtb, mta = jobs[i]
        lo, hi = bbox(segid)
        minpt = np.array(lo, dtype=np.int64)
        labels = e.crop(d_cc, shape, lo, hi) == segid
        dbf = np.where(labels, e.crop(d_dbf, shape, lo, hi, np.float32), 0.0).astype(np.float32)
        tr = lambda ls: [tuple(int(v) for v in (np.array(unloc(l)) - minpt)) for l in ls]
        skel = trace_one(labels, dbf, anisotropy=an, fix_branching=fix_branching, manual_targets_before=tr(mtb),
                         manual_targets_after=tr(mta), root=(None if root == NONE32 else tr([root])[0]),
                         max_paths=params.get("max_paths"), _engine=e,
                         voxel_graph=(None if d_graph is None else e.crop(d_graph, shape, lo, hi)), **kw)    # intake.py:467
        if not skel.empty():
            skel.vertices += minpt.astype(skel.vertices.dtype)
        return skel

    width = min(int(getattr(eng, "soma_lanes", 1)), len(jobs))
    if width > 1:
        eng.sync_stream()              # the component volume and its EDT are complete before another stream reads them
        results = (skel for _, skel in eng.soma_lane_pool(width).run(one, len(jobs), width=width))
    else:
        results = (one(eng, i) for i in range(len(jobs)))
    for (segid, _, _, _), skel in zip(jobs, results):
        if skel.empty():
            continue
        orig = remapping[segid]
        skel.id = orig
        skel.vertices = np.multiply(skel.vertices, an, dtype=np.float32)
        skel.space = "physical"
        out[orig] = Skeleton.simple_merge([out[orig], skel]).consolidate() if orig in out else skel.consolidate()


def _needs_soma_path(eng, d_cc, shape, box, segid, dbf_max, params):
    """kimimaro/trace.py:108-119 for a label whose DBF max exceeds soma_detection_threshold: does it take the
    soma branch?  True if the DBF max is already above soma_acceptance_threshold, or if the label has
    internal voids (fill_voids.fill would change it and its DBF; kh_fill_voids on the label's crop).  A label
    without voids below the acceptance threshold continues unchanged in the reference, so it stays in the
    shared-volume batch."""
    if dbf_max > params["soma_acceptance_threshold"]:
        return True
    t = eng.torch
    lo, hi = box
    cshape = (hi[0] - lo[0], hi[1] - lo[1], hi[2] - lo[2])
    d_mask = (eng.box(d_cc, shape, lo, hi) == int(segid)).to(t.uint8).contiguous().view(-1)
    _, nfilled = eng.fill_voids(d_mask, cshape)
    return nfilled > 0


def paths_of(res, slot, shape):
    """list of (n,3) integer voxel paths of task `slot`."""
    sx, sy = shape[0], shape[1]
    v0, l0, l1 = res["voff"][slot], res["loff"][slot], res["loff"][slot + 1]
    out = []
    pos = v0
    for n in res["lens"][l0:l1]:
        locs = res["verts"][pos:pos + n].astype(np.int64)
        out.append(np.stack([locs % sx, (locs // sx) % sy, locs // (sx * sy)], axis=1))
        pos += n
    return out


def consolidate_paths(locs, lens, radii, shape):
    """Skeleton.from_path per path + simple_merge + consolidate (kimimaro/trace.py:182-184) for one label, on
    linear voxel indices: returns (vertices (n,3) f32 sorted lexicographically by (x,y,z) like
    np.unique(axis=0), edges (m,2) u32 sorted/unique without self loops, radii of the first occurrences).
    Same result as kimimaro_amd.skeleton.Skeleton.consolidate (vertices no edge refers to dropped), ~10x cheaper
    (1-D unique on a key)."""
    sx, sy, sz = shape
    x, y, z = locs % sx, (locs // sx) % sy, locs // (sx * sy)
    key = (x * sy + y) * sz + z                      # row-lexicographic order of (x, y, z)
    ukey, first, inv = np.unique(key, return_index=True, return_inverse=True)
    n = locs.size
    starts = np.cumsum(lens)[:-1]
    eidx = np.arange(n - 1)
    if starts.size:
        keep = np.ones(n - 1, dtype=bool)
        keep[starts - 1] = False                     # no edge across two paths
        eidx = eidx[keep]
    a, b = inv[eidx], inv[eidx + 1]
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    ok = lo != hi
    ekey = np.unique(lo[ok] * np.int64(ukey.size) + hi[ok])
    edges = np.stack([ekey // ukey.size, ekey % ukey.size], axis=1)
    used = np.zeros(ukey.size, dtype=bool)
    used[edges.ravel()] = True
    if not used.all():      # a one-vertex path off every other path: no edge refers to it (consolidate drops it)
        first, edges = first[used], (np.cumsum(used) - 1)[edges]
    verts = np.stack([x[first], y[first], z[first]], axis=1).astype(np.float32)
    return verts, edges.astype(np.uint32), radii[first]


def _ranges(starts, counts):
    """concatenation of starts[i] + arange(counts[i]) over i, without a Python loop"""
    counts = np.asarray(counts, dtype=np.int64)
    total = int(counts.sum())
    before = np.cumsum(counts) - counts
    return np.repeat(np.asarray(starts, dtype=np.int64) - before, counts) + np.arange(total, dtype=np.int64)


def consolidate_paths_flat(res, shape):
    """consolidate_paths for EVERY label of a result group in ONE native call outside the interpreter
    (kh_host_consolidate_paths, include/kimi_hip.h: with twenty volumes in flight the lanes reach this point together and what
    holds the interpreter lock is paid twenty times in a row).  Returns None for a group without vertices, else the slots' arrays
    back to back: verts (N,3) f32, radii (N) f32, edges (M,2) u32 with indices local to the slot, vstart / estart [nslots+1].
    Same arrays as consolidate_paths_flat_numpy (tests/test_host.py compares them)."""
    import ctypes as C
    from . import _abi
    sx, sy, sz = shape
    voff = np.ascontiguousarray(res["voff"], dtype=np.int64)
    loff = np.ascontiguousarray(res["loff"], dtype=np.int64)
    nslots = voff.size - 1
    locs = np.ascontiguousarray(res["verts"], dtype=np.uint32)
    n = int(locs.size)
    if n == 0:
        return None
    lens = np.ascontiguousarray(res["lens"], dtype=np.uint32)
    radii = np.ascontiguousarray(res["radii"], dtype=np.float32)
    oV, oR, oE = np.empty((n, 3), np.float32), np.empty(n, np.float32), np.empty((n, 2), np.uint32)
    vstart, estart = np.empty(nslots + 1, np.int64), np.empty(nslots + 1, np.int64)
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    got = _abi.lib().kh_host_consolidate_paths(nslots, P(voff), P(loff), P(locs), P(lens), P(radii), int(sx), int(sy), int(sz),
                                               P(oV), P(oR), P(oE), P(vstart), P(estart))
    if got < 0:
        raise MemoryError("kh_host_consolidate_paths failed")
    return {"verts": oV[:got], "radii": oR[:got], "edges": oE[:int(estart[-1])], "vstart": vstart, "estart": estart, "voff": voff}


def consolidate_paths_flat_numpy(res, shape):
    """the numpy form of consolidate_paths_flat (one sort over all path vertices instead of three np.unique calls per label); kept
    as the statement the native call is tested against.  consolidate_paths for EVERY label of a result group in one go (one sort over all path vertices instead of three
    np.unique calls per label: the per-label numpy overhead, 170 us x 3.4 k labels, was most of the assembly time of a
    512^3 volume).  Returns None for a group without vertices, else the slots' arrays back to back:
    verts (N,3) f32, radii (N) f32, edges (M,2) u32 with indices local to the slot, vstart / estart [nslots+1]."""
    sx, sy, sz = shape
    voff = np.asarray(res["voff"], dtype=np.int64)
    nslots = voff.size - 1
    locs = res["verts"].astype(np.int64)
    n = locs.size
    if n == 0:
        return None
    V = np.int64(sx) * sy * sz
    slot_of = np.repeat(np.arange(nslots, dtype=np.int64), np.diff(voff))
    x, y, z = locs % sx, (locs // sx) % sy, locs // (sx * sy)
    key = slot_of * V + (x * sy + y) * sz + z                 # slot, then row-lexicographic order of (x, y, z)
    ukey, first, inv = np.unique(key, return_index=True, return_inverse=True)
    nu = ukey.size
    uslot = ukey // V
    ustart = np.searchsorted(uslot, np.arange(nslots + 1, dtype=np.int64))     # unique vertices of slot s: [ustart[s], ustart[s+1])
    # consecutive pairs inside a path are edges: drop the pair that straddles two paths (path ends, incl. label ends)
    lens = res["lens"].astype(np.int64)
    path_end = np.cumsum(lens) - 1
    keep = np.ones(max(n - 1, 0), dtype=bool)
    keep[path_end[path_end < n - 1]] = False
    eidx = np.flatnonzero(keep)
    a, b = inv[eidx], inv[eidx + 1]
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    ok = lo != hi
    ekey = np.unique(lo[ok] * np.int64(nu) + hi[ok])           # sorted by (lo, hi): grouped by slot, rows sorted like np.unique(axis=0)
    elo, ehi = ekey // nu, ekey % nu
    used = np.zeros(nu, dtype=bool)
    used[elo] = True
    used[ehi] = True
    # vertices no edge refers to are dropped (Skeleton.consolidate); local index = rank among the slot's used vertices
    cum = np.concatenate([[0], np.cumsum(used)])
    rank = cum[1:] - 1
    base = cum[ustart[:-1]] if nu else np.zeros(nslots, np.int64)
    fu = first[used]
    verts_all = np.stack([x[fu], y[fu], z[fu]], axis=1).astype(np.float32)
    radii_all = res["radii"][fu]
    vstart = cum[ustart]                                       # used vertices of slot s: [vstart[s], vstart[s+1])
    eslot = uslot[elo]
    estart = np.searchsorted(eslot, np.arange(nslots + 1, dtype=np.int64))
    edges_all = np.stack([rank[elo] - base[eslot], rank[ehi] - base[eslot]], axis=1).astype(np.uint32)
    return {"verts": verts_all, "radii": radii_all, "edges": edges_all, "vstart": vstart, "estart": estart, "voff": voff}


def consolidate_paths_batch(res, shape):
    """consolidate_paths_flat slot by slot: yields (slot, vertices (n,3) f32, edges (m,2) u32, radii) for the slots that have
    vertices, the same arrays the per-label function returns."""
    f = consolidate_paths_flat(res, shape)
    if f is None:
        return
    vstart, estart, voff = f["vstart"], f["estart"], f["voff"]
    for s in range(voff.size - 1):
        if voff[s + 1] == voff[s]:
            continue
        yield s, f["verts"][vstart[s]:vstart[s + 1]], f["edges"][estart[s]:estart[s + 1]], f["radii"][vstart[s]:vstart[s + 1]]


class Assembler:
    """Skeleton assembly: kimimaro/trace.py:182-192 + intake.py:506-517, 587-593.  Results arrive in groups of
    labels (Engine.run_labels hands them over as the groups finish on the GPU): `add` consolidates the paths of a group's
    components, `finish` merges the components of every original label.  Nothing here loops over components in Python: with
    twenty volumes in flight the lanes reach this point together and every millisecond of interpreter time is paid twenty times
    in a row (0.8 s of a 7.8 s round before this form)."""

    def __init__(self, shape, anisotropy, remapping):
        self.shape = shape
        self.remapping = remapping
        self.an = np.asarray(anisotropy, dtype=np.float32)
        an = self.an
        self.transform = np.array([[an[0], 0, 0, 0], [0, an[1], 0, 0], [0, 0, an[2], 0]], dtype=np.float32)
        self.skeletons = defaultdict(list)       # original label -> [(component id, verts, edges, radii)]: per-component hand-over (tests)
        self.groups = []                         # (component ids of the group's slots, consolidate_paths_flat of the group)

    def add(self, res):
        flat = consolidate_paths_flat(res, self.shape)
        if flat is not None:
            self.groups.append((np.asarray(res["tasks"]["segid"], dtype=np.int64), flat))

    def _parts(self):
        """the components that have edges (Skeleton.empty() ones are dropped, intake.py:506), in arrival order, as arrays: component
        id, original label (as a code into `labels`), and where their vertices / edges lie in the concatenated arrays"""
        seg, v0, nv, e0, ne, Vs, Rs, Es = [], [], [], [], [], [], [], []
        vbase = ebase = 0
        for segids, f in self.groups:
            cnt_e = np.diff(f["estart"])
            keep = np.flatnonzero(cnt_e > 0)
            seg.append(segids[keep])
            v0.append(f["vstart"][keep] + vbase)
            nv.append(np.diff(f["vstart"])[keep])
            e0.append(f["estart"][keep] + ebase)
            ne.append(cnt_e[keep])
            Vs.append(f["verts"]); Rs.append(f["radii"]); Es.append(f["edges"])
            vbase += f["verts"].shape[0]
            ebase += f["edges"].shape[0]
        for orig, parts in self.skeletons.items():            # (hand-over per component: the same arrays, one part at a time)
            for comp, verts, edges, radii in parts:
                if edges.shape[0] == 0:
                    continue
                seg.append(np.array([-1 - len(self._extra)], dtype=np.int64))
                self._extra.append((orig, comp))
                v0.append(np.array([vbase])); nv.append(np.array([verts.shape[0]]))
                e0.append(np.array([ebase])); ne.append(np.array([edges.shape[0]]))
                Vs.append(np.asarray(verts, dtype=np.float32)); Rs.append(np.asarray(radii, dtype=np.float32))
                Es.append(np.asarray(edges, dtype=np.uint32))
                vbase += verts.shape[0]
                ebase += edges.shape[0]
        if not seg:
            return None
        cat = lambda xs, dt: np.concatenate(xs).astype(dt, copy=False)
        return (cat(seg, np.int64), cat(v0, np.int64), cat(nv, np.int64), cat(e0, np.int64), cat(ne, np.int64),
                np.concatenate(Vs), np.concatenate(Rs), np.concatenate(Es))

    def finish(self):
        """one Skeleton per original label, in the order in which the labels' first components arrived.  The components of a
        label are disjoint voxel sets, so Skeleton.simple_merge(...).consolidate() (intake.py:587-593) is a concatenation
        re-sorted lexicographically by vertex: done on integer keys for all labels in ONE native call outside the interpreter
        (kh_host_merge_components; same result as np.unique(vertices, axis=0) + edge remap per label)."""
        import ctypes as C
        from . import _abi
        sx, sy, sz = self.shape
        self._extra = []
        got = self._parts()
        if got is None:
            return {}
        seg, v0, nv, e0, ne, Vall, Rall, Eall = got
        # original label of every part, as a code; the dict of component ids is read once, not once per component
        keys = np.fromiter(self.remapping.keys(), dtype=np.int64, count=len(self.remapping)) if len(self.remapping) else np.zeros(0, np.int64)
        vals = list(self.remapping.values())
        comp_of = seg.copy()
        label_objs = []
        code_of_obj = {}
        if keys.size:
            ks = np.argsort(keys, kind="stable")
            pos = np.searchsorted(keys[ks], np.maximum(seg, 0))
            pos = np.minimum(pos, keys.size - 1)
            idx_in_vals = ks[pos]
        else:
            idx_in_vals = np.zeros(seg.size, dtype=np.int64)
        # code per distinct original label VALUE (several component ids map to one label)
        val_code = np.empty(len(vals), dtype=np.int64)
        for i, v in enumerate(vals):
            c = code_of_obj.get(v)
            if c is None:
                c = code_of_obj[v] = len(label_objs)
                label_objs.append(v)
            val_code[i] = c
        code = val_code[idx_in_vals] if len(vals) else np.zeros(seg.size, dtype=np.int64)
        for j in np.flatnonzero(seg < 0):                       # per-component hand-over: (label, component id) given directly
            orig, comp = self._extra[-1 - int(seg[j])]
            c = code_of_obj.get(orig)
            if c is None:
                c = code_of_obj[orig] = len(label_objs)
                label_objs.append(orig)
            code[j] = c
            comp_of[j] = comp
        ucode, first_idx = np.unique(code, return_index=True)
        label_order = ucode[np.argsort(first_idx, kind="stable")]                # labels by first arrival
        rank_of_code = np.empty(len(label_objs), dtype=np.int64)
        rank_of_code[label_order] = np.arange(label_order.size)
        order = np.lexsort((comp_of, rank_of_code[code]))                        # label by label, components by id (intake.py:444)
        nvs, nes = nv[order], ne[order]
        V = np.ascontiguousarray(Vall[_ranges(v0[order], nvs)], dtype=np.float32)
        R = np.ascontiguousarray(Rall[_ranges(v0[order], nvs)], dtype=np.float32)
        E = np.ascontiguousarray(Eall[_ranges(e0[order], nes)], dtype=np.uint32)
        vstart = np.concatenate([[0], np.cumsum(nvs)]).astype(np.int64)
        estart = np.concatenate([[0], np.cumsum(nes)]).astype(np.int64)
        pol = np.concatenate([[0], np.cumsum(np.bincount(rank_of_code[code], minlength=label_order.size))]).astype(np.int64)
        oV, oR, oE = np.empty_like(V), np.empty_like(R), np.empty_like(E)
        P = lambda a: a.ctypes.data_as(C.c_void_p)
        if _abi.lib().kh_host_merge_components(int(label_order.size), P(pol), P(vstart), P(estart), P(V), P(R), P(E), int(sy), int(sz),
                                               np.float32(self.an[0]), np.float32(self.an[1]), np.float32(self.an[2]),
                                               P(oV), P(oR), P(oE)) != 0:
            raise MemoryError("kh_host_merge_components failed")
        merged = {}
        va, ea = vstart[pol].tolist(), estart[pol].tolist()       # first vertex / edge of every label
        wrap, tf = Skeleton.wrap, self.transform
        for li, c in enumerate(label_order.tolist()):
            # copies: the public arrays own their memory (a kept Skeleton does not pin the volume's buffers)
            a, b, e0_, e1_ = va[li], va[li + 1], ea[li], ea[li + 1]
            merged[label_objs[c]] = wrap(oV[a:b].copy(), oE[e0_:e1_].copy(), oR[a:b].copy(), label_objs[c], tf.copy(), "physical")
        return merged


def assemble(res, shape, anisotropy, remapping):
    asm = Assembler(shape, anisotropy, remapping)
    asm.add(res)
    return asm.finish()
