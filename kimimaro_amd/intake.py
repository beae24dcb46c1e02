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
import time

from collections import defaultdict

import numpy as np

from . import _abi, ops, points
from .border import compute_border_targets
from .engine import Engine, NONE32
from .plan import LabelSet
from .skeleton import Skeleton
# what moved to modules of its own stays importable from here
from .assemble import (Assembler, assemble, consolidate_paths, consolidate_paths_batch, consolidate_paths_flat,  # noqa: F401
                       consolidate_paths_flat_numpy, paths_of)
from .avocado import _avocado_fruit_from_lines, engage_avocado_protection_device  # noqa: F401
from .holes import enclosed_regions, resolve_holes  # noqa: F401
from .trace import TRACE_DEFAULTS, point_to_point, trace as trace_one
from .volume import (DimensionError, LazyVolume, _device_labels, apply_object_mask, coords_of, format_labels,  # noqa: F401
                     last_run_starts, linear_index)

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


def compute_cc_labels(all_labels):
    """kimimaro/utility.py:58-83 -> (cc_labels uint32 F-order, N, {cc id: original id}).
    Row f1: 26-connected multi-label CCL, host C++ helper in libkimi_hip.so for now."""
    lib = _abi.lib()
    lab = all_labels
    if lab.dtype.kind not in "ui" or lab.dtype.itemsize not in (1, 2, 4, 8):
        lab = lab.astype(np.uint64)
    lab = np.asfortranarray(lab)
    cc = np.zeros(lab.shape, dtype=np.uint32, order="F")
    n = lib.kh_host_ccl26(_abi.np_ptr(lab), lab.dtype.itemsize, lab.shape[0], lab.shape[1], lab.shape[2], _abi.np_ptr(cc))
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
    if d_graph is not None and n:
        # a graph joins voxels whatever their labels: the voxel get_mapping reads then decides the name -- the component's LAST run
        # start in the raster.  (Without a graph a component holds one label and its representative voxel says the same.)
        t = eng.torch
        rep = last_run_starts(t, d_cc.to(t.int64) & 0xFFFFFFFF, n).cpu().numpy()
    orig = all_labels.reshape(-1, order="F")[rep[1:].astype(np.int64)] if n else []
    remap = {i + 1: orig[i].item() for i in range(n)}  # skeletontricks.get_mapping :490-525
    return d_cc, n, remap


def _points_to_labels(pts, cc_labels):
    mapping = defaultdict(list)
    for pt in pts:
        pt = tuple(int(v) for v in pt)
        mapping[int(cc_labels[pt])].append(pt)
    return mapping


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
        d_graph = eng.graph_to_device(voxel_graph, all_labels.shape)
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
    # A target belongs to the component that holds its voxel when tracing starts: the points are mapped AFTER the avocado pass.
    # The reference maps them before it (kimimaro/intake.py:171-172) on ids the pass then merges and renumbers (:187); that order
    # is NOT reproduced: a target inside a pit is dropped, and one whose old id is reused lands on another label, off its crop
    # (DESIGN.md section 4).  After fill_holes, as there (:168-172).
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


def synapse_queries(synapses, span, itemsize):
    """The queries of synapses_to_targets for a volume whose dtype holds `span` in `itemsize` bytes -> (groups, words, query_start,
    centroids), None when no label is left.  groups: per entry of `synapses`, in its order, (word, {swc label: [centroids]}) with the
    swc labels in first-seen order (intake.py:735-737), None for a label the dtype cannot hold, one without pairs and a repeated
    word; words: u64, the distinct words ascending; query_start: u32 [len(words) + 1]; centroids: f64 [Q, 3], the queries of
    words[k] at rows [query_start[k], query_start[k + 1]), swc label after swc label."""
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
        return None
    words = np.array(sorted(by_word), dtype=np.uint64)
    counts = [sum(len(c) for c in groups[by_word[int(w)]][1].values()) for w in words]
    query_start = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)
    centroids = np.concatenate([np.stack(c) for w in words for c in groups[by_word[int(w)]][1].values()])
    return groups, words, query_start, centroids


def synapse_targets(groups, words, query_start, winners, sy, sz):
    """{(x, y, z): swc_label} from the winners (u64 [Q]: C-order indices x*sy*sz + y*sz + z, points.NONE64 where the label does not
    occur) of the queries of synapse_queries, in the reference's insertion and overwrite order"""
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
    eng = ops.engine()                                   # raises HipUnavailableError without the library or a gfx950 device
    d_flat, itemsize, _, shape, _, span = _device_labels(eng, labels)
    queries = synapse_queries(synapses, span, itemsize)
    if queries is None:
        return {}
    groups, words, query_start, centroids = queries
    winners = points.nearest_label_voxels(eng, d_flat, itemsize, shape, words, query_start, centroids)
    return synapse_targets(groups, words, query_start, winners, shape[1], shape[2])


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

    eng = ops.engine()                                   # raises HipUnavailableError without the library or a gfx950 device
    d_cc, _, _ = compute_cc_labels_device(eng, labels)
    cc = LazyVolume(eng, d_cc, labels.shape)
    if cc[start] == 0 or cc[start] != cc[end]:
        raise ValueError("Cannot extract centerline from disconnected components.")
    del cc, d_cc

    skel = point_to_point(labels, start, end, anisotropy=anisotropy, pdrf_scale=pdrf_scale, pdrf_exponent=pdrf_exponent)
    skel.vertices *= anisotropy
    skel.space = "physical"
    return skel


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
    eng = ops.engine()                                   # raises HipUnavailableError without the library or a gfx950 device
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
    def _mark(name):
        if timings is not None:
            eng.sync_stream()
            timings.append((name, time.perf_counter()))

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
            mtb = [linear_index(p, shape) for p in border_targets[segid]]
            root = mtb.pop()
        if segid in before and len(before[segid]) > 0:
            mtb.extend(linear_index(p, shape) for p in before[segid])
        if segid in after and len(after[segid]) > 0:
            mta.extend(linear_index(p, shape) for p in after[segid])
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
    an = np.asarray(anisotropy, dtype=np.float32)
    kw = {k: params[k] for k in ("scale", "const", "pdrf_scale", "pdrf_exponent", "soma_detection_threshold",
                                 "soma_acceptance_threshold", "soma_invalidation_scale", "soma_invalidation_const")}

    def one(e, i):
        segid, root, mtb, mta = jobs[i]
        lo, hi = bbox(segid)
        minpt = np.array(lo, dtype=np.int64)
        labels = e.crop(d_cc, shape, lo, hi) == segid
        dbf = np.where(labels, e.crop(d_dbf, shape, lo, hi, np.float32), 0.0).astype(np.float32)
        tr = lambda ls: [tuple(int(v) for v in pt) for pt in coords_of(ls, shape) - minpt]
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
