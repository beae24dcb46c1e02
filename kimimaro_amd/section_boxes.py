"""Cross sections for a dataset that is never resident as a whole, on the plumbing of kimimaro_amd.boxes (every public name is
kimimaro_amd.post's too):

    cross_sectional_area_chunked(dataset, skeletons, chunk_shape, halo)  the skeletons' sections, the dataset in boxes
    cross_sectional_area_filled_chunked(dataset, skeletons, ...)         the same of the filled labels, on
    region_graph_chunked(dataset, chunk_shape, region_store)             the region graph of a dataset from its cores, and hole_lists
    fill_all_holes_chunked(dataset, chunk_shape, out, region_store)      the holes of every label of the dataset filled
"""
import time
from collections import namedtuple

import numpy as np

from . import _abi, ops, section, utility
from .boxes import (_load_box, _slices, axes, count_core, count_core_device, down, group_by_core, label_table, label_type,
                    store_like, up, upload_labels)
from .holes import enclosed_regions, resolve_holes
from .plan import core_of, halo_boxes
from .volume import _device_labels, ranges

XS_CLIPPED = 64          # cross_sectional_area_contacts: the section was still clipped by the largest box that could be loaded


def _xs_box_budget(eng, itemsize, region_bytes=0):
    """The default max_box_voxels: what the free HBM pays for.  While a box is resident a voxel costs the label itself and, in round
    0, the copy of the core that is counted (2 x itemsize); labels of eight bytes are renumbered per box (utility._narrow_labels:
    torch.unique with its inverse -- the sorted copy, the permutation, the inverse and the shifted ids at 8 bytes each, the u32 ids,
    a mask: 56 bytes with the volume).  region_bytes: what else a voxel costs (cross_sectional_area_filled_chunked: 4, the box of
    the region store).  Kept back: the kernel's scratch (section.SCRATCH_BUDGET) and 1 GiB for the 2^24-voxel pieces of the count."""
    free = int(eng.torch.cuda.mem_get_info(eng.device)[0])
    return max(0, (free - section.SCRATCH_BUDGET - (1 << 30)) // ((2 * itemsize if itemsize < 8 else 56) + region_bytes))


# ---------------------------------------------------------------------------------------------------------------
RegionGraph = namedtuple("RegionGraph", "store value face pairs bases member_offsets members info")


def _merge_regions(value, face, core_pairs, seam_keys):
    """The host merge of region_graph_chunked on provisional ids 1..N (value u64, face u8: [N + 1]; core_pairs: the cores' adjacency
    keys in provisional ids; seam_keys: low << 32 | high of every cross-cut pair).  A seam pair of equal value joins two pieces of one
    region (union-find, numpy: roots are hooked to the smaller root and the forest is flattened, until every pair agrees), one of
    unequal value is an adjacency.  -> (merged u32 [N + 1]: the merged id 1..G of a provisional id, value, face [G + 1], pairs)"""
    n = int(value.size) - 1
    low, high = seam_keys >> np.uint64(32), seam_keys & np.uint64(0xFFFFFFFF)
    same = value[low] == value[high]
    joined, index = np.unique(np.concatenate([low[same], high[same]]), return_inverse=True)      # union-find on the ids that occur
    index = np.asarray(index).reshape(-1)
    a, b = index[:index.size // 2], index[index.size // 2:]
    parent = np.arange(joined.size, dtype=np.int64)
    while True:
        ra, rb = parent[a], parent[b]
        apart = ra != rb
        if not apart.any():
            break
        ra, rb = ra[apart], rb[apart]
        small = np.minimum(ra, rb)
        np.minimum.at(parent, ra, small)
        np.minimum.at(parent, rb, small)
        while True:
            above = parent[parent]
            if np.array_equal(above, parent):
                break
            parent = above
    root = np.arange(n + 1, dtype=np.int64)
    root[joined.astype(np.int64)] = joined[parent].astype(np.int64)
    roots, merged = np.unique(root[1:], return_inverse=True)
    merged = np.concatenate([np.zeros(1, dtype=np.int64), np.asarray(merged).reshape(-1) + 1])
    g = int(roots.size)
    m_value = np.zeros(g + 1, dtype=np.uint64)
    m_value[merged] = value                                                 # (all members carry one value)
    m_face = (np.bincount(merged[1:], weights=face[1:], minlength=g + 1) > 0).astype(np.uint8)
    keys = np.concatenate([core_pairs, seam_keys[~same]])
    p, q = merged[(keys >> np.uint64(32)).astype(np.int64)], merged[(keys & np.uint64(0xFFFFFFFF)).astype(np.int64)]
    assert np.all(p != q), "region_graph_chunked: a pair joins a merged region with itself"
    pairs = np.unique((np.minimum(p, q).astype(np.uint64) << np.uint64(32)) | np.maximum(p, q).astype(np.uint64))
    return merged.astype(np.uint32), m_value, m_face, pairs


def hole_lists(graph, words):
    """hole(L) on a RegionGraph for each of the label words `words` (the unsigned words the dataset's dtype holds): per word the
    u32 PROVISIONAL ids of its hole regions, ascending -- kh_host_enclosed_regions on the merged graph, every merged region
    replaced by its members.  The ids of one core are one range (graph.bases), so a box's share of a list is a filter."""
    offsets, regions = enclosed_regions(graph.value, graph.face, graph.pairs, np.array(list(words), dtype=np.uint64))
    out = []
    for i in range(len(offsets) - 1):
        mine = regions[int(offsets[i]):int(offsets[i + 1])].astype(np.int64)
        first = graph.member_offsets[mine]
        out.append(np.sort(graph.members[ranges(first, graph.member_offsets[mine + 1] - first)]))
    return out


def region_graph_chunked(dataset, chunk_shape=(512, 512, 512), region_store=None, timings=None, _regions=None, face_axes=3,
                         return_counts=False):
    """The region graph (the 6-connected components of equal value, 0 included, and which of them share a voxel face)
    of a dataset that is never resident as a whole, from one sweep over the cores of plan.halo_boxes(shape, chunk_shape, 0) in raster
    order.  A core is loaded, uploaded as it is (1, 2, 4 or 8 bytes per label; bool as bytes) and handed to
    Engine.region_graph with the mask of its faces that are faces of the DATASET (kh_region_table_box); its region r gets the
    PROVISIONAL id base_k + r, base_k = the regions of all earlier cores.  The provisional ids go, per voxel, into the region store.
    For each axis on which the core has a lower neighbour its lowest plane of ids is paired with the facing plane of the store
    (kh_region_seam_pairs).  The host then joins the pieces that a seam pair of equal value connects (numpy union-find) into the
    merged regions 1..G.

    region_store: an array-like of the dataset's shape (three axes), u32, indexed [x, y, z], read and written by slices only --
    e.g. an np.memmap; default: a numpy array in host memory.  It costs 4 BYTES PER VOXEL OF THE DATASET.  Id 0 never occurs.
    Returns RegionGraph(store; value u64, face u8: [G + 1], entry 0 unused, face = the region owns a voxel on a face of the dataset,
    an axis of extent 1 putting every voxel on one; pairs: u64, smaller merged id << 32 | larger, each once; bases: int64
    [cores + 1], core k owns the provisional ids bases[k] + 1 .. bases[k + 1]; member_offsets, members: the provisional ids of merged
    region g are members[member_offsets[g] : member_offsets[g + 1]], ascending; info: the figures `timings` receives).
    ValueError for 2^32 regions or more in all.
    timings (a dict) receives regions_s (the sweep: loading, upload, Engine.region_graph, the store), seam_ms (of that, the seams:
    host milliseconds around the upload of the store's plane, the kernel and the download of its keys), merge_s, provisional_regions,
    merged_regions, seam_pairs (distinct cross-cut pairs) and cores.
    _regions: a function with Engine.region_graph's contract on a HOST array -- _regions(core [x, y, z], label_bytes, shape, 3,
    mark, faces) -> (region ids 1..R per voxel as an array of that shape, value, count, face, pairs, info) -- that runs instead of
    the engine; the seams are then made by numpy and nothing touches the GPU (the host-logic tests).
    face_axes: the leading axes whose two ends are faces of the dataset.  3 (default): all of them, an axis of extent 1 putting every
    voxel on a face; 2: the dataset is a 2-D image (fill_all_holes_chunked) and the ends of its unit z axis are none.
    return_counts=True: -> (RegionGraph, count: int64 [G + 1], the voxels of every merged region, its pieces summed in 64 bits)."""
    shape0, shape, extent = axes(dataset, "region_graph_chunked")
    core_lo, core_hi, _, _ = halo_boxes(shape0, chunk_shape, 0)
    eng = ops.engine() if _regions is None else None
    store = store_like(region_store, shape, np.uint32, "region_store", "u32", zeros=True)
    bases = np.zeros(core_lo.shape[0] + 1, dtype=np.int64)
    values, faces, core_pairs, seams = [np.zeros(1, dtype=np.uint64)], [np.zeros(1, dtype=np.uint8)], [], []
    counts = [np.zeros(1, dtype=np.int64)]
    seam_ms, base = 0.0, 0
    t0 = time.perf_counter()
    for k in range(core_lo.shape[0]):                                       # raster order (x fastest): a lower neighbour comes first
        lo, hi = core_lo[k], core_hi[k]
        ext = tuple(int(v) for v in hi - lo)
        host = _load_box(dataset, lo, hi, "region_graph_chunked")
        if label_type(host)[1]:
            host = host.view(np.uint8)
        with_faces = range(int(face_axes))
        on_face = sum(1 << (2 * a) for a in with_faces if lo[a] == 0) | sum(2 << (2 * a) for a in with_faces if hi[a] == extent[a])
        if eng is None:
            region, value, count, face, pairs, _ = _regions(host, host.dtype.itemsize, ext, 3, lambda name: None, on_face)
            region = np.asarray(region).reshape(ext, order="F")
        else:
            d_flat, itemsize, _, _, _, _ = _device_labels(eng, host)
            region, value, count, face, pairs, _ = eng.region_graph(d_flat, itemsize, ext, 3, faces=on_face)
        n_regions = int(value.size) - 1
        if base + n_regions >= 2 ** 32:
            raise ValueError("region_graph_chunked: fewer than 2^32 regions in all (core {} ends at {})".format(k, base + n_regions))
        if eng is None:
            ids = (region.astype(np.int64) + base).astype(np.uint32)
        else:
            d_ids = region + (base - 2 ** 32 if base >= 2 ** 31 else base)  # (u32 words in an int32 tensor: the sum wraps)
            ids = down(d_ids, ext).view(np.uint32)
        store[_slices(lo, hi)] = ids
        values.append(value[1:])
        faces.append(face[1:])
        counts.append(np.asarray(count[1:], dtype=np.int64))
        shift = np.uint64(base)
        core_pairs.append((((pairs >> np.uint64(32)) + shift) << np.uint64(32)) | ((pairs & np.uint64(0xFFFFFFFF)) + shift))
        t1 = time.perf_counter()
        for axis in range(3):
            if lo[axis] == 0:
                continue
            below, top = lo.copy(), hi.copy()                               # the facing plane of the lower neighbour, out of the store
            below[axis], top[axis] = lo[axis] - 1, lo[axis]
            low = np.take(_load_box(store, below, top), 0, axis=axis)
            if eng is None:
                high = np.take(ids, 0, axis=axis)
                keys = np.unique((low.astype(np.uint64) << np.uint64(32)) | high.astype(np.uint64))
            else:
                cube = d_ids.view(ext[2], ext[1], ext[0])                   # (the device array is Fortran ordered: [z, y, x] here)
                d_high = cube.select(2 - axis, 0).contiguous().view(-1)
                keys, _, _ = eng.region_seam_pairs(up(eng, low), d_high)
            seams.append(keys)
        seam_ms += (time.perf_counter() - t1) * 1e3
        base += n_regions
        bases[k + 1] = base
    regions_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    cat = lambda parts, dtype: np.concatenate(parts) if parts else np.zeros(0, dtype=dtype)
    seam_keys = cat(seams, np.uint64)
    merged, value, face, pairs = _merge_regions(np.concatenate(values), np.concatenate(faces), cat(core_pairs, np.uint64), seam_keys)
    by_region = np.argsort(merged[1:], kind="stable").astype(np.uint32) + np.uint32(1)
    member_offsets = np.concatenate([np.zeros(2, dtype=np.int64), np.cumsum(np.bincount(merged[1:], minlength=value.size)[1:])])
    merge_s = time.perf_counter() - t0
    info = dict(regions_s=regions_s, seam_ms=seam_ms, merge_s=merge_s, provisional_regions=int(base), merged_regions=int(value.size) - 1,
                seam_pairs=int(seam_keys.size), cores=int(core_lo.shape[0]))
    if timings is not None:
        timings.update(info)
    graph = RegionGraph(store, value, face, pairs, bases, member_offsets, by_region, info)
    if not return_counts:
        return graph
    count = np.zeros(value.size, dtype=np.int64)
    np.add.at(count, merged[1:].astype(np.int64), np.concatenate(counts)[1:])
    return graph, count


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


def fill_all_holes_chunked(dataset, chunk_shape=(512, 512, 512), out=None, region_store=None, return_fill_count=False, progress=False,
                           stats=None, _regions=None, _apply=None):
    """kimimaro_amd.intake.fill_all_holes for a dataset that is never resident as a whole.  The result is DEFINED as
    what fill_all_holes(whole dataset) returns: the volume voxel for voxel, the fill count (a voxel filled twice counts twice) and
    the verdict per label.  hole(L) is taken on the DATASET: a cavity that a cut between two cores runs through is filled when it is
    closed in the dataset, and one that is closed in a core's view but joined to a face of the dataset through another core is not.
    The labels take their turn in ascending order of their VALUES, as the unsigned words the dataset holds; values need not be
    dense, nor need a value be connected.

    dataset: what the other box drivers take -- a numpy array of any order, an np.memmap, a tensor on the GPU, anything with .shape
      and slicing; two or three axes; integers of 1, 2, 4 or 8 bytes or bool; 2^32 voxels or more are fine, only a core has to stay
      below that.  Two axes are a 2-D image, as fill_all_holes fills a 2-D array: its border is its outline.  A three-axis dataset
      with an axis of extent 1 has every voxel on a face and no holes.
    out: None -- the dataset is modified in place and returned, and only the cores that hold a painted voxel are written; or an
      array-like of the dataset's shape and dtype, written by slices -- every core is written, painted or copied, the dataset is
      left alone and `out` is returned.  ValueError for another shape or dtype.
    region_store: region_graph_chunked's -- 4 BYTES PER VOXEL OF THE DATASET, in host memory by default.
    return_fill_count: return (volume, N).  progress: accepted, no effect.

    Two sweeps over the cores of plan.halo_boxes(shape, chunk_shape, 0).  The first is region_graph_chunked with its counts: the
    region graph of the dataset over the cuts.  kh_host_resolve_holes then decides on the merged graph who fills what, and the
    owners of the painted merged regions are handed to their provisional ids.  The second sweep visits the cores whose id range
    holds a painted id: the core and its slice of the store are uploaded, kh_region_apply_box paints, the core is written back.
    A merged region that owns a face of the dataset is never painted and its count is clamped to 2^32 - 1 (the resolver takes
    u32); one without a face that has 2^32 voxels or more is a ValueError.  KimiHipError, naming the core, when the store hands
    back an id outside the core's range (a caller's store that changed between the sweeps).
    stats (a dict) receives region_graph_chunked's figures, labels, label_value / label_state (the verdict per label, _abi.HOLES_*
    bits), filled, resolve_ms, apply_s (the second sweep), cores_painted and cores.
    _regions: region_graph_chunked's; _apply(core, ids, base, owner) -> (the painted core, voxels painted) on host arrays -- the core
    as unsigned words [x, y, z], its u32 ids, the core's first id - 1 and the owners u64 of base .. base + regions (entry 0 unused).
    The two come together, and with them nothing touches the GPU (the host-logic tests).  Without them there is no CPU fallback:
    HipUnavailableError without the library or an MI355X."""
    name = "fill_all_holes_chunked"
    if (_regions is None) != (_apply is None):
        raise ValueError("{}: _regions and _apply come together".format(name))
    eng = ops.engine() if _apply is None else None       # raises HipUnavailableError without the library or a gfx950 device
    shape0, shape, extent = axes(dataset, name)
    dtype, is_bool, _ = label_type(dataset)
    word = np.dtype("u%d" % dtype.itemsize)
    if out is not None:
        try:
            same = np.dtype(out.dtype) == dtype
        except TypeError:                                # (a tensor's dtype)
            same = str(out.dtype).split(".")[-1] == dtype.name
        if tuple(int(v) for v in out.shape) != shape0 or not same:
            raise ValueError("{}: out of shape {} and dtype {}. Got: {} of shape {}".format(name, shape0, dtype, out.dtype, tuple(out.shape)))
    target = dataset if out is None else out
    core_lo, core_hi, _, _ = halo_boxes(shape0, chunk_shape, 0)
    info = {}
    graph, count = region_graph_chunked(dataset, chunk_shape, region_store, info, _regions, face_axes=len(shape0), return_counts=True)

    t0 = time.perf_counter()
    big = count >= 2 ** 32
    if np.any(big & (graph.face == 0)):
        g = int(np.flatnonzero(big & (graph.face == 0))[0])
        raise ValueError("{}: the region of value {} that touches no face of the dataset has {} voxels; fewer than 2^32 can be "
                         "resolved".format(name, int(graph.value[g]), int(count[g])))
    owner, label_value, label_state, filled = resolve_holes(graph.value, np.minimum(count, 2 ** 32 - 1).astype(np.uint32), graph.face,
                                                            graph.pairs)
    painted_regions = np.flatnonzero(owner)                                # merged ids -> the provisional ids of their pieces
    first = graph.member_offsets[painted_regions]
    pieces = graph.member_offsets[painted_regions + 1] - first
    painted_ids = graph.members[ranges(first, pieces)].astype(np.int64)
    owner_of = np.zeros(int(graph.bases[-1]) + 1, dtype=np.uint64)
    owner_of[painted_ids] = np.repeat(owner[painted_regions], pieces)
    visit = np.zeros(core_lo.shape[0], dtype=bool)
    visit[np.searchsorted(graph.bases, painted_ids, side="left") - 1] = True   # core k owns bases[k] + 1 .. bases[k + 1]
    expected = int(count[painted_regions].sum())
    resolve_ms = (time.perf_counter() - t0) * 1e3

    t0 = time.perf_counter()
    painted = 0
    for k in range(core_lo.shape[0]):
        lo, hi = core_lo[k], core_hi[k]
        if not visit[k]:
            if out is not None:
                _store_box(out, lo, hi, _load_box(dataset, lo, hi, name))
            continue
        ext = tuple(int(v) for v in hi - lo)
        core = np.asfortranarray(_load_box(dataset, lo, hi, name)).view(word)
        ids = _load_box(graph.store, lo, hi)
        base = int(graph.bases[k])
        mine = owner_of[base:int(graph.bases[k + 1]) + 1].copy()
        mine[0] = 0
        if eng is None:
            core, n = _apply(core, ids, base, mine)
            core = np.asarray(core)
        else:
            d_lab = eng.to_device(core)
            n, strangers = eng.region_apply_box(up(eng, ids), base, eng.torch.from_numpy(mine.view(np.int64)).to(eng.device), d_lab,
                                                word.itemsize)
            if strangers:
                raise _abi.KimiHipError("{}: core {} ([{}:{}]): {} voxels of the region store carry an id outside the core's range "
                                        "{}..{}; the store changed between the sweeps".format(
                                            name, k, [int(v) for v in lo], [int(v) for v in hi], strangers, base + 1, int(graph.bases[k + 1])))
            core = d_lab.cpu().numpy().view(word).reshape(ext, order="F")
        painted += int(n)
        _store_box(target, lo, hi, core.view(dtype))
    if painted != expected:
        raise _abi.KimiHipError("{}: {} voxels painted, {} in the painted regions; the store changed between the sweeps".format(
            name, painted, expected))
    if stats is not None:
        stats.update(info, labels=int(label_value.size), label_value=label_value, label_state=label_state, filled=int(filled),
                     resolve_ms=resolve_ms, apply_s=time.perf_counter() - t0, cores_painted=int(visit.sum()), cores=int(core_lo.shape[0]))
    return (target, int(filled)) if return_fill_count else target


def cross_sectional_area_chunked(dataset, skeletons, chunk_shape=(512, 512, 512), halo=64, anisotropy=(1, 1, 1), smoothing_window=1,
                                 step=1, multipass=False, repair_contacts=False, max_box_voxels=None, progress=False, timings=None,
                                 fill_holes=False, visualize_section_planes=False, _sections=None):
    """kimimaro_amd.cross_sectional_area for a dataset that is never resident as a whole: the other half of what
    igneous does around kimimaro.  The result is DEFINED as what cross_sectional_area(whole dataset, skeletons, ...) returns, bit for
    bit in cross_sectional_area and equal in cross_sectional_area_contacts (whose bits name the faces of the DATASET), wherever a
    box large enough could be loaded; the dataset may hold 2^32 voxels or more, which cross_sectional_area refuses.

    dataset: what skeletonize_chunked takes.  skeletons: a dict, a list or one Skeleton, vertices in DATASET coordinates (what
    skeletonize_chunked returns); changed in place and returned.  anisotropy, smoothing_window, step, multipass, repair_contacts,
    the attributes, the extra_attributes entries and the skip rules: cross_sectional_area's.

    The (vertex, normal) pairs are made once from the whole skeletons, so a path that crosses a cut has the normals of an unchunked
    run.  The cores of plan.halo_boxes(dataset.shape, chunk_shape, halo) partition the dataset.  Round 0 visits every core once,
    loads its box (the core widened by `halo` voxels, clamped), counts the skeletons' labels in the core and runs the sections whose
    vertex lies in the core in one launch (kh_cross_sections_box).  A section that reached a face of its box that is a cut through
    the dataset (clip != 0) is run again in round r = 1, 2, ... in the box of its core at halo * 2^r, those sections alone, until
    none is clipped: a box equal to the dataset clips nothing.  Boxes run one after the other on one engine.

    max_box_voxels: the largest box that is loaded (default: sized from the free HBM, _xs_box_budget); never 2^32 - 1 voxels or more.
    A section whose next box would exceed it keeps its last values and gets bit 64 in cross_sectional_area_contacts: "clipped by
    the largest box tried, the area may be an underestimate" (bits 1..32 keep cross_sectional_area's meaning).  ValueError when
    a box of round 0 does not fit already, and for halo < 1.
    Where cross_sectional_area launches again (a vertex whose area came back 0 and that occurs again on another path), the boxes
    start again at `halo`.  fill_holes=True raises NotImplementedError here: cross_sectional_area_filled_chunked is that option.
    visualize_section_planes=True raises NotImplementedError too; progress: no effect.
    timings (a dict) receives calls (per launch of the driver loop a dict of `boxes` loaded and `items` run, one entry per growth
    round), cores, boxes_loaded, voxels_loaded, items (round 0), items_rerun (growth rounds), capped_items, kernel_ms (HIP events),
    load_s (host: loading, upload, counting), and rounds, vertices, occurrences of the driver loop.
    _sections: a function with the signature of section.cross_sections_box that runs the boxes instead; it is handed the box as the
    host array and the labels themselves as words, and nothing here touches the GPU (the host-logic tests).  Without it there is no
    CPU fallback: HipUnavailableError without the library or an MI355X."""
    utility._xs_check_arguments(step, smoothing_window, visualize_section_planes)
    if fill_holes:
        raise NotImplementedError("cross_sectional_area_chunked(fill_holes=True) keeps raising at this entry point; the sections of "
                                  "filled labels of a dataset in boxes are cross_sectional_area_filled_chunked, which takes the same "
                                  "arguments and a region_store")
    return _xs_chunked("cross_sectional_area_chunked", False, None, dataset, skeletons, chunk_shape, halo, anisotropy, smoothing_window,
                       step, multipass, repair_contacts, max_box_voxels, timings, _sections, None)


def cross_sectional_area_filled_chunked(dataset, skeletons, chunk_shape=(512, 512, 512), halo=64, anisotropy=(1, 1, 1),
                                        smoothing_window=1, step=1, multipass=False, repair_contacts=False, max_box_voxels=None,
                                        progress=False, timings=None, visualize_section_planes=False, region_store=None,
                                        _sections=None, _regions=None):
    """kimimaro_amd.cross_sectional_area_filled for a dataset that is never resident as a whole: the result is DEFINED
    as what cross_sectional_area_filled(whole dataset, skeletons, ...) returns -- bit for bit in cross_sectional_area, equal in
    cross_sectional_area_contacts -- wherever a box large enough could be loaded.  hole(L) is taken on the DATASET: a cavity that
    reaches a cut between two cores is a hole if it is closed in the dataset, and one that is closed in a core's view but joined to
    a face of the dataset through another core is none.  A dataset with an axis of extent 1 has no holes.

    Every argument, the rounds, the growth of the boxes, bit 64 and the skip rules (which count the label as given) are
    cross_sectional_area_chunked's.  In front of the boxes one more sweep over the cores builds the region graph of the dataset
    (region_graph_chunked; only when a skeleton has a label) and kh_host_enclosed_regions lists hole(L) for the skeletons' labels;
    every box then loads its slice of the region store beside its labels and runs kh_cross_sections_filled_box with the lists cut
    down to the cores the box intersects.  A vertex in a hole voxel of its label is a valid seed, in a box that holds no voxel of
    the label too.

    region_store: where the region id of every voxel is kept between the sweep and the boxes: an array-like of the dataset's shape
    (three axes), u32, indexed [x, y, z], read and written by slices -- an np.memmap, say.  Default: a numpy array in host memory.
    Either way it costs 4 BYTES PER VOXEL OF THE DATASET.  max_box_voxels' default counts 4 more bytes per voxel, the region box.
    timings receives cross_sectional_area_chunked's entries and regions_s, seam_ms, merge_s, provisional_regions, merged_regions,
    seam_pairs (region_graph_chunked), enclosed_ms (the host search) and listed_ids (hole regions over all labels, provisional ids).
    _sections: a function with the signature of section.cross_sections_filled_box, handed the box and its region box as host arrays
    [x, y, z], the labels themselves as words and the lists as a host array; _regions: region_graph_chunked's.  With both nothing
    touches the GPU (the host-logic tests).  Without them there is no CPU fallback."""
    utility._xs_check_arguments(step, smoothing_window, visualize_section_planes)
    return _xs_chunked("cross_sectional_area_filled_chunked", True, region_store, dataset, skeletons, chunk_shape, halo, anisotropy,
                       smoothing_window, step, multipass, repair_contacts, max_box_voxels, timings, _sections, _regions)


def _xs_chunked(name, filled, region_store, dataset, skeletons, chunk_shape, halo, anisotropy, smoothing_window, step, multipass,
                repair_contacts, max_box_voxels, timings, _sections, _regions):
    """the body of cross_sectional_area_chunked and cross_sectional_area_filled_chunked (filled), after the argument checks"""
    if int(halo) != halo or int(halo) < 1:
        raise ValueError("{}: halo must be a positive integer. Got: {}".format(name, halo))
    if filled and (_sections is None) != (_regions is None):
        raise ValueError("{}: _sections and _regions come together".format(name))
    eng = ops.engine() if _sections is None else None    # raises HipUnavailableError without the library or a gfx950 device
    run_sections = (section.cross_sections_filled_box if filled else section.cross_sections_box) if _sections is None else _sections
    an = utility._xs_anisotropy(anisotropy)
    an64 = an.astype(np.float64)
    shape0, shape, extent = axes(dataset, name)
    core_lo, core_hi, _, _ = halo_boxes(shape0, chunk_shape, 0)
    n_cores = int(core_lo.shape[0])
    dtype, is_bool, span = label_type(dataset)
    limit = 2 ** 32 - 2
    if max_box_voxels is None and eng is not None:
        max_box_voxels = _xs_box_budget(eng, dtype.itemsize, 4 if filled else 0)
    if max_box_voxels is not None:
        limit = min(limit, int(max_box_voxels))

    skels, labels_of, table, place = label_table(skeletons, is_bool)    # a job's word: the place of its label here
    jobs = [(s, place[L], (0, 0, 0)) for s, L in zip(skels, labels_of) if L is not None]
    kept = [(getattr(s, "cross_sectional_area", None), getattr(s, "cross_sectional_area_contacts", None)) for s, _, _ in jobs]
    counts = np.zeros(len(table), dtype=np.int64)                        # voxels per label, from the cores of the first sweep
    total = dict(calls=[], cores=n_cores, boxes_loaded=0, voxels_loaded=0, items=0, items_rerun=0, capped_items=0, load_s=0.0)
    stats, state = {}, {"counted": False}
    none = np.zeros(0, dtype=np.int64)

    graph, hole_ids = None, [np.zeros(0, dtype=np.uint32)] * len(table)  # (filled) per entry of `table`: hole(L), provisional ids
    if filled and jobs:
        graph = region_graph_chunked(dataset, chunk_shape, region_store, total, _regions)
        known = [L for L in table if span[0] <= L <= span[1]]
        t0 = time.perf_counter()
        for L, ids in zip(known, hole_lists(graph, [L % (1 << (8 * dtype.itemsize)) for L in known])):
            hole_ids[place[L]] = ids
        total["enclosed_ms"] = (time.perf_counter() - t0) * 1e3
        total["listed_ids"] = int(sum(ids.size for ids in hole_ids))

    def box_holes(lo, hi):
        """-> (per entry of `table` where its list starts and how many ids it has, the lists): hole(L) cut down to the regions of
        the cores that the box [lo, hi) intersects -- no other region has a voxel in the box"""
        meets = np.all((core_lo < hi) & (core_hi > lo), axis=1)
        parts, begin, count = [], np.zeros(len(table), dtype=np.uint32), np.zeros(len(table), dtype=np.uint32)
        for w, ids in enumerate(hole_ids):
            if ids.size:
                ids = ids[meets[np.searchsorted(graph.bases, ids, side="left") - 1]]       # core k owns bases[k] + 1 .. bases[k + 1]
                begin[w], count[w] = sum(p.size for p in parts), ids.size
                parts.append(ids)
        return begin, count, np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint32)

    def box_labels(host, lo, k, count):
        """-> (the box for run_sections, bytes per label, per entry of `table` the word it has in this box or -1)"""
        words = np.full(len(table), -1, dtype=np.int64)
        inner = _slices(core_lo[k] - lo, core_hi[k] - lo)
        if eng is None:
            for L in table:
                if span[0] <= L <= span[1]:
                    words[place[L]] = L % (1 << 32)
            if count:
                count_core(host[inner], place, counts)
            return host, host.dtype.itemsize, words
        d_lab, label_bytes, device_word = upload_labels(eng, host, span, table)
        for L, w in device_word.items():
            words[place[L]] = w
        if count:
            count_core_device(eng, d_lab, host.shape, inner, device_word, place, counts)
        return d_lab, label_bytes, words

    def run_box(k, reach, vox, wrd, nrm, count):
        """the sections (vox, wrd, nrm) in the box of core k at halo `reach` -> (area, contact, clip), None when it may not be loaded"""
        lo, hi = np.maximum(core_lo[k] - reach, 0), np.minimum(core_hi[k] + reach, extent)
        ext = tuple(int(v) for v in hi - lo)
        if ext[0] * ext[1] * ext[2] > limit:
            return None
        t0 = time.perf_counter()
        d_lab, label_bytes, words = box_labels(_load_box(dataset, lo, hi, name), lo, k, count)
        total["load_s"] += time.perf_counter() - t0
        total["boxes_loaded"] += 1
        total["voxels_loaded"] += ext[0] * ext[1] * ext[2]
        seed = section.seed_index(vox - lo, ext)
        holes = ()
        if filled:
            t0 = time.perf_counter()
            begin, listed, ids = box_holes(lo, hi)
            regions = _load_box(graph.store, lo, hi)
            # a label the box cannot hold may still have hole voxels in it, and a seed in one is valid: such a label
            # gets a word that no voxel of the box carries.  Only renumbered labels (eight bytes) can lack a word for a label they hold
            lost = (words < 0) & (listed > 0)
            if lost.any():
                words[lost] = int(d_lab.max().item()) + 1
            if eng is not None:
                regions = up(eng, regions)
                ids = up(eng, ids if ids.size else np.zeros(1, dtype=np.uint32))
            total["load_s"] += time.perf_counter() - t0
            holes = ((regions, begin[wrd], listed[wrd], ids),)
        want = words[wrd]
        seed[want < 0] = section.OUTSIDE                                 # a label this box cannot hold, nor (filled) one of its holes
        area, contact, clip, _ = run_sections(eng, d_lab, label_bytes, lo, ext, shape, an64, seed, np.maximum(want, 0).astype(np.uint32),
                                              nrm, *holes, stats)
        return area, contact, clip

    def hook(vox, wrd, nrm):
        cores = core_of(vox, shape, chunk_shape)

        def launch(which):
            which = np.asarray(which, dtype=np.int64)
            area, contact = np.zeros(which.size, dtype=np.float32), np.zeros(which.size, dtype=np.uint8)
            call = dict(boxes=[], items=[])
            total["calls"].append(call)
            pending, reach, grown = np.arange(which.size, dtype=np.int64), int(halo), 0
            sweep = not state["counted"]                                 # the first launch visits every core, for the counts
            while pending.size or sweep:
                group = group_by_core(cores[which[pending]], pending)
                clipped, boxes = [none], 0
                for k in (range(n_cores) if sweep else list(group)):
                    sel = group.get(k, none)
                    got = run_box(k, reach, vox[which[sel]], wrd[which[sel]], nrm[which[sel]], sweep)
                    if got is None:
                        if grown == 0:
                            raise ValueError("{}: the box of core {} at halo {} exceeds max_box_voxels = {}".format(name, k, reach, limit))
                        contact[sel] |= XS_CLIPPED
                        total["capped_items"] += int(sel.size)
                        continue
                    boxes += 1
                    area[sel], contact[sel] = got[0], got[1]
                    clipped.append(sel[got[2] != 0])
                call["boxes"].append(boxes)
                call["items"].append(int(pending.size))
                total["items" if grown == 0 else "items_rerun"] += int(pending.size)
                state["counted"], sweep = True, False
                pending = np.sort(np.concatenate(clipped))
                reach, grown = 2 * reach, grown + 1
            return area, contact

        return launch

    if jobs:
        utility._xs_run(None, None, None, shape, an, jobs, smoothing_window, step, multipass, repair_contacts, stats, launch_hook=hook)
        if not state["counted"]:                                         # (no vertex lies on a path: the counts decide -1 or 0 all the same)
            hook(np.zeros((0, 3), dtype=np.int64), np.zeros(0, dtype=np.uint32), np.zeros((0, 3)))(none)
        for (s, word, _), (area, contact) in zip(jobs, kept):           # utility.py:141-154, once the counts are known
            if counts[word] < 2:
                for attribute, value in (("cross_sectional_area", area), ("cross_sectional_area_contacts", contact)):
                    if value is None:
                        delattr(s, attribute)
                    else:
                        setattr(s, attribute, value)
    utility._xs_finish(skels)
    if timings is not None:
        timings.update(total, kernel_ms=stats.get("kernel_ms", 0.0), rounds=stats.get("rounds", 0), vertices=stats.get("vertices", 0),
                       occurrences=stats.get("occurrences", 0))
    return skeletons
