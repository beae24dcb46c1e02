"""The region graph of a dataset that is never resident as a whole, and what fills from it, on the plumbing of kimimaro_amd.boxes
(every public name is kimimaro_amd.post's too).  Nothing here takes a cross section: section_boxes builds its filled sections on
this graph, fill_all_holes_chunked and skeletonize_chunked(fill_holes_global=True) use it without one.

    region_graph_chunked(dataset, chunk_shape, region_store)             the region graph of a dataset from its cores:
    RegionGraph, _merge_regions                                          its result, and the host merge over the cuts
    hole_lists(graph, words)                                             hole(L) on that graph, as provisional ids
    fill_all_holes_chunked(dataset, chunk_shape, out, region_store)      the holes of every label of the dataset filled
"""
import time
from collections import namedtuple

import numpy as np

from . import _abi, ops
from .boxes import _load_box, _slices, _store_box, axes, down, label_type, store_like, up
from .holes import enclosed_regions, resolve_holes
from .plan import halo_boxes
from .volume import _device_labels, ranges

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
