"""Cross sections for a dataset that is never resident as a whole, on the plumbing of kimimaro_amd.boxes (every public name is
kimimaro_amd.post's too):

    cross_sectional_area_chunked(dataset, skeletons, chunk_shape, halo)  the skeletons' sections, the dataset in boxes
    cross_sectional_area_filled_chunked(dataset, skeletons, ...)         the same of the filled labels, on
    region_graph_chunked, hole_lists                                     the region graph of the dataset: region_boxes', imported here
"""
import time

import numpy as np

from . import ops, section, utility
from .boxes import (_load_box, _slices, axes, count_core, count_core_device, group_by_core, label_table, label_type, up,
                    upload_labels)
from .plan import core_of, halo_boxes
from .region_boxes import RegionGraph, hole_lists, region_graph_chunked  # noqa: F401

XS_CLIPPED = 64          # cross_sectional_area_contacts: the section was still clipped by the largest box that could be loaded


def _xs_box_budget(eng, itemsize, region_bytes=0):
    """The default max_box_voxels: what the free HBM pays for.  While a box is resident a voxel costs the label itself and, in round
    0, the copy of the core that is counted (2 x itemsize); labels of eight bytes are renumbered per box (utility._narrow_labels:
    torch.unique with its inverse -- the sorted copy, the permutation, the inverse and the shifted ids at 8 bytes each, the u32 ids,
    a mask: 56 bytes with the volume).  region_bytes: what else a voxel costs (cross_sectional_area_filled_chunked: 4, the box of
    the region store).  Kept back: the kernel's scratch (section.SCRATCH_BUDGET) and 1 GiB for the 2^24-voxel pieces of the count."""
    free = int(eng.torch.cuda.mem_get_info(eng.device)[0])
    return max(0, (free - section.SCRATCH_BUDGET - (1 << 30)) // ((2 * itemsize if itemsize < 8 else 56) + region_bytes))


def cross_sectional_area_chunked(dataset, skeletons, chunk_shape=(512, 512, 512), halo=64, anisotropy=(1, 1, 1), smoothing_window=1,
                                 step=1, multipass=False, repair_contacts=False, max_box_voxels=None, progress=False, timings=None,
                                 fill_holes=False, visualize_section_planes=False, _sections=None, walk="host"):
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
    CPU fallback: HipUnavailableError without the library or an MI355X.
    walk: cross_sectional_area's; "device" needs an engine (ops.engine()) whoever runs the boxes."""
    utility._xs_check_arguments(step, smoothing_window, visualize_section_planes)
    utility._xs_check_walk(walk)
    if fill_holes:
        raise NotImplementedError("cross_sectional_area_chunked(fill_holes=True) keeps raising at this entry point; the sections of "
                                  "filled labels of a dataset in boxes are cross_sectional_area_filled_chunked, which takes the same "
                                  "arguments and a region_store")
    return _xs_chunked("cross_sectional_area_chunked", False, None, dataset, skeletons, chunk_shape, halo, anisotropy, smoothing_window,
                       step, multipass, repair_contacts, max_box_voxels, timings, _sections, None, walk)


def cross_sectional_area_filled_chunked(dataset, skeletons, chunk_shape=(512, 512, 512), halo=64, anisotropy=(1, 1, 1),
                                        smoothing_window=1, step=1, multipass=False, repair_contacts=False, max_box_voxels=None,
                                        progress=False, timings=None, visualize_section_planes=False, region_store=None,
                                        _sections=None, _regions=None, walk="host"):
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
    touches the GPU (the host-logic tests).  Without them there is no CPU fallback.
    walk: cross_sectional_area's; "device" needs an engine (ops.engine()) whoever runs the boxes."""
    utility._xs_check_arguments(step, smoothing_window, visualize_section_planes)
    utility._xs_check_walk(walk)
    return _xs_chunked("cross_sectional_area_filled_chunked", True, region_store, dataset, skeletons, chunk_shape, halo, anisotropy,
                       smoothing_window, step, multipass, repair_contacts, max_box_voxels, timings, _sections, _regions, walk)


def _xs_chunked(name, filled, region_store, dataset, skeletons, chunk_shape, halo, anisotropy, smoothing_window, step, multipass,
                repair_contacts, max_box_voxels, timings, _sections, _regions, walk="host"):
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
        walker = None if walk == "host" else (eng if eng is not None else ops.engine())
        utility._xs_run(walker, None, None, shape, an, jobs, smoothing_window, step, multipass, repair_contacts, stats, launch_hook=hook,
                        walk=walk)
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
        timings.update({k: stats[k] for k in ("walk_host", "paths", "walk_s", "pack_s", "prepare_s") if k in stats})
    return skeletons
