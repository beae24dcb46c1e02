"""The analysis half of the reference's API: kimimaro.oversegment (kimimaro/utility.py:562-644) and kimimaro.cross_sectional_area /
cross_sectional_area_single (kimimaro/utility.py:168-560; further down).

The reference walks the skeletons label by label, crops each label (shape_iterator, utility.py:114-166), asks dijkstra3d for the
feature map of the distance field from the skeleton's vertices and adds the crops into one uint64 volume on the host.  Here the
whole volume is relaxed at once on the MI355X (kimimaro_amd.feature, csrc/feature.hip): same-label connectivity is in the neighbour
masks, so all labels share one distance array and one feature array.  dijkstra3d and fastremap are absent from the reference tree:
PARITY UNPINNED, the result is defined order free."""
from __future__ import annotations

import copy
import time

import numpy as np

from . import _abi, feature, forest, ops, points, section
from .skeleton import Skeleton
from .volume import _device_labels

SEGMENTS_ATTRIBUTE = {"id": "segments", "data_type": "uint64", "num_components": 1}    # utility.py:583-587
XS_PROP = {"id": "cross_sectional_area", "data_type": "float32", "num_components": 1}                # utility.py:23-27
XS_CONTACT_PROP = {"id": "cross_sectional_area_contacts", "data_type": "uint8", "num_components": 1}  # utility.py:29-33


def extract_skeleton_from_binary_image(image):
    """kimimaro.extract_skeleton_from_binary_image (kimimaro/utility.py:54-56): turn a binary image that another algorithm has
    thinned already into a Skeleton -- every foreground voxel with a foreground 26-neighbour is a vertex, every such pair an edge
    (kimimaro_amd.ops.extract_edges_from_binary_image: the canonical numbering of DESIGN.md 3.11).  image: numpy, or a torch tensor
    on the GPU indexed [x, y(, z)]; bool or integers, foreground = non-zero."""
    verts, edges = ops.extract_edges_from_binary_image(image)
    return Skeleton(verts, edges)


def _skeleton_list(skeletons):
    """utility.py:592-597: a single skeleton, the values of a dict in its iteration order, or the sequence itself"""
    if hasattr(skeletons, "vertices"):
        return [skeletons]
    if isinstance(skeletons, dict):
        return list(skeletons.values())
    return list(skeletons)


def _narrow_labels(eng, d_flat, itemsize, span, wanted):
    """Labels of eight bytes -> dense u32 ids on the device (the searches read 1, 2 or 4 bytes per label); `wanted`: the original
    labels the skeletons name (Python ints; one outside `span`, what the volume's dtype holds, occurs nowhere).
    Returns (device labels, bytes per label, {original label: device label})."""
    t = eng.torch
    wanted = [L for L in wanted if span[0] <= L <= span[1]]
    if itemsize in (1, 2, 4):
        return d_flat, itemsize, {L: L % (1 << (8 * itemsize)) for L in wanted}      # (signed volumes: the unsigned view's word)
    uniq, inv = t.unique(d_flat.view(t.int64), return_inverse=True)      # sorted as SIGNED words
    d_lab = (inv + 1).to(t.int32)
    d_lab[d_flat.view(t.int64) == 0] = 0
    host = uniq.cpu().numpy()
    out = {}
    for L in wanted:
        word = L - 2 ** 64 if L >= 2 ** 63 else L
        k = int(np.searchsorted(host, word))
        if k < host.size and int(host[k]) == word:
            out[L] = k + 1
    return d_lab, 4, out


def _label_of(skel, is_bool):
    """utility.py:134-145: the label a skeleton segments, None when it is skipped outright"""
    if is_bool:
        return 1
    try:
        L = int(skel.id)
        if L != skel.id:
            return None
    except (TypeError, ValueError):
        return None
    return L if L != 0 else None


def _oversegment_check_arguments(downsample, fill_holes):
    """what oversegment and segment_boxes.oversegment_chunked refuse, before anything else happens"""
    if downsample > 0:
        raise NotImplementedError("oversegment(downsample > 0) needs osteoid's Skeleton.downsample, whose source is not available")
    if fill_holes:
        raise NotImplementedError("oversegment(fill_holes=True): the reference fills every crop on its own and ADDS overlapping "
                                  "crops, so a filled hole that holds another label sums two numberings (DESIGN.md 7)")


def oversegment(all_labels, skeletons, anisotropy=(1, 1, 1), progress=False, fill_holes=False, in_place=False, downsample=0,
                _stats=None):
    """kimimaro.oversegment (kimimaro/utility.py:562-644): use skeletons to cut a label volume into one segment per skeleton
    vertex -- every voxel goes to the vertex of its label's skeleton that is nearest along the geodesic (26-connected, anisotropic,
    float32) distance inside the label.  Returns (all_features, skeletons): the segments numbered 1..K by first appearance in the
    Fortran raster of the volume, in the smallest unsigned dtype that holds K (0: background, labels without a skeleton, parts of a
    label no vertex lies in), and a deep copy of the skeletons (dict -> dict, list -> list, one -> one) each with `segments`
    (uint64, the segment at every vertex's voxel, 0 for a vertex outside the volume) and the "segments" entry in extra_attributes.

    Among vertices that are equally far (in float32) the smallest-numbered one wins, vertices numbered in the container's order.
    A skeleton is skipped when its id is 0, its label does not occur or occupies a single voxel (utility.py:141-154); a bool
    volume assigns every skeleton to label 1.  all_labels: numpy, or a torch tensor on the GPU indexed [x, y, z].
    `progress` and `in_place` are accepted and have no effect (nothing is drawn, the input is never written to)."""
    _oversegment_check_arguments(downsample, fill_holes)
    eng = ops.engine()                                  # raises HipUnavailableError without the library or a gfx950 device
    t = eng.torch
    an = np.array(anisotropy, dtype=np.float32).reshape(-1)
    if an.shape != (3,) or not np.all(np.isfinite(an)) or not np.all(an > 0):
        raise ValueError("anisotropy must be three finite positive numbers")

    skeletons = copy.deepcopy(skeletons)
    skels = _skeleton_list(skeletons)
    d_flat, itemsize, is_bool, shape, shape0, span = _device_labels(eng, all_labels)
    sx, sy, sz = shape
    nvox = sx * sy * sz
    if nvox >= 2 ** 32:
        raise ValueError("the volume must hold fewer than 2^32 voxels")

    # every vertex of every skeleton gets a provisional number in the container's order; after the renumbering by first
    # appearance only the ORDER of these numbers is observable (it breaks ties), so the numbers of skipped skeletons are not reused
    labels_of = [_label_of(s, is_bool) for s in skels]
    d_lab, label_bytes, device_label = _narrow_labels(eng, d_flat, itemsize, span, {L for L in labels_of if L is not None})
    lin_parts, lab_parts = [], []
    for s, L in zip(skels, labels_of):
        v = np.asarray(s.vertices).reshape(-1, 3)
        vox = (v / an).round().astype(np.int64)                        # utility.py:610
        inside = np.all((vox >= 0) & (vox < np.array(shape, dtype=np.int64)), axis=1)
        lin = np.where(inside, vox[:, 0] + sx * (vox[:, 1] + sy * vox[:, 2]), -1)
        lin_parts.append(lin)
        lab_parts.append(np.full(lin.shape, device_label.get(L, 0) if L is not None else 0, dtype=np.int64))
        if not any(a["id"] == SEGMENTS_ATTRIBUTE["id"] for a in s.extra_attributes):        # add_property, utility.py:104-112
            s.extra_attributes.append(dict(SEGMENTS_ATTRIBUTE))
    lin_all = np.concatenate(lin_parts) if lin_parts else np.zeros(0, dtype=np.int64)
    lab_all = np.concatenate(lab_parts) if lab_parts else np.zeros(0, dtype=np.int64)
    total = int(lin_all.size)
    if total >= 2 ** 32 - 1:
        raise ValueError("fewer than 2^32 - 1 vertices in all")
    number_all = np.arange(1, total + 1, dtype=np.int64)
    seeds = np.flatnonzero((lin_all >= 0) & (lab_all != 0))

    # utility.py:152-154: a label whose bounding box is one voxel is skipped.  Only a seed voxel without any same-label neighbour
    # can be one: count such labels' voxels (a handful of reductions; one sort when there are many)
    if seeds.size:
        d_seed_lin = t.from_numpy(lin_all[seeds]).to(eng.device)
        word = (1 << (8 * label_bytes)) - 1
        lab_at = d_lab[d_seed_lin].to(t.int64) & word
        on_label = lab_at.cpu().numpy() == lab_all[seeds]
        seeds = seeds[on_label]                                        # (a vertex off its label seeds nothing)
    d_nbr = feature.neighbor_mask(eng, d_lab, label_bytes, shape, _stats)
    if seeds.size:
        lonely = d_nbr[t.from_numpy(lin_all[seeds]).to(eng.device)].cpu().numpy() == 0
        cand = np.unique(lab_all[seeds][lonely])
        if cand.size:
            if cand.size <= 64:
                # (the device tensor holds the u16 / u32 words as signed ones)
                native = lambda L: L - (word + 1) if label_bytes > 1 and L > word // 2 else L
                single = [int(L) for L in cand if int((d_lab == native(int(L))).sum().item()) <= 1]
            else:
                u, c = t.unique(d_lab, return_counts=True)
                u = (u.to(t.int64) & word).cpu().numpy()
                ones = set(int(x) for x in u[c.cpu().numpy() <= 1])
                single = [int(L) for L in cand if int(L) in ones]
            if single:
                seeds = seeds[~np.isin(lab_all[seeds], single)]

    d_dist, d_feat = feature.geodesic_voronoi(eng, d_lab, label_bytes, shape, an, lin_all[seeds].astype(np.uint32),
                                              number_all[seeds].astype(np.uint32), lab_all[seeds].astype(np.uint32), stats=_stats, d_nbr=d_nbr)
    del d_dist, d_nbr
    K = feature.renumber_first_appearance(eng, d_feat, nvox, total, stats=_stats)

    # skel.segments = all_features[vertex voxel] (utility.py:640-642)
    inside_all = lin_all >= 0
    seg_all = np.zeros(total, dtype=np.uint64)
    if inside_all.any():
        got = d_feat[t.from_numpy(lin_all[inside_all]).to(eng.device)].cpu().numpy().view(np.uint32)
        seg_all[inside_all] = got
    at = 0
    for s, lin in zip(skels, lin_parts):
        s.segments = seg_all[at:at + lin.size].copy()
        at += lin.size

    # fastremap.renumber returns the smallest unsigned dtype that holds the largest new label
    if K < 2 ** 8:
        out = d_feat.to(t.uint8).cpu().numpy()
    elif K < 2 ** 16:
        out = d_feat.to(t.int16).cpu().numpy().view(np.uint16)
    else:
        out = d_feat.cpu().numpy().view(np.uint32)
    return out.reshape(shape, order="F").reshape(shape0, order="F"), skeletons


# ---------------------------------------------------------------------------------------------------------------------
# kimimaro.cross_sectional_area (kimimaro/utility.py:168-560).  The reference crops every label, walks its skeleton's paths and asks
# xs3d for one section per vertex, one after the other.  Here the whole volume stays in HBM and every (vertex, normal) pair of every
# skeleton goes to the MI355X in one launch (kimimaro_amd.section, csrc/section.hip); the host only walks the paths.  xs3d and
# osteoid are absent from the reference tree: PARITY UNPINNED, sections and path order are defined in DESIGN.md 3.12.

def moving_average(a, n, mode="symmetric"):
    """kimimaro.utility.moving_average (kimimaro/utility.py:647-664): the mean over the trailing window a[i-n+1 .. i] along axis 0 of
    the input extended by n entries on both sides (np.pad's `mode`), accumulated in float64 as one running sum; the output has the
    input's length.  n == 1 and an empty input come back as they are."""
    if n <= 0:
        raise ValueError("Window size (%s), must be >= 1." % (n,))
    if n == 1 or len(a) == 0:
        return a
    width = [[n, n]] + [[0, 0]] * (a.ndim - 1)
    running = np.cumsum(np.pad(a, width, mode=mode), dtype=np.float64, axis=0)
    out = running[n:len(running) - n] - running[:len(running) - 2 * n]
    out /= float(n)
    return out


def _add_property(skel, prop):
    """utility.py:104-112"""
    if not any(a["id"] == prop["id"] for a in skel.extra_attributes):
        skel.extra_attributes.append(dict(prop))


def _xs_check_arguments(step, smoothing_window, visualize_section_planes, fill_holes=False):
    assert step > 0
    assert smoothing_window > 0
    if visualize_section_planes:
        raise NotImplementedError("visualize_section_planes=True paints the planes for microviewer, which is not a dependency here")
    if fill_holes:
        raise NotImplementedError("cross_sectional_area(fill_holes=True) keeps raising at this entry point; the sections of filled "
                                  "labels are cross_sectional_area_filled, which takes the same arguments")


def _label_voxel_counts(eng, d_lab, words):
    """how many voxels carry each of `words` (the unsigned words of the device labels) -> {word: count}"""
    t = eng.torch
    words = sorted(set(int(w) for w in words))
    if not words:
        return {}
    bits = 8 * d_lab.element_size()
    native = [w - (1 << bits) if d_lab.dtype.is_signed and w >= 1 << (bits - 1) else w for w in words]     # (u16 / u32 words in signed tensors)
    order = np.argsort(native)
    table = t.tensor([native[k] for k in order], dtype=d_lab.dtype, device=eng.device)
    counts = t.zeros(len(words) + 1, dtype=t.int64, device=eng.device)
    for chunk in d_lab.split(1 << 24):
        at = t.searchsorted(table, chunk).clamp_(max=len(words) - 1)
        at = t.where(table[at] == chunk, at, t.full_like(at, len(words)))
        counts += t.bincount(at, minlength=len(words) + 1)
    counts = counts.cpu().numpy()
    return {words[k]: int(counts[j]) for j, k in enumerate(order)}


def _xs_occurrences(skel, an, offset, shape, smoothing_window, step):
    """The (vertex, normal) pairs the loop of utility.py:269-332 visits, in its order.  Returns (vox int64 (n, 3): every vertex's
    voxel; occ_vertex int64 [m]; occ_normal f64 [m, 3])."""
    v = np.asarray(skel.vertices).reshape(-1, 3)
    if skel.space == "physical":
        vox = (v / an).round().astype(np.int64)                        # utility.py:238-239
    else:
        vox = np.round(v).astype(np.int64)                             # (UNPINNED for vertices that are not integral)
    vox = vox - np.asarray(offset, dtype=np.int64).reshape(1, 3)
    n = vox.shape[0]
    occ_vertex, occ_normal = [np.zeros(0, dtype=np.int64)], [np.zeros((0, 3), dtype=np.float64)]
    if n:
        # utility.py:246: `mapping` sends a voxel to the LAST vertex that lies in it
        _, inverse = np.unique(vox, axis=0, return_inverse=True)
        inverse = np.asarray(inverse).reshape(-1)
        last = np.zeros(int(inverse.max()) + 1, dtype=np.int64)
        np.maximum.at(last, inverse, np.arange(n))
        canon = last[inverse]
        extent = np.array(shape, dtype=np.int64)
        for path in skel.paths(return_indices=True):
            pts = vox[path]
            normals = (pts[1:] - pts[:-1]).astype(np.float32)
            normals = np.concatenate([normals, normals[-1:]])
            normals = moving_average(normals, smoothing_window)                       # forwards, then backwards: no phase shift
            normals = moving_average(normals[::-1], smoothing_window)[::-1]
            with np.errstate(invalid="ignore", divide="ignore"):
                normals = normals / np.linalg.norm(normals, axis=1, keepdims=True)
            i = np.arange(len(path))
            keep = ((i + 1) % step == 0) | (i == 0) | (i == len(path) - 1)            # utility.py:285-294: both ends stay
            keep &= np.all((pts >= 0) & (pts < extent), axis=1)
            occ_vertex.append(canon[path[keep]])
            occ_normal.append(normals[keep].astype(np.float64))
    return vox, np.concatenate(occ_vertex), np.concatenate(occ_normal)


def _xs_voxels(skels, an, offsets):
    """the voxel of every vertex of every skeleton, as _xs_occurrences rounds them, minus the job's offset -> int64 [V, 3], back to
    back; one pass over the call where every skeleton holds float32 vertices"""
    verts = [np.asarray(s.vertices).reshape(-1, 3) for s in skels]
    counts = np.array([v.shape[0] for v in verts], dtype=np.int64)
    shift = np.repeat(np.asarray(offsets, dtype=np.int64).reshape(-1, 3), counts, axis=0)
    if not verts:
        return np.zeros((0, 3), dtype=np.int64)
    if all(v.dtype == np.float32 for v in verts):
        v = np.concatenate(verts)
        physical = np.repeat(np.array([s.space == "physical" for s in skels], dtype=bool), counts)
        vox = np.round(v)
        if physical.any():
            vox[physical] = (v[physical] / an).round()
        return vox.astype(np.int64) - shift
    parts = [(v / an).round().astype(np.int64) if s.space == "physical" else np.round(v).astype(np.int64) for s, v in zip(skels, verts)]
    return np.concatenate(parts) - shift


def _xs_occurrences_many(eng, jobs, an, shape, smoothing_window, step, stats=None):
    """_xs_occurrences for every job (skeleton, word, offset) of a call, the paths walked and the normals smoothed on the device
    (forest.walk) -> per job (vox, occ_vertex, occ_normal, is_branch): the first three what _xs_occurrences(skel, an,
    offset, shape, smoothing_window, step) returns, bit for bit (NaNs by position); is_branch bool [n], True at skel.branches().
    Host numpy over the whole call: the rounding, canon, the keep filter, the compaction.  A skeleton with a cyclic component, or
    with a voxel coordinate of forest.VOX_LIMIT or more, goes through _xs_occurrences whole and counts in stats["walk_host"];
    stats also receives paths, occurrences (kept ones), walk_s and pack_s."""
    t0 = time.perf_counter()
    skels = [skel for skel, _, _ in jobs]
    vox = _xs_voxels(skels, an, [offset for _, _, offset in jobs])
    counts = np.array([np.asarray(s.vertices).reshape(-1, 3).shape[0] for s in skels], dtype=np.int64)
    vstart = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    owner = np.repeat(np.arange(len(skels)), counts)
    far = np.zeros(len(skels), dtype=bool)
    if vox.size:
        far[owner[np.abs(vox).max(axis=1) >= forest.VOX_LIMIT]] = True
    inner = {} if stats is None else stats
    pack0, walk0 = inner.get("pack_s", 0.0), inner.get("walk_s", 0.0)
    w = forest.walk(eng, [Skeleton(s.vertices) if f else s for s, f in zip(skels, far)], np.where(far[owner][:, None], 0, vox), smoothing_window, inner)
    if far.any():
        inner["walk_host"] = inner.get("walk_host", 0) + int(far.sum())
    # canon: the LAST vertex in a voxel, per skeleton -- the largest index of every (skeleton, voxel) group
    order = np.lexsort((vox[:, 2], vox[:, 1], vox[:, 0], owner)) if vox.size else np.zeros(0, dtype=np.int64)
    rows = np.concatenate([owner[order][:, None], vox[order]], axis=1)
    tail = np.ones(order.size, dtype=bool)
    tail[:-1] = np.any(rows[1:] != rows[:-1], axis=1)
    group = np.cumsum(tail) - tail                                           # lexsort is stable: a group's vertices ascend
    canon = np.empty(order.size, dtype=np.int64)
    canon[order] = order[np.flatnonzero(tail)[group]]
    # keep: every step-th vertex of a path and both its ends, inside the volume
    lens = np.diff(w.pstart)
    path_of = np.repeat(np.arange(lens.size), lens)
    i = np.arange(w.occ.size) - w.pstart[path_of]
    keep = ((i + 1) % step == 0) | (i == 0) | (i == lens[path_of] - 1)
    pts = vox[w.occ]
    keep &= np.all((pts >= 0) & (pts < np.array(shape, dtype=np.int64)), axis=1)
    kept = np.concatenate([[0], np.cumsum(keep)])
    cut = kept[w.pstart[w.pcut]]                                             # per skeleton: its kept occurrences
    occ_vertex = canon[w.occ[keep]] - np.repeat(vstart[:-1], np.diff(cut))
    occ_normal = w.normal[keep]
    branch = w.degree >= 3
    out, hosted = [], w.host | far
    for k, (skel, _, offset) in enumerate(jobs):
        a, b = vstart[k], vstart[k + 1]
        if hosted[k]:
            _, ov, on = _xs_occurrences(skel, an, offset, shape, smoothing_window, step)
            is_branch = np.zeros(b - a, dtype=bool)
            is_branch[skel.branches()] = True
        else:
            ov, on, is_branch = occ_vertex[cut[k]:cut[k + 1]], occ_normal[cut[k]:cut[k + 1]], branch[a:b]
        out.append((vox[a:b], ov, on, is_branch))
    if stats is not None:
        stats["paths"] = stats.get("paths", 0) + int(lens.size)
        stats["occurrences"] = int(sum(ov.size for _, ov, _, _ in out))
        spent = (stats.get("pack_s", 0.0) - pack0) + (stats.get("walk_s", 0.0) - walk0)
        stats["pack_s"] = stats.get("pack_s", 0.0) + (time.perf_counter() - t0) - spent
    return out


def _xs_check_walk(walk):
    if walk not in ("host", "device"):
        raise ValueError('walk must be "host" or "device". Got: %r' % (walk,))


def _xs_run(eng, d_lab, label_bytes, shape, an, jobs, smoothing_window, step, multipass, repair_contacts, stats, holes=None,
            launch_hook=None, walk="host"):
    """walk="device": the occurrences of all jobs come from _xs_occurrences_many, which needs `eng`; "host": from
    _xs_occurrences, job by job.  The items are the same, in the same order.
    launch_hook (cross_sectional_area_chunked, kimimaro_amd.post): who evaluates the items when the volume is not resident.  Once
    the items are laid out it is called as launch_hook(voxel int64 [m, 3], word u32 [m], normal f64 [m, 3]) -- item position k is
    the section through `voxel[k]` (in the frame of `shape`, which may hold 2^32 voxels or more) of the job word `word[k]` with
    `normal[k]` -- and returns the function from item positions (an int64 array) to (area f32, contact u8) that every round below
    calls in place of section.cross_sections; eng, d_lab and label_bytes are not read then.
    holes (fill_holes=True): section.hole_tables' (d_region, word_range, d_hole_regions), handed to the launch of every round.
    jobs: (skeleton, the device word of its label, the offset of the volume in the skeleton's voxel frame).  The sequential loop
    of the reference treats every vertex on its own -- a section depends on (voxel, normal, label) alone -- so its outcome is: a
    branch point is evaluated at every occurrence and ends as the mean; any other vertex is evaluated at its first occurrence when
    its area is 0 (or, repairing, its contact is not), then at the next one for as long as the area comes back 0.  Round 0 launches
    the first group, every later round the vertices that came back 0 and occur again."""
    t0 = time.perf_counter()
    an64 = an.astype(np.float64)
    starts, area_parts, contact_parts, seed_parts, word_parts, branch_parts, occ_v, occ_n = [0], [], [], [], [], [], [], []
    vox_parts = []
    _xs_check_walk(walk)
    many = _xs_occurrences_many(eng, jobs, an, shape, smoothing_window, step, stats) if walk == "device" and jobs else None
    for at, (skel, word, offset) in enumerate(jobs):
        nv = int(np.asarray(skel.vertices).reshape(-1, 3).shape[0])
        if repair_contacts or (multipass and hasattr(skel, "cross_sectional_area")):       # utility.py:250-255
            area_parts.append(np.array(skel.cross_sectional_area, dtype=np.float32).reshape(-1))
            contact_parts.append(np.array(skel.cross_sectional_area_contacts, dtype=np.uint8).reshape(-1))
            assert area_parts[-1].size == nv and contact_parts[-1].size == nv
        else:
            area_parts.append(np.zeros(nv, dtype=np.float32))
            contact_parts.append(np.zeros(nv, dtype=np.uint8))
        if many is None:
            vox, ov, on = _xs_occurrences(skel, an, offset, shape, smoothing_window, step)
            is_branch = np.zeros(nv, dtype=bool)
            is_branch[skel.branches()] = True
        else:
            vox, ov, on, is_branch = many[at]
        if launch_hook is None:
            seed_parts.append(section.seed_index(vox, shape))
        else:
            vox_parts.append(vox)
        word_parts.append(np.full(nv, word, dtype=np.uint32))
        branch_parts.append(is_branch)
        occ_v.append(ov + starts[-1])
        occ_n.append(on)
        starts.append(starts[-1] + nv)
    cat = lambda parts, dtype: np.concatenate(parts) if parts else np.zeros(0, dtype=dtype)
    areas, contacts = cat(area_parts, np.float32), cat(contact_parts, np.uint8)
    seeds, words, branch = cat(seed_parts, np.uint32), cat(word_parts, np.uint32), cat(branch_parts, bool)
    occ_v = cat(occ_v, np.int64)
    occ_n = np.concatenate(occ_n) if occ_n else np.zeros((0, 3), dtype=np.float64)

    t1 = t2 = time.perf_counter()
    rounds = 0
    sv = occ_v
    if occ_v.size:
        # the occurrences of every vertex side by side, in the loop's order
        order = np.argsort(occ_v, kind="stable")
        sv, sn = occ_v[order], occ_n[order]
        first = np.ones(sv.size, dtype=bool)
        first[1:] = sv[1:] != sv[:-1]
        group_start = np.flatnonzero(first)
        group_end = np.append(group_start[1:], sv.size)
        last_of_vertex = np.zeros(sv.size, dtype=bool)
        last_of_vertex[group_end - 1] = True

        if holes is not None:
            d_region, word_range, d_hole_regions = holes
            uniq, inverse = np.unique(words, return_inverse=True)
            ranges = np.array([word_range[int(w)] for w in uniq], dtype=np.uint32).reshape(-1, 2)
            hole_begin, hole_count = ranges[inverse, 0], ranges[inverse, 1]           # per vertex, as `words`

        def resident(which):
            filled = None if holes is None else (d_region, hole_begin[sv[which]], hole_count[sv[which]], d_hole_regions)
            return section.cross_sections(eng, d_lab, label_bytes, shape, an64, seeds[sv[which]], words[sv[which]], sn[which], stats,
                                          filled)[:2]

        launch = resident
        if launch_hook is not None:
            launch = launch_hook(np.concatenate(vox_parts)[sv], words[sv], sn)

        t1 = time.perf_counter()
        open0 = (areas[sv] == 0) | ((contacts[sv] > 0) if repair_contacts else False)
        at_branch = branch[sv]
        batch = np.flatnonzero(at_branch | (first & open0))
        got_area, got_contact = launch(batch)
        t2 = time.perf_counter()
        # branch points: the mean of all their values (float32, summed in the loop's order), the contacts of all / of the last
        is_b = at_branch[batch]
        b_pos, b_area, b_contact = batch[is_b], got_area[is_b], got_contact[is_b]
        if b_pos.size:
            if repair_contacts:
                ends = last_of_vertex[b_pos]
                contacts[sv[b_pos[ends]]] = b_contact[ends]
            else:
                np.bitwise_or.at(contacts, sv[b_pos], b_contact)
            cuts = np.flatnonzero(first[b_pos])
            for lo, hi in zip(cuts, np.append(cuts[1:], b_pos.size)):
                total = np.float32(0)
                for value in b_area[lo:hi]:
                    total = np.float32(total + value)
                areas[sv[b_pos[lo]]] = np.float32(total / np.float32(hi - lo))
        pending, p_area, p_contact = batch[~is_b], got_area[~is_b], got_contact[~is_b]
        rounds = 1
        while pending.size:
            v = sv[pending]
            areas[v] = p_area
            contacts[v] = p_contact if repair_contacts else contacts[v] | p_contact
            again = (p_area == 0) & ~last_of_vertex[pending]
            pending = pending[again] + 1
            if pending.size:
                p_area, p_contact = launch(pending)
                rounds += 1
    t3 = time.perf_counter()
    for k, (skel, _, _) in enumerate(jobs):
        skel.cross_sectional_area = areas[starts[k]:starts[k + 1]].copy()
        skel.cross_sectional_area_contacts = contacts[starts[k]:starts[k + 1]].copy()
    if stats is not None:
        stats["prepare_s"] = stats.get("prepare_s", 0.0) + (t1 - t0)
        stats["first_launch_s"] = stats.get("first_launch_s", 0.0) + (t2 - t1)
        stats["finish_s"] = stats.get("finish_s", 0.0) + (t3 - t2)
        stats["rounds"] = rounds
        stats["vertices"] = int(starts[-1])
        stats["occurrences"] = int(sv.size)


def _xs_anisotropy(anisotropy):
    an = np.array(anisotropy, dtype=np.float32).reshape(-1)
    if an.shape != (3,) or not np.all(np.isfinite(an)) or not np.all(an > 0):
        raise ValueError("anisotropy must be three finite positive numbers")
    return an


def cross_sectional_area_single(binimg, skel, roi=None, anisotropy=(1, 1, 1), smoothing_window=1, progress=False, in_place=False,
                                multipass=False, repair_contacts=False, visualize_section_planes=False, step=1, _stats=None, walk="host"):
    """kimimaro.cross_sectional_area_single (kimimaro/utility.py:168-349): the cross sectional areas of ONE skeleton against a binary
    image of its object (foreground = non-zero; numpy, or a torch tensor on the GPU).  roi: where the image sits in the skeleton's
    voxel frame -- anything with a `.minpt`, or three numbers -- subtracted from the vertices.  Everything else as
    cross_sectional_area.  The skeleton is changed in place and returned."""
    _xs_check_arguments(step, smoothing_window, visualize_section_planes)
    _xs_check_walk(walk)
    img = points.check_binary_image(binimg)
    eng = ops.engine()                                   # raises HipUnavailableError without the library or a gfx950 device
    an = _xs_anisotropy(anisotropy)
    d_img, shape = points.device_binary_image(eng, img)
    offset = np.zeros(3, dtype=np.int64) if roi is None else np.asarray(getattr(roi, "minpt", roi), dtype=np.int64).reshape(3)
    _xs_run(eng, d_img, 1, shape, an, [(skel, 1, offset)], smoothing_window, step, multipass, repair_contacts, _stats, walk=walk)
    _add_property(skel, XS_PROP)
    _add_property(skel, XS_CONTACT_PROP)
    return skel


def cross_sectional_area(all_labels, skeletons, anisotropy=(1, 1, 1), smoothing_window=1, progress=False, in_place=False,
                         fill_holes=False, multipass=False, repair_contacts=False, visualize_section_planes=False, step=1,
                         _stats=None, walk="host"):
    """kimimaro.cross_sectional_area (kimimaro/utility.py:351-560): for every vertex of every skeleton the area of the section of its
    label by the plane through the vertex's voxel whose normal points to the next vertex of the path (the part of
    the plane inside the 26-connected piece of cut voxels of the label around the vertex).  Every skeleton gains

      cross_sectional_area           float32 per vertex, physical units; -1 everywhere for a skeleton that was skipped
      cross_sectional_area_contacts  uint8 per vertex: bits 1, 2 the section touches the x = 0 / x = sx-1 face of the volume,
                                     4, 8 the y faces, 16, 32 the z faces -- the area may be an underestimate

    and both entries in extra_attributes.  The skeletons are changed in place and returned (dict -> dict, list -> list, one -> one).

    smoothing_window > 1 smooths the normals along every path (moving_average, forwards and backwards); step > 1 evaluates every
    step-th vertex of a path and its two ends; multipass keeps existing values and re-evaluates vertices whose area is 0 (several
    volumes, one skeleton); repair_contacts re-evaluates vertices whose contact is not 0 (after widening the volume).
    A skeleton is skipped when its id is 0, its label does not occur or occupies a single voxel (utility.py:141-154); a bool volume
    assigns every skeleton to label 1.  all_labels: numpy, or a torch tensor on the GPU indexed [x, y, z].
    fill_holes=True raises NotImplementedError here: cross_sectional_area_filled is that option.
    `progress` and `in_place` are accepted and have no effect.
    walk="device" walks the paths and smooths the normals of all skeletons on the GPU instead of skeleton by skeleton
    in the interpreter ("host", the default); the attributes come out equal, bit for bit.  Any other value is a ValueError."""
    _xs_check_arguments(step, smoothing_window, visualize_section_planes, fill_holes)
    _xs_check_walk(walk)
    return _xs_labels(all_labels, skeletons, anisotropy, smoothing_window, False, multipass, repair_contacts, step, _stats, walk)


def cross_sectional_area_filled(all_labels, skeletons, anisotropy=(1, 1, 1), smoothing_window=1, progress=False, in_place=False,
                                multipass=False, repair_contacts=False, visualize_section_planes=False, step=1, _stats=None,
                                walk="host"):
    """kimimaro.cross_sectional_area(fill_holes=True): cross_sectional_area, same arguments and outputs, with one substitution.  It
    takes the sections of filled(L) = L and its holes instead of L (kimimaro/utility.py:152-162 fills every label's
    crop with fill_voids): a hole of L is a 6-connected piece of the rest of the volume that owns no voxel on a face of the volume,
    whatever labels it holds, and a vertex inside one is a valid seed.  The volume itself is not changed,
    and the skip rules look at the label as given.  It costs one region pass over the volume and, while the call lasts,
    4 bytes per voxel (the region ids) plus 4 bytes per listed hole region on the device; the region pass (Engine.region_graph)
    allocates another 8 bytes per voxel (union-find parents, representatives), 13 bytes per region (its table) and the pair table
    (8 bytes x the power of two above 32 slots per region, 4 x that on a retry) and frees them before the first section.
    cross_sectional_area(fill_holes=False) allocates none of this."""
    _xs_check_arguments(step, smoothing_window, visualize_section_planes)
    _xs_check_walk(walk)
    return _xs_labels(all_labels, skeletons, anisotropy, smoothing_window, True, multipass, repair_contacts, step, _stats, walk)


def _xs_finish(skels):
    """utility.py:551-558: both properties on every skeleton; -1 / 0 for one that was skipped and has no values yet"""
    for s in skels:
        _add_property(s, XS_PROP)
        _add_property(s, XS_CONTACT_PROP)
        if not hasattr(s, "cross_sectional_area"):
            s.cross_sectional_area = np.full(len(s.vertices), -1, dtype=np.float32)
        if not hasattr(s, "cross_sectional_area_contacts"):
            s.cross_sectional_area_contacts = np.zeros(len(s.vertices), dtype=np.uint8)


def _xs_labels(all_labels, skeletons, anisotropy, smoothing_window, fill_holes, multipass, repair_contacts, step, _stats, walk="host"):
    """the body of cross_sectional_area and cross_sectional_area_filled, after the argument checks"""
    eng = ops.engine()                                   # raises HipUnavailableError without the library or a gfx950 device
    an = _xs_anisotropy(anisotropy)
    skels = _skeleton_list(skeletons)
    if int(np.prod([int(v) for v in getattr(all_labels, "shape", ())], dtype=object)) >= 2 ** 32 - 1:       # (before anything is copied)
        raise ValueError("the volume must hold fewer than 2^32 - 1 voxels")
    d_flat, itemsize, is_bool, shape, _, span = _device_labels(eng, all_labels)
    labels_of = [_label_of(s, is_bool) for s in skels]
    d_lab, label_bytes, device_label = _narrow_labels(eng, d_flat, itemsize, span, {L for L in labels_of if L is not None})
    counts = _label_voxel_counts(eng, d_lab, device_label.values())
    jobs = [(s, device_label[L], (0, 0, 0)) for s, L in zip(skels, labels_of)
            if L is not None and L in device_label and counts[device_label[L]] >= 2]       # utility.py:141-154
    holes = None
    if fill_holes and jobs:
        hole_stats = None if _stats is None else _stats.setdefault("holes", {})
        holes = section.hole_tables(eng, d_lab, label_bytes, shape, {word for _, word, _ in jobs}, hole_stats)
    _xs_run(eng, d_lab, label_bytes, shape, an, jobs, smoothing_window, step, multipass, repair_contacts, _stats, holes, walk=walk)
    _xs_finish(skels)
    return skeletons
