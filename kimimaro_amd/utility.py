"""The analysis half of the reference's API that needs nothing from xs3d: kimimaro.oversegment (kimimaro/utility.py:562-644).

The reference walks the skeletons label by label, crops each label (shape_iterator, utility.py:114-166), asks dijkstra3d for the
feature map of the distance field from the skeleton's vertices and adds the crops into one uint64 volume on the host.  Here the
whole volume is relaxed at once on the MI355X (kimimaro_amd.feature, csrc/feature.hip): same-label connectivity is in the neighbour
masks, so all labels share one distance array and one feature array.  dijkstra3d and fastremap are absent from the reference tree:
PARITY UNPINNED, the result is defined order free."""
from __future__ import annotations

import copy

import numpy as np

from . import _abi, feature
from .intake import format_labels
from .skeleton import Skeleton

SEGMENTS_ATTRIBUTE = {"id": "segments", "data_type": "uint64", "num_components": 1}    # utility.py:583-587


def extract_skeleton_from_binary_image(image):
    """kimimaro.extract_skeleton_from_binary_image (kimimaro/utility.py:54-56): turn a binary image that another algorithm has
    thinned already into a Skeleton -- every foreground voxel with a foreground 26-neighbour is a vertex, every such pair an edge
    (kimimaro_amd.ops.extract_edges_from_binary_image: the canonical numbering of DESIGN.md 3.11).  image: numpy, or a torch tensor
    on the GPU indexed [x, y(, z)]; bool or integers, foreground = non-zero."""
    from .ops import extract_edges_from_binary_image
    verts, edges = extract_edges_from_binary_image(image)
    return Skeleton(verts, edges)


def _skeleton_list(skeletons):
    """utility.py:592-597: a single skeleton, the values of a dict in its iteration order, or the sequence itself"""
    if hasattr(skeletons, "vertices"):
        return [skeletons]
    if isinstance(skeletons, dict):
        return list(skeletons.values())
    return list(skeletons)


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
    if downsample > 0:
        raise NotImplementedError("oversegment(downsample > 0) needs osteoid's Skeleton.downsample, whose source is not available")
    if fill_holes:
        raise NotImplementedError("oversegment(fill_holes=True): the reference fills every crop on its own and ADDS overlapping "
                                  "crops, so a filled hole that holds another label sums two numberings")
    from .ops import engine
    eng = engine()                                   # raises HipUnavailableError without the library or a gfx950 device
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
