"""Function-level mirrors of the reference's hot-path call sites, running on the MI355X.
Same names, argument meaning and error behaviour as the modules kimimaro imports, so the parity tests
read like the reference's own tests (automated_test.py).  numpy in, numpy out; every call uploads,
runs the HIP kernel(s) through the C ABI, and downloads."""
from __future__ import annotations

import numpy as np

from . import _abi, feature, forest, points, section
from .engine import Engine
from .volume import DimensionError, _device_labels, as_3d, coords_of, linear_index

_engine = None


def engine():
    global _engine
    if _engine is None:
        _engine = Engine()
    return _engine


def edt(labels, anisotropy=(1, 1, 1), black_border=False, parallel=1, voxel_graph=None):
    """edt.edt as called at kimimaro/intake.py:178-183."""
    eng = engine()
    lab = np.asarray(labels)
    shape0 = lab.shape
    ndim = max(1, min(lab.ndim, 3))
    if lab.dtype == bool:
        lab = lab.view(np.uint8)
    if lab.dtype.kind not in "ui" or lab.dtype.itemsize > 4:
        lab = lab.astype(np.uint32)
    lab = np.asfortranarray(as_3d(lab))
    an = list(anisotropy) + [1.0] * (3 - len(anisotropy))
    if voxel_graph is not None:
        # edt.edt(voxel_graph=): walls between voxels (kh_edt_graph_cells / kh_edt_graph_sample; the package is absent from the
        # reference tree: PARITY UNPINNED, include/kimi_hip.h)
        if ndim < 3 and black_border:
            raise NotImplementedError("edt(voxel_graph=, black_border=True) on fewer than three axes")
        d_graph = eng.graph_to_device(voxel_graph, lab.shape)
        out = eng.edt_graph(eng.to_device(lab), lab.dtype.itemsize, d_graph, lab.shape, an, black_border)
        return out.cpu().numpy().reshape(lab.shape, order="F").reshape(shape0, order="F")
    out = eng.edt(eng.to_device(lab), lab.dtype.itemsize, lab.shape, an, black_border, ndim=ndim)
    return out.cpu().numpy().reshape(lab.shape, order="F").reshape(shape0, order="F")


def merge_pairs(merges, span, itemsize):
    """`merges` of voxel_connectivity_graph -> the pair table kh_voxel_graph reads: uint64 [m, 2], each row (lo, hi) the words a
    volume of `itemsize` bytes per label whose dtype holds `span` = (smallest, largest) stores for the two labels (intake._label_word),
    lo < hi, rows sorted lexicographically, unique.  A pair that names 0 or one value twice is dropped; order and duplicates of the
    input do not matter.  None and an empty list: no rows.  ValueError for anything but an (m, 2) array-like of integers and for a
    value the dtype cannot hold.  numpy only."""
    none = np.zeros((0, 2), dtype=np.uint64)
    if merges is None:
        return none
    arr = np.asarray(merges)
    if arr.size == 0 and arr.ndim <= 2:
        return none
    if arr.ndim != 2 or arr.shape[1] != 2:
        raise ValueError("merges must be an (m, 2) array of label values. Got shape: {}".format(arr.shape))
    if arr.dtype.kind not in "iub":
        raise ValueError("merges must be integers. Got: {}".format(arr.dtype))
    if int(arr.min()) < span[0] or int(arr.max()) > span[1]:
        raise ValueError("merges name a value outside the labels' range {}..{}".format(span[0], span[1]))
    if arr.dtype.kind == "u":
        words = arr.astype(np.uint64)
    else:
        words = arr.astype(np.int64).view(np.uint64) & np.uint64((1 << (8 * itemsize)) - 1)     # (two's complement: value mod 2^bits)
    words = np.sort(words, axis=1)
    words = words[(words[:, 0] != 0) & (words[:, 0] != words[:, 1])]
    return np.unique(words, axis=0) if words.shape[0] else none


def pairs_to_device(eng, pairs):
    """merge_pairs' table -> the flat int64 device tensor Engine.voxel_graph takes, None for an empty table"""
    if not pairs.shape[0]:
        return None
    return eng.torch.from_numpy(np.ascontiguousarray(pairs).reshape(-1).view(np.int64)).to(eng.device)


def voxel_connectivity_graph(labels, connectivity=26, merges=None):
    """cc3d.voxel_connectivity_graph(labels, connectivity), the source of skeletonize's voxel_graph= that the reference's docstring
    names (kimimaro/intake.py:113-117), on the MI355X (kh_voxel_graph; cc3d is absent from the reference tree: PARITY UNPINNED, the
    word is DEFINED in DESIGN.md 3.21).  Returns a uint32 array of the labels' shape, Fortran ordered, in cc3d's bit layout: the bit
    of a step is set iff the step is one of the `connectivity` (6, 18 or 26) neighbours, the neighbour lies inside the array and the
    two labels are equal (background included) or listed together in `merges`.
    labels: a 2-D or 3-D integer or bool numpy array of any order, or a tensor on the GPU; compared at full width.
    merges: None, or an (m, 2) integer array-like of label values that belong together although they differ (the supervoxels of an
      agglomerated segmentation).  NOT transitive: (a, b) and (b, c) do not connect a to c.  A pair that names 0 or a value twice is
      dropped.  ValueError for another shape and for a value the labels' dtype cannot hold; so for another connectivity."""
    if connectivity not in (6, 18, 26):
        raise ValueError("connectivity must be 6, 18 or 26. Got: {}".format(connectivity))
    if not hasattr(labels, "shape"):
        labels = np.asarray(labels)
    if len(labels.shape) not in (2, 3):
        raise DimensionError("voxel_connectivity_graph needs labels of two or three axes. Got: {}".format(tuple(labels.shape)))
    eng = engine()
    d_lab, itemsize, is_bool, shape, shape0, span = _device_labels(eng, labels)
    pairs = merge_pairs(merges, (0, 1) if is_bool else span, itemsize)
    if d_lab.numel() == 0:
        return np.zeros(shape0, dtype=np.uint32, order="F")
    d_graph = eng.voxel_graph(d_lab, itemsize, shape, connectivity, pairs_to_device(eng, pairs))
    return d_graph.cpu().numpy().view(np.uint32).reshape(shape, order="F").reshape(shape0, order="F")


def roll_invalidation_cube(labels, DBF, path, scale, const, anisotropy=(1, 1, 1), invalid_vertices={}):
    """kimimaro.skeletontricks.roll_invalidation_cube (skeletontricks.pyx:766-836).
    Accepts C or F contiguous `labels` (mutated in place and returned, like the reference: `out is labels`),
    coerces the DBF layout without touching the caller's array, raises ValueError when non contiguous."""
    is_f = labels.flags.f_contiguous
    if not (is_f or labels.flags.c_contiguous):
        raise ValueError(
            "roll_invalidation_cube: `labels` must be C- or F-contiguous. "
            "Got shape=({0}, {1}, {2}), strides=({3}, {4}, {5}).".format(*labels.shape, *labels.strides))
    if is_f and not DBF.flags.f_contiguous:
        DBF = np.asfortranarray(DBF)
    elif (not is_f) and not DBF.flags.c_contiguous:
        DBF = np.ascontiguousarray(DBF)
    s0, s1, s2 = labels.shape
    if is_f:
        sx, sy, sz = s0, s1, s2
        w = (anisotropy[0], anisotropy[1], anisotropy[2])
        locs = [c[0] + s0 * c[1] + s0 * s1 * c[2] for c in path if tuple(c) not in invalid_vertices]
    else:
        sx, sy, sz = s2, s1, s0
        w = (anisotropy[2], anisotropy[1], anisotropy[0])
        locs = [c[2] + s2 * c[1] + s2 * s1 * c[0] for c in path if tuple(c) not in invalid_vertices]
    if len(locs) == 0:
        return 0, labels
    eng = engine()
    t = eng.torch
    flat = labels.reshape(-1, order="F" if is_f else "C").view(np.uint8)
    d_mask = t.from_numpy(np.ascontiguousarray(flat)).to(eng.device)
    d_dbf = t.from_numpy(np.ascontiguousarray(DBF.reshape(-1, order="F" if is_f else "C").astype(np.float32, copy=False))).to(eng.device)
    d_path = t.from_numpy(np.asarray(locs, dtype=np.int64)).to(eng.device)
    d_cnt = t.zeros(1, dtype=t.int64, device=eng.device)
    _abi.check(eng.lib.kh_invalidate_cube(eng.ptr(d_mask), eng.ptr(d_dbf), sx, sy, sz, float(w[0]), float(w[1]), float(w[2]),
                                          eng.ptr(d_path), len(locs), np.float32(scale), np.float32(const),
                                          eng.ptr(d_cnt), eng.stream()))
    flat[...] = d_mask.cpu().numpy()
    return int(d_cnt.item()), labels


def roll_invalidation_ball_inside_component(labels, DBF, scale, const, anisotropy=(1, 1, 1), path=(), voxel_connectivity_graph=None):
    """kimimaro.skeletontricks.roll_invalidation_ball_inside_component (skeletontricks.pyx:373-418), call site
    kimimaro/trace.py:253-259: `labels` (uint8 / bool, Fortran order) is the mask of ONE object and is zeroed in place
    inside the rolling ball of every path vertex (radius scale * DBF[v] + const); returns (invalidated, labels).
    voxel_connectivity_graph (uint32, the labels' shape, cc3d's bit layout; skeletontricks.pyx:380,405-416 ->
    dijkstra_invalidation.hpp:126-191): a direction whose bit is clear in the word of the voxel being expanded is not followed."""
    if not labels.flags.f_contiguous:
        raise ValueError("roll_invalidation_ball_inside_component: labels must be Fortran ordered (skeletontricks.pyx:398)")
    eng = engine()
    lab = labels.view(np.uint8)
    dbf = np.asfortranarray(DBF, dtype=np.float32)
    pts = np.asarray(path, dtype=np.int64).reshape(-1, 3)
    if pts.shape[0] == 0:
        return 0, labels
    sx, sy = lab.shape[0], lab.shape[1]
    locs = pts[:, 0] + sx * (pts[:, 1] + sy * pts[:, 2])
    f = np.float32
    radii = (f(scale) * dbf.reshape(-1, order="F")[locs]).astype(np.float32) + f(const)     # f32 ops, pyx:393-395
    ctx = eng.single_object(lab, anisotropy, rmax=float(radii.max()), dbf=dbf, voxel_graph=voxel_connectivity_graph)
    d_alive = eng.torch.from_numpy(np.ascontiguousarray(lab.reshape(-1, order="F"))).to(eng.device)
    cnt, _ = eng.invalidate_ball(ctx, d_alive, locs, scale, const, anisotropy)
    lab.reshape(-1, order="F")[...] = d_alive.cpu().numpy()
    return cnt, labels


# ---------------------------------------------------------------------------------------------------------------------
# Function-level mirrors of the modules kimimaro/trace.py imports: same names, argument meaning
# and return values as at the call sites cited, every computation a HIP kernel reached through the C ABI.  The path
# loop of skeletonize() does not go through these (it has them fused on the device); they exist so that the reference's
# own vectors can be fed to the HIP implementation of every step.

def _f3(a, dtype=None):
    a = as_3d(a)
    return np.asfortranarray(a if dtype is None else a.astype(dtype, copy=False))


def zero2inf(field):
    """kimimaro.skeletontricks.zero2inf (skeletontricks.pyx:203-224): in place, returns the same array."""
    eng = engine()
    flat = field.reshape(-1, order="F")
    d = eng.torch.from_numpy(np.ascontiguousarray(flat)).to(eng.device)
    _abi.check(eng.lib.kh_zero2inf(eng.ptr(d), flat.size, eng.stream()))
    flat[...] = d.cpu().numpy()
    return field


def inf2zero(field):
    """kimimaro.skeletontricks.inf2zero (skeletontricks.pyx:177-198): in place, returns the same array."""
    eng = engine()
    flat = field.reshape(-1, order="F")
    d = eng.torch.from_numpy(np.ascontiguousarray(flat)).to(eng.device)
    _abi.check(eng.lib.kh_inf2zero(eng.ptr(d), flat.size, eng.stream()))
    flat[...] = d.cpu().numpy()
    return field


def fill(img, in_place=True, return_fill_count=True):
    """fill_voids.fill as called at kimimaro/trace.py:109."""
    eng = engine()
    m = _f3(img)
    d_mask = eng.torch.from_numpy(np.ascontiguousarray((m != 0).astype(np.uint8).reshape(-1, order="F"))).to(eng.device)
    d_out, n = eng.fill_voids(d_mask, m.shape)
    out = d_out.cpu().numpy().reshape(m.shape, order="F").astype(img.dtype).reshape(img.shape, order="F")
    if in_place:
        img[...] = out
        out = img
    return (out, n) if return_fill_count else out


def compute_pdrf(dbf_max, pdrf_scale, pdrf_exponent, DBF, DAF, max_daf):
    """kimimaro.trace.compute_pdrf (kimimaro/trace.py:315-356): DBF has been through zero2inf, DAF is normalised in
    place (like the reference).  Power-of-two exponents take the repeated-squaring branch (:343-345); any other
    exponent the np.power branch (:346-347): the device computes the base and the tail, numpy itself the power (its
    rounding is the host libm's -- the only function that reproduces the reference's bits on a given machine)."""
    eng = engine()
    f = np.float32
    M = f(1 / (f(dbf_max) ** 1.01))
    t = eng.torch
    d_dbf = t.from_numpy(np.ascontiguousarray(np.asarray(DBF, dtype=np.float32).reshape(-1, order="F"))).to(eng.device)
    daf_flat = DAF.reshape(-1, order="F")
    d_daf = t.from_numpy(np.ascontiguousarray(daf_flat)).to(eng.device)
    d_out = eng.empty(d_dbf.numel(), t.float32)
    call = lambda stage: _abi.check(eng.lib.kh_pdrf_field(eng.ptr(d_dbf), eng.ptr(d_daf), d_dbf.numel(), M, stage, f(pdrf_scale),
                                                          f(max_daf), eng.ptr(d_out), eng.stream()))
    if _abi.is_pow2_exponent(pdrf_exponent):
        call(int(pdrf_exponent).bit_length() - 1)
    else:
        call(_abi.PDRF_BASE)
        base = d_out.cpu().numpy()
        with np.errstate(all="ignore"):
            np.power(base, pdrf_exponent, out=base)
        d_out.copy_(t.from_numpy(base))
        call(_abi.PDRF_FINISH)
    daf_flat[...] = d_daf.cpu().numpy()
    return d_out.cpu().numpy().reshape(np.asarray(DBF).shape, order="F")


def _edf_many_sources(labels, sources, anisotropy, return_max_location, return_feature_map):
    """euclidean_distance_field from several sources at once, as kimimaro/utility.py:613-617 calls it: the whole-volume relaxation
    of kimimaro_amd.feature (csrc/feature.hip) on the mask; feature_map = 1-based number of the nearest source (the smallest among
    equally far ones), 0 where the field is +inf."""
    eng = engine()
    lab = _f3(labels)
    shape = tuple(int(v) for v in lab.shape)
    src = np.asarray(sources, dtype=np.int64).reshape(-1, 3)
    if src.shape[0] >= 2 ** 32 - 2:
        raise ValueError("fewer than 2^32 - 2 sources")
    if np.any(src < 0) or np.any(src >= np.array(shape)):
        raise ValueError("a source lies outside the array")
    d_mask = eng.to_device((lab != 0).astype(np.uint8))
    lin = src[:, 0] + shape[0] * (src[:, 1] + shape[1] * src[:, 2])
    d_dist, d_feat = feature.geodesic_voronoi(eng, d_mask, 1, shape, anisotropy, lin, np.arange(1, src.shape[0] + 1),
                                              np.ones(src.shape[0]), features=return_feature_map)
    host_shape = np.asarray(labels).shape
    out = [d_dist.cpu().numpy().reshape(shape, order="F").reshape(host_shape, order="F")]
    if return_max_location:
        t = eng.torch
        reach = t.where(t.isfinite(d_dist), d_dist, t.full_like(d_dist, -1.0))
        loc = int(t.nonzero(reach == reach.max())[0].item())          # ties -> smallest linear index, like kh_edf_batch
        out.append(tuple(int(v) for v in coords_of([loc], shape)[0]))
    if return_feature_map:
        fm = d_feat.cpu().numpy().view(np.uint32)
        fm[fm == _abi.NO_FEATURE] = 0
        out.append(fm.reshape(shape, order="F").reshape(host_shape, order="F"))
    return out[0] if len(out) == 1 else tuple(out)


def euclidean_distance_field(labels, source, anisotropy=(1, 1, 1), free_space_radius=0, voxel_graph=None,
                             return_max_location=False, return_feature_map=False):
    """dijkstra3d.euclidean_distance_field as called at kimimaro/trace.py:139-145, 302-307: geodesic distance inside
    the mask from `source`, +inf elsewhere; with return_max_location also the (x, y, z) of the largest finite value.
    `source` as an (n, 3) array of sources and / or return_feature_map=True (kimimaro/utility.py:613-617): the distance to the
    nearest source and, with return_feature_map, which source that is -- (field[, max_location][, feature_map])."""
    if return_feature_map or np.asarray(source).ndim == 2:
        if voxel_graph is not None:
            raise NotImplementedError("euclidean_distance_field from several sources does not take a voxel_graph (one-way edges)")
        if free_space_radius:
            raise NotImplementedError("euclidean_distance_field from several sources does not take a free_space_radius")
        return _edf_many_sources(labels, source, anisotropy, return_max_location, return_feature_map)
    eng = engine()
    lab = _f3(labels)
    # voxel_graph: the directions a voxel's word does not allow leave the neighbour masks the search works from
    # (kh_apply_voxel_graph; one-way edges for an asymmetric graph, like the invalidation reads it)
    ctx = eng.single_object(lab, anisotropy, voxel_graph=voxel_graph)
    shape = ctx["shape"]
    t = eng.torch
    task = ctx["task"]
    task["root"] = linear_index(source, shape)
    task["fsr"] = np.float32(free_space_radius)
    d_task = t.from_numpy(task.view(np.uint8).reshape(-1).copy()).to(eng.device)
    d_field = t.full((ctx["nvox"] + 4,), float("inf"), dtype=t.float32, device=eng.device)   # (+ padding: the searches read rows of three words)
    P = eng.ptr
    _abi.check(eng.lib.kh_edf_batch(P(d_task), 1, 2, P(ctx["d_lists"]), P(ctx["d_nbr"]), shape[0], shape[1], shape[2],
                                    float(anisotropy[0]), float(anisotropy[1]), float(anisotropy[2]), P(d_field),
                                    P(ctx["d_qstate"]), P(ctx["d_queues"]), eng.stream()))
    out = d_field[:ctx["nvox"]].cpu().numpy().reshape(shape, order="F").reshape(np.asarray(labels).shape, order="F")
    if not return_max_location:
        return out
    done = d_task.cpu().numpy().view(_abi.LABEL_T)
    return out, tuple(int(v) for v in coords_of([int(done["max_loc"][0])], shape)[0])


class _Search:
    """an object's device context + its weight field for kh_path_search"""

    def __init__(self, field, voxel_graph=None):
        eng = engine()
        self.eng = eng
        self.host_shape = np.asarray(field).shape
        f = _f3(field, np.float32)
        self.shape = f.shape
        self.graph = voxel_graph is not None
        self.ctx = eng.single_object(np.isfinite(f), (1, 1, 1), voxel_graph=voxel_graph)
        t = eng.torch
        flat = np.concatenate([f.reshape(-1, order="F"), np.full(4, np.inf, dtype=np.float32)])     # (+ padding: rows of three words)
        self.d_field = t.from_numpy(np.ascontiguousarray(flat)).to(eng.device)
        self.d_dist = t.full((f.size + 4,), float("inf"), dtype=t.float32, device=eng.device)

    def run(self, mode, source, target=0):
        eng, ctx, t, P = self.eng, self.ctx, self.eng.torch, self.eng.ptr
        cap = 4 * ctx["count"] + 1024
        d_path = eng.empty(cap, t.int32)
        d_n = t.zeros(1, dtype=t.int32, device=eng.device)
        sx, sy, sz = self.shape
        _abi.check(eng.lib.kh_path_search(P(ctx["d_task"]), mode, P(ctx["d_lists"]), P(ctx["d_nbr"]), sx, sy, sz, 1.0, 1.0, 1.0,
                                          P(self.d_field), P(self.d_dist), P(ctx["d_qstate"]), P(ctx["d_queues"]), int(source),
                                          int(target), P(d_path), cap, P(d_n), int(self.graph), eng.stream()))
        status = int(ctx["d_task"].cpu().numpy().view(_abi.LABEL_T)["status"][0])
        if status:
            raise _abi.KimiHipError("kh_path_search: %s" % _abi.describe_status(status))
        n = int(d_n.item())
        return coords_of(d_path[:n].cpu().numpy().view(np.uint32), self.shape)

    def parents(self, source):
        """kh_parental_field from `source` (a linear index): the parents array in the field's shape"""
        eng, ctx, t, P = self.eng, self.ctx, self.eng.torch, self.eng.ptr
        sx, sy, sz = self.shape
        d_par = eng.empty(sx * sy * sz, t.int32)
        _abi.check(eng.lib.kh_parental_field(P(ctx["d_task"]), P(ctx["d_lists"]), P(ctx["d_nbr"]), sx, sy, sz, P(self.d_field), P(self.d_dist),
                                             P(ctx["d_qstate"]), P(ctx["d_queues"]), int(source), P(d_par), int(self.graph),
                                             eng.stream()))
        status = int(ctx["d_task"].cpu().numpy().view(_abi.LABEL_T)["status"][0])
        if status:
            raise _abi.KimiHipError("kh_parental_field: %s" % _abi.describe_status(status))
        return d_par.cpu().numpy().view(np.uint32).reshape(self.shape, order="F").reshape(self.host_shape, order="F")


def railroad(field, source, voxel_graph=None):
    """dijkstra3d.railroad(field, source) as called at kimimaro/trace.py:240-242: the path from `source` to the nearest
    zero-weight voxel, rail end first, as an (n, 3) array."""
    s = _Search(field, voxel_graph)
    return s.run(0, linear_index(source, s.shape))


def parental_field(field, source, voxel_graph=None):
    """dijkstra3d.parental_field(field, source) as called at kimimaro/trace.py:155: the parents ARRAY of the weighted Dijkstra
    from `source` (uint32, the field's shape, Fortran order; entry = linear index of the predecessor + 1, 0 = none), which the
    caller may edit (`parents[tuple(root)] = 0`, trace.py:220) before handing it to path_from_parents (kh_parental_field)."""
    s = _Search(field, voxel_graph)
    return s.parents(linear_index(source, s.shape))


def path_from_parents(parents, target):
    """dijkstra3d.path_from_parents(parents, target) as called at kimimaro/trace.py:244: the pointer chase from `target`
    to the voxel whose entry is 0, returned source -> target as an (n, 3) array (kh_path_from_parents)."""
    eng = engine()
    t, P = eng.torch, eng.ptr
    par = _f3(parents, np.uint32)
    shape = par.shape
    d_par = t.from_numpy(np.ascontiguousarray(par.reshape(-1, order="F")).view(np.int32)).to(eng.device)
    cap = par.size
    d_path = eng.empty(cap, t.int32)
    d_n = t.zeros(1, dtype=t.int32, device=eng.device)
    _abi.check(eng.lib.kh_path_from_parents(P(d_par), par.size, linear_index(target, shape), P(d_path), cap, P(d_n), eng.stream()))
    n = int(d_n.item())
    if n == 0:
        raise _abi.KimiHipError("kh_path_from_parents: the parents of the target do not lead to a voxel without a parent")
    return coords_of(d_path[:n].cpu().numpy().view(np.uint32), shape)


def dijkstra(field, source, target, voxel_graph=None):
    """dijkstra3d.dijkstra(field, source, target) as called at kimimaro/trace.py:385 (point_to_point): the cheapest path
    from `source` to `target` where entering a voxel costs its field value, as an (n, 3) array source first.  The same
    search as parental_field + path_from_parents (one weighted Dijkstra from the source, predecessor walk from the
    target); ties between equally cheap paths follow the canonical predecessor rule of DESIGN.md 3.3."""
    s = _Search(field, voxel_graph)
    src = linear_index(source, s.shape)
    s.run(1, src)                                   # (the predecessor WALK crosses float-absorption plateaus, which a
    return s.run(2, src, linear_index(target, s.shape))     # parents array cannot express: DESIGN.md 3.3)


def extract_edges_from_binary_image(binimg, connectivity=26):
    """kimimaro.skeletontricks.extract_edges_from_binary_image (skeletontricks.pyx:1047-1086): (vertices uint32 (n, 3), edges uint32
    (m, 2)) of a 2-D / 3-D binary image, foreground = non-zero: the pairs of foreground voxels that are neighbours (6: along an
    axis, 18: also across a face diagonal, 26: also across a corner) and the voxels that lie on such a pair.  The reference numbers
    them in the iteration order of an unordered_set; here vertices come by ascending Fortran index, edges as (a, b), a < b, sorted
    by a, then b.  binimg: numpy, or a torch tensor on the GPU; bool or any integer dtype."""
    img = points.check_binary_image(binimg)          # TypeError / DimensionError before anything touches the GPU
    eng = engine()
    d_img, shape = points.device_binary_image(eng, img)
    return points.binary_edges(eng, d_img, shape, connectivity)


def first_label(labels):
    """kimimaro.skeletontricks.first_label (skeletontricks.pyx:307-326): (x, y, z) of the first non-zero voxel in the
    z / y / x raster, None when there is none."""
    eng = engine()
    lab = _f3(labels)
    t = eng.torch
    d = t.from_numpy(np.ascontiguousarray((lab != 0).astype(np.uint8).reshape(-1, order="F"))).to(eng.device)
    d_out = t.zeros(1, dtype=t.int64, device=eng.device)
    _abi.check(eng.lib.kh_first_label(eng.ptr(d), lab.size, eng.ptr(d_out), eng.stream()))
    loc = int(d_out.cpu().numpy().view(np.uint64)[0])
    if loc == 0xFFFFFFFFFFFFFFFF:
        return None
    return tuple(int(v) for v in coords_of([loc], lab.shape)[0])


def find_target(labels, PDRF):
    """the legacy kimimaro.skeletontricks.find_target(labels, PDRF) (skeletontricks.pyx:331-367): the first voxel in the
    reference's scan order (x outermost, z innermost) holding the maximum of PDRF over the mask; (-1, -1, -1) when the
    mask is empty (or holds only -inf / NaN)."""
    eng = engine()
    lab = _f3(labels)
    t = eng.torch
    d_lab = t.from_numpy(np.ascontiguousarray((lab != 0).astype(np.uint8).reshape(-1, order="F"))).to(eng.device)
    d_f = t.from_numpy(np.ascontiguousarray(_f3(PDRF, np.float32).reshape(-1, order="F"))).to(eng.device)
    d_out = t.zeros(1, dtype=t.int64, device=eng.device)
    sx, sy, sz = lab.shape
    _abi.check(eng.lib.kh_find_target(eng.ptr(d_lab), eng.ptr(d_f), sx, sy, sz, eng.ptr(d_out), eng.stream()))
    key = int(d_out.cpu().numpy().view(np.uint64)[0])
    if key == 0:
        return (-1, -1, -1)
    scan = 0xFFFFFFFF - (key & 0xFFFFFFFF)
    return (int(scan // (sy * sz)), int((scan // sz) % sy), int(scan % sz))


class CachedTargetFinder:
    """kimimaro.skeletontricks.CachedTargetFinder (skeletontricks.pyx:995-1045): find_target(labels) returns the
    still-valid voxel with the largest DAF (ties: the larger index), None when none is left."""

    def __init__(self, labels, daf):
        eng = engine()
        self.eng = eng
        lab = _f3(labels)
        self.shape = lab.shape
        self.ctx = eng.single_object(lab, (1, 1, 1))
        t = eng.torch
        d_daf = t.from_numpy(np.ascontiguousarray(_f3(daf, np.float32).reshape(-1, order="F"))).to(eng.device)
        self.d_ldaf = eng.empty(max(self.ctx["count"], 1), t.float32)
        _abi.check(eng.lib.kh_gather_f32(eng.ptr(d_daf), eng.ptr(self.ctx["d_lists"]), self.ctx["count"], eng.ptr(self.d_ldaf),
                                         eng.stream()))

    def find_target(self, labels):
        eng, t = self.eng, self.eng.torch
        d_alive = t.from_numpy(np.ascontiguousarray(_f3(labels).view(np.uint8).reshape(-1, order="F"))).to(eng.device)
        d_out = t.zeros(1, dtype=t.int64, device=eng.device)
        _abi.check(eng.lib.kh_target_max(eng.ptr(self.ctx["d_lists"]), eng.ptr(self.d_ldaf), eng.ptr(d_alive), self.ctx["count"],
                                         eng.ptr(d_out), eng.stream()))
        key = int(d_out.cpu().numpy().view(np.uint64)[0])
        if key == 0:
            return None
        return tuple(int(v) for v in coords_of([key & 0xFFFFFFFF], self.shape)[0])


def cross_sectional_area(binimg, pos, normal, anisotropy=(1, 1, 1), return_contact=False):
    """xs3d.cross_sectional_area as called at kimimaro/utility.py:315-320 (the package is absent from the reference tree: PARITY
    UNPINNED, the section is defined in DESIGN.md 3.12): the area, in physical units, of the part of the plane through the centre
    of voxel `pos` with normal `normal` (any length) that lies in the 26-connected piece of the foreground it starts in; with
    return_contact also the bits of the volume faces that piece touches (1, 2: x low, high; 4, 8: y; 16, 32: z).  0 for a position
    on the background or outside the image and for a zero or non-finite normal.  `pos` is rounded to a voxel.
    binimg: numpy, or a torch tensor on the GPU; bool or any integer dtype, foreground = non-zero."""
    img = points.check_binary_image(binimg)          # TypeError / DimensionError before anything touches the GPU
    eng = engine()
    d_img, shape = points.device_binary_image(eng, img)
    vox = np.round(np.asarray(pos, dtype=np.float64).reshape(1, 3)).astype(np.int64)
    n = np.asarray(normal, dtype=np.float64).reshape(1, 3)
    area, contact, _ = section.cross_sections(eng, d_img, 1, shape, anisotropy, section.seed_index(vox, shape), np.ones(1, np.uint32), n)
    return (float(area[0]), int(contact[0])) if return_contact else float(area[0])


def component_gaps(parts, bound=np.inf):
    """The table of nearest vertex pairs join_close_components_many works from (kh_part_gaps), for the parts of ONE
    group: Skeletons or (k, 3) vertex arrays, none of them empty.  Returns (d2 f64 [n, n], idx u32 [n, n, 2]): row = tree part,
    column = query part, d2 = the smallest squared distance in f64, idx = (tree vertex, query vertex) of the lexicographically
    smallest (d2, query vertex, tree vertex).  A pair whose d2 >= bound * bound has no record: d2 = +inf, both indices 0xFFFFFFFF;
    so has the diagonal."""
    verts = [np.asarray(getattr(p, "vertices", p), dtype=np.float32).reshape(-1, 3) for p in parts]
    eng = engine()
    bound = float(bound)
    return points.part_gaps(eng, [verts], [bound * bound])[0]


def component_clusters(parts, bound):
    """The sets join_close_components_many(split=True) cuts ONE group into (kh_part_clusters): parts as in
    component_gaps.  Returns cluster u32 [n]: for every part the smallest index among the parts connected to it through pairs whose
    bounding boxes are nearer than `bound` (their box distance squared, in f64, below bound * bound).  A pair with a record in
    component_gaps(parts, bound) is such a pair, so no record crosses two clusters."""
    verts = [np.asarray(getattr(p, "vertices", p), dtype=np.float32).reshape(-1, 3) for p in parts]
    eng = engine()
    bound = float(bound)
    if not verts:
        return np.zeros(0, dtype=np.uint32)
    _, _, boxes = points.part_boxes(verts)
    return points.part_clusters(eng, boxes, [0, len(verts)], [bound * bound])


def skeleton_component_labels(skeleton):
    """The labelling components_many works from (kh_forest_components), for ONE skeleton: comp u32 [n] over the vertices
    of skeleton.consolidate(), comp[v] = the smallest vertex connected to v.  The components of the skeleton, in the order
    Skeleton.components() lists them, are the distinct values in ascending order."""
    eng = engine()
    return forest.labels(eng, forest.pack([skeleton.consolidate()]))


def skeleton_paths(skeleton, return_indices=True):
    """Skeleton.paths(return_indices=...) of ONE skeleton as given, walked on the device where it is a forest (kh_walk_orient,
    kh_walk_emit): what paths_many returns for it.  A skeleton with a cyclic component is walked by the host."""
    eng = engine()
    w = forest.walk(eng, [skeleton])
    paths = skeleton.paths(return_indices=True) if w.host[0] else w.paths(0)
    return paths if return_indices else [skeleton.vertices[p] for p in paths]
