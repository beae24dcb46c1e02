"""Device plumbing of the geodesic Voronoi labels (csrc/feature.hip): seed, relax the distances to their
fixpoint, relax the features over the achieving edges of the final distances, renumber by first appearance.  Everything works on
whole-volume arrays resident in HBM; kimimaro_amd.utility.oversegment and kimimaro_amd.ops.euclidean_distance_field(...,
return_feature_map=True) are the callers.  kimimaro_amd.segment_boxes.oversegment_chunked relaxes a dataset box by box with the same
kernels; seed_at, relax_box, box_shell_diff, first_appearance_box, first_appearance_map and remap_u32 are its."""
from __future__ import annotations

import numpy as np

from . import _abi

FIRST_BATCH, MAX_BATCH = 8, 64     # sweeps per launch batch (the host reads `changed` once per batch); doubled up to MAX_BATCH


class _Phases:
    """HIP events around the phases of a call, on the launch stream, when the caller asked for statistics"""

    def __init__(self, eng, stats):
        self.eng, self.stats, self.marks = eng, stats, []
        self.mark(None)

    def mark(self, name):
        if self.stats is None:
            return
        ev = self.eng.torch.cuda.Event(enable_timing=True)
        ev.record(self.eng.torch.cuda.current_stream(self.eng.device))
        self.marks.append((name, ev))

    def finish(self):
        if self.stats is None:
            return
        self.eng.sync()
        ms = self.stats.setdefault("ms", {})
        for (_, a), (name, b) in zip(self.marks, self.marks[1:]):
            ms[name] = ms.get(name, 0.0) + a.elapsed_time(b)


def brick_count(shape):
    bx, by, bz = _abi.BRICK
    return ((shape[0] + bx - 1) // bx) * ((shape[1] + by - 1) // by) * ((shape[2] + bz - 1) // bz)


def _to_fixpoint(eng, launch, shape, what):
    """Run `launch(d_dirty, d_changed, sweeps, first_sweep)` in batches until a sweep changed nothing.  Returns (sweeps up to and
    including the one that changed nothing, bricks visited by each of them).  The end is the fixpoint, never a count: the limit --
    a shortest path has fewer hops than the volume has voxels, and a sweep settles one more hop of every path -- only turns a
    defect into an error instead of a partial field."""
    t = eng.torch
    nbricks = brick_count(shape)
    nvox = shape[0] * shape[1] * shape[2]
    limit = nvox + 2
    d_dirty = t.zeros(3 * nbricks, dtype=t.uint8, device=eng.device)
    d_dirty[:nbricks] = 1                      # sweep 0 reads plane 0: every brick is awake
    done, batch, visited = 0, FIRST_BATCH, []
    while done < limit:
        n = min(batch, limit - done)
        d_changed = t.zeros(2 * n, dtype=t.int32, device=eng.device)
        _abi.check(launch(d_dirty, d_changed, n, done))
        c = d_changed.cpu().numpy().view(np.uint32).reshape(n, 2)
        still = np.flatnonzero(c[:, 0] == 0)
        if still.size:
            k = int(still[0]) + 1
            visited.extend(int(v) for v in c[:k, 1])
            return done + k, visited
        visited.extend(int(v) for v in c[:, 1])
        done += n
        batch = min(2 * batch, MAX_BATCH)
    raise _abi.KimiHipError("%s: no fixpoint after %d sweeps over %d voxels" % (what, done, nvox))


def neighbor_mask(eng, d_lab, label_bytes, shape, stats=None):
    """the same-label 26-connectivity words of the whole volume (kh_neighbor_mask), int32 [nvox] on the device"""
    ph = _Phases(eng, stats)
    d_nbr = eng.empty(shape[0] * shape[1] * shape[2], eng.torch.int32)
    _abi.check(eng.lib.kh_neighbor_mask(eng.ptr(d_lab), label_bytes, shape[0], shape[1], shape[2], eng.ptr(d_nbr), eng.stream()))
    ph.mark("mask")
    ph.finish()
    return d_nbr


def geodesic_voronoi(eng, d_lab, label_bytes, shape, anisotropy, seed_voxel, seed_number, seed_label, stats=None, features=True,
                     d_nbr=None):
    """d_lab: the label volume on the device (1-D, Fortran order, label_bytes 1 / 2 / 4; only equality and != 0 matter);
    seed_voxel / seed_number / seed_label: u32 host arrays, one entry per seed (linear voxel index, its number >= 1, the label its
    voxel has to carry); d_nbr: the volume's neighbour masks when the caller has them already.  Returns (d_dist f32 [nvox], d_feat
    int32 [nvox] holding the u32 numbers, _abi.NO_FEATURE where no seed reaches; None with features=False).  stats (a dict) receives milliseconds per phase (HIP events), sweeps and bricks visited."""
    t, lib, P = eng.torch, eng.lib, eng.ptr
    sx, sy, sz = (int(v) for v in shape)
    nvox = sx * sy * sz
    if nvox <= 0 or nvox >= 2 ** 32:
        raise ValueError("the volume must hold fewer than 2^32 voxels")
    an = np.asarray(anisotropy, dtype=np.float32)
    if an.shape != (3,) or not np.all(np.isfinite(an)) or not np.all(an > 0):
        raise ValueError("anisotropy must be three finite positive numbers")
    w = [float(v) for v in an]
    seed_voxel = np.ascontiguousarray(seed_voxel, dtype=np.uint32)
    seed_number = np.ascontiguousarray(seed_number, dtype=np.uint32)
    seed_label = np.ascontiguousarray(seed_label, dtype=np.uint32)
    nseeds = int(seed_voxel.size)
    assert seed_number.size == nseeds and seed_label.size == nseeds
    st = eng.stream()
    if d_nbr is None:
        d_nbr = neighbor_mask(eng, d_lab, label_bytes, (sx, sy, sz), stats)
    ph = _Phases(eng, stats)
    up = lambda a: t.from_numpy(a.view(np.int32)).to(eng.device) if nseeds else eng.empty(1, t.int32)
    d_sv, d_sn, d_sl = up(seed_voxel), up(seed_number), up(seed_label)
    d_dist = eng.empty(nvox, t.float32)
    d_feat = eng.empty(nvox, t.int32)
    _abi.check(lib.kh_geodesic_seed(P(d_sv), P(d_sn), nseeds, P(d_lab), label_bytes, P(d_sl), nvox, P(d_dist), P(d_feat), st))
    ph.mark("seed")
    sweeps_d, visited_d = _to_fixpoint(
        eng, lambda dirty, changed, n, first: lib.kh_geodesic_relax(P(d_nbr), sx, sy, sz, w[0], w[1], w[2], P(d_dist), P(dirty),
                                                                    P(changed), n, first, st), (sx, sy, sz), "kh_geodesic_relax")
    ph.mark("distance")
    # the feature recursion is well founded while fl(d + w) > d, i.e. while d / w < 2^24: refuse rather than loop
    finite = d_dist[t.isfinite(d_dist)]
    if finite.numel() and float(finite.max()) >= float(np.float32(2 ** 23) * an.min()):
        raise _abi.KimiHipError("geodesic distances reach 2^23 steps of the smallest voxel pitch: float32 absorbs further steps")
    del finite
    sweeps_f, visited_f = 0, []
    if features:
        sweeps_f, visited_f = _to_fixpoint(
            eng, lambda dirty, changed, n, first: lib.kh_feature_relax(P(d_nbr), sx, sy, sz, w[0], w[1], w[2], P(d_dist), P(d_feat),
                                                                       P(dirty), P(changed), n, first, st), (sx, sy, sz),
            "kh_feature_relax")
    ph.mark("feature")
    ph.finish()
    if stats is not None:
        stats.update(distance_sweeps=sweeps_d, feature_sweeps=sweeps_f, distance_bricks=visited_d, feature_bricks=visited_f,
                     bricks=brick_count((sx, sy, sz)), nvox=nvox, nseeds=nseeds)
    return d_dist, (d_feat if features else None)


# ---- a dataset in boxes (kimimaro_amd.segment_boxes.oversegment_chunked) ---------------------------------------------------
def _i64x3(values):
    a = np.ascontiguousarray(values, dtype=np.int64).reshape(-1)
    assert a.size == 3
    return a


def _words(eng, a):
    """u32 host words -> an int32 device tensor (one entry at least: an empty tensor has no pointer)"""
    t = eng.torch
    a = np.ascontiguousarray(a, dtype=np.uint32)
    return t.from_numpy(a.view(np.int32)).to(eng.device) if a.size else eng.empty(1, t.int32)


def seed_at(eng, d_lab, label_bytes, nvox, seed_voxel, seed_number, seed_label, d_dist=None, d_feat=None):
    """kh_geodesic_seed_at: the seeds (u32 host arrays as in geodesic_voronoi) into a box whose distances and / or features are
    there already; an array that is None is left out"""
    n = int(np.asarray(seed_voxel).size)
    if n == 0:
        return
    P = eng.optr
    d_sv, d_sn, d_sl = _words(eng, seed_voxel), _words(eng, seed_number), _words(eng, seed_label)
    _abi.check(eng.lib.kh_geodesic_seed_at(P(d_sv), P(d_sn), n, P(d_lab), label_bytes, P(d_sl), nvox, P(d_dist), P(d_feat), eng.stream()))


def relax_box(eng, d_nbr, shape, anisotropy, d_dist, d_feat=None):
    """the box's distances (d_feat None: kh_geodesic_relax) or its features on these distances (kh_feature_relax) to the box's
    fixpoint, in place -> sweeps"""
    P, lib, st = eng.ptr, eng.lib, eng.stream()
    sx, sy, sz = (int(v) for v in shape)
    w = [float(v) for v in np.asarray(anisotropy, dtype=np.float32)]
    if d_feat is None:
        launch = lambda dirty, changed, n, first: lib.kh_geodesic_relax(P(d_nbr), sx, sy, sz, w[0], w[1], w[2], P(d_dist), P(dirty),
                                                                        P(changed), n, first, st)
        return _to_fixpoint(eng, launch, (sx, sy, sz), "kh_geodesic_relax")[0]
    launch = lambda dirty, changed, n, first: lib.kh_feature_relax(P(d_nbr), sx, sy, sz, w[0], w[1], w[2], P(d_dist), P(d_feat),
                                                                   P(dirty), P(changed), n, first, st)
    return _to_fixpoint(eng, launch, (sx, sy, sz), "kh_feature_relax")[0]


def box_shell_diff(eng, d_old, d_now, shape, core_lo, core_hi):
    """kh_box_shell_diff on two device arrays of 32-bit words of a box of `shape` -> (the 26-bit mask of directions, in
    kh_neighbor_mask's order, towards which a changed core voxel lies in the core's outermost layer; the core voxels that changed;
    the largest finite non-negative f32 among the core's words of d_now, as bits)"""
    lo, hi = _i64x3(core_lo), _i64x3(core_hi)
    d_out = eng.empty(3, eng.torch.int32)
    _abi.check(eng.lib.kh_box_shell_diff(eng.ptr(d_old), eng.ptr(d_now), int(shape[0]), int(shape[1]), int(shape[2]), _abi.np_ptr(lo),
                                         _abi.np_ptr(hi), eng.ptr(d_out), eng.stream()))
    out = d_out.cpu().numpy().view(np.uint32)
    return int(out[0]), int(out[1]), int(out[2])


def first_appearance_table(eng, total):
    """the table kh_first_appearance_box accumulates into: int64 [total + 1] on the device, all ones"""
    return eng.torch.full((int(total) + 1,), -1, dtype=eng.torch.int64, device=eng.device)


def first_appearance_box(eng, d_feat, shape, core_lo, core_hi, origin, SX, SY, total, d_first):
    """kh_first_appearance_box: the smallest dataset raster index of every number 1..total among the core voxels of this box, into
    d_first (first_appearance_table)"""
    lo, hi, org = _i64x3(core_lo), _i64x3(core_hi), _i64x3(origin)
    _abi.check(eng.lib.kh_first_appearance_box(eng.ptr(d_feat), int(shape[0]), int(shape[1]), int(shape[2]), _abi.np_ptr(lo),
                                               _abi.np_ptr(hi), _abi.np_ptr(org), int(SX), int(SY), int(total), eng.ptr(d_first),
                                               eng.stream()))


def first_appearance_map(first):
    """first: int64 host array [total + 1], the table of kh_first_appearance_box (-1: the number owns no voxel; entry 0 unused) ->
    (map u32 [total + 1]: 1..K in the order of the first voxels, 0 for the others; K) -- renumber_first_appearance's map"""
    first = np.asarray(first, dtype=np.int64)[1:]
    owned = np.flatnonzero(first >= 0)
    order = owned[np.argsort(first[owned], kind="stable")]
    lut = np.zeros(first.size + 1, dtype=np.uint32)
    lut[order + 1] = np.arange(1, order.size + 1, dtype=np.uint32)
    return lut, int(order.size)


def remap_u32(eng, d_feat, d_map, total, nvox):
    _abi.check(eng.lib.kh_remap_u32(eng.ptr(d_feat), eng.ptr(d_map), int(total), int(nvox), eng.stream()))


def renumber_first_appearance(eng, d_feat, nvox, total, stats=None):
    """fastremap.renumber of the composite (kimimaro/utility.py:638; PARITY UNPINNED): the numbers 1..total that own a voxel become
    1..K in the order of their first voxel in the Fortran raster, everything else 0.  In place; returns K."""
    t, P = eng.torch, eng.ptr
    if total >= 2 ** 32 - 1:
        raise ValueError("fewer than 2^32 - 1 vertices in all")
    ph = _Phases(eng, stats)
    d_first = eng.empty(total + 1, t.int32)
    _abi.check(eng.lib.kh_first_appearance(P(d_feat), nvox, total, P(d_first), eng.stream()))
    first = d_first[1:].to(t.int64) & 0xFFFFFFFF
    K = int((first != _abi.NO_FEATURE).sum().item())
    order = t.argsort(first, stable=True)                       # (numbers without a voxel sort behind every index)
    d_map = t.zeros(total + 1, dtype=t.int64, device=eng.device)
    d_map[order[:K] + 1] = t.arange(1, K + 1, dtype=t.int64, device=eng.device)
    d_map = d_map.to(t.int32)                                   # (u32 words in an int32 tensor)
    _abi.check(eng.lib.kh_remap_u32(P(d_feat), P(d_map), total, nvox, eng.stream()))
    ph.mark("renumber")
    ph.finish()
    return K
