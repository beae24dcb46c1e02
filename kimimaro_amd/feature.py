"""Device plumbing of the geodesic Voronoi labels (csrc/feature.hip): seed, relax the distances to their
fixpoint, relax the features over the achieving edges of the final distances, renumber by first appearance.  Everything works on
whole-volume arrays resident in HBM; kimimaro_amd.utility.oversegment and kimimaro_amd.ops.euclidean_distance_field(...,
return_feature_map=True) are the callers."""
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
