"""A reference for the searches of csrc/sssp.h that shares nothing with them or with the oracle's heap Dijkstra: the Bellman
fixpoint d[v] = min over allowed neighbours u of fl32(d[u] + w), computed by 26 shifted-array relaxations in numpy float32,
repeated until no word changes.  No heap, no work lists, no order: distances start at +inf (0 at the source) and only go down, and
fl32(d + w) is monotone in d, so the iteration ends at the fixpoint the header comment of csrc/trace.hip claims.

Volumes are (x, y, z), Fortran order, linear index = x + sx * (y + sy * z).  A graph (cc3d's layout, voxel_graphs.GRAPH_BIT) gates a
step by the word of the voxel being EXPANDED (u), so an asymmetric graph gives one-way edges."""
import numpy as np

from voxel_graphs import DIRS, GRAPH_BIT

F32 = np.float32


def _as3(a):
    a = np.asarray(a)
    while a.ndim < 3:
        a = a[..., np.newaxis]
    return a


def lin(pt, shape):
    return int(pt[0]) + shape[0] * (int(pt[1]) + shape[1] * int(pt[2]))


def point(loc, shape):
    loc = int(loc)
    return (loc % shape[0], (loc // shape[0]) % shape[1], loc // (shape[0] * shape[1]))


def edge_lengths(anisotropy):
    """centre-to-centre length of each of the 26 steps, every operation rounded to float32"""
    w = np.array([F32(a) for a in anisotropy], dtype=F32)
    out = np.zeros(26, dtype=F32)
    for k, d in enumerate(DIRS):
        a, b, c = (w[i] if d[i] else F32(0) for i in range(3))
        out[k] = np.sqrt(F32(F32(a * a + b * b) + c * c))
    return out


def _slices(d, shape):
    """(the voxels u that have a neighbour in direction d, those neighbours v) as slice tuples"""
    src = tuple(slice(max(0, -e), n - max(0, e)) for e, n in zip(d, shape))
    dst = tuple(slice(max(0, e), n - max(0, -e)) for e, n in zip(d, shape))
    return src, dst


def _fixpoint(d, inside, expands, step_cost, graph):
    """d: float32 start values (changed in place and returned).  inside: voxels a step may enter.  expands: voxels a step may
    leave.  step_cost(k, src, dst): float32 scalar or array added for direction k."""
    shape = d.shape
    inf = F32(np.inf)
    steps = []
    for k, e in enumerate(DIRS):
        if any(abs(e[i]) >= shape[i] for i in range(3)):
            continue
        src, dst = _slices(e, shape)
        ok = expands[src] & inside[dst]
        if graph is not None:
            ok = ok & (((graph[src] >> np.uint32(GRAPH_BIT[k])) & np.uint32(1)) != 0)
        if ok.any():
            steps.append((src, dst, ok, step_cost(k, src, dst)))
    changed = True
    while changed:
        changed = False
        for src, dst, ok, w in steps:
            cand = np.where(ok, (d[src] + w).astype(F32), inf)
            old = d[dst]
            new = np.minimum(old, cand)
            if not np.array_equal(new, old):
                d[dst] = new
                changed = True
    return d


def edf_fixpoint(mask, source, anisotropy, graph=None, free_space_radius=0):
    """geodesic distance inside `mask` from `source` (an (x, y, z) point), +inf elsewhere; a step costs the edge length of its
    direction.  free_space_radius: mask voxels closer to the source than that in a straight line start at that distance."""
    m = _as3(mask) != 0
    shape = m.shape
    g = None if graph is None else _as3(graph).astype(np.uint32)
    d = np.full(shape, np.inf, dtype=F32, order="F")
    fsr = F32(free_space_radius)
    if fsr > 0:
        w = [F32(a) for a in anisotropy]
        ax = [(np.arange(shape[i], dtype=np.int64) - int(source[i])).astype(F32) * w[i] for i in range(3)]
        a, b, c = np.meshgrid(*ax, indexing="ij")
        s = ((a * a).astype(F32) + (b * b).astype(F32)).astype(F32)
        s = (s + (c * c).astype(F32)).astype(F32)
        sd = np.sqrt(s).astype(F32)
        seed = m & (sd < fsr)
        d[seed] = sd[seed]
    d[tuple(source)] = 0
    w26 = edge_lengths(anisotropy)
    return _fixpoint(d, m, m, lambda k, src, dst: w26[k], g)


def field_fixpoint(field, source, graph=None, rails_absorb=False):
    """distances of the weighted search from `source` over `field` (float32; +inf = outside the object): entering voxel v costs
    field[v].  rails_absorb: a zero-weight voxel other than the source is entered but never left (the railroad)."""
    f = np.asfortranarray(_as3(field), dtype=F32)
    inside = np.isfinite(f)
    expands = inside.copy()
    if rails_absorb:
        expands &= f != 0
        expands[tuple(source)] = True
    g = None if graph is None else _as3(graph).astype(np.uint32)
    d = np.full(f.shape, np.inf, dtype=F32, order="F")
    d[tuple(source)] = 0
    return _fixpoint(d, inside, expands, lambda k, src, dst: f[dst], g)


def farthest(d):
    """(linear index, value) of the largest finite value of d, ties to the smallest Fortran linear index"""
    flat = _as3(d).reshape(-1, order="F")
    key = np.where(np.isfinite(flat), flat, F32(-1))
    loc = int(np.argmax(key))
    return loc, flat[loc]


def nearest_rail(field, d, source):
    """(linear index, distance) of the zero-weight voxel (not the source) with the smallest (distance, index); None when none is
    reachable"""
    f = _as3(field).reshape(-1, order="F")
    flat = _as3(d).reshape(-1, order="F")
    rails = np.flatnonzero((f == 0) & np.isfinite(flat))
    rails = rails[rails != lin(source, _as3(field).shape)]
    if rails.size == 0:
        return None
    best = rails[np.lexsort((rails, flat[rails]))[0]]
    return int(best), flat[best]
