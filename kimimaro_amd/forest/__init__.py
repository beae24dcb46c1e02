"""The forest form: the consolidated skeletons of a call packed back to back, the device calls on it (csrc/forest.hip)
and the way back to Skeletons.  One layer below kimimaro_amd.post, beside kimimaro_amd.points: it imports _abi and skeleton and nothing
else of the package, and the package imports it as `from . import forest`.  post.components_many, remove_dust_many, remove_loops_many
and remove_ticks_many are written on it.

    consolidated(skeleton)           consolidate(), skipped where the skeleton is in that form already
    pack(skeletons)                  -> Forest: xyz, radii, vertex_types, edges in call-wide numbering, vstart / estart per skeleton
    batches(skeletons)               -> the slices of a list that fit one device call each (V, M < 2^31)
    labels / measure / ticks         the device calls: kh_forest_components, kh_forest_measure, kh_forest_ticks
    adjacency, critical_lists        what kh_forest_ticks reads, made with numpy from the sorted edges and the measures
    unpack_components / _dust / _ticks   device results -> Skeletons, vectorised over the whole batch (stable argsort by label,
                                     rank renumbering, np.split); the only Python loops run over skeletons and components, to
                                     construct the objects
    Walk, WalkTables, walk(...)      the path walk (csrc/walk.hip): skeletons AS GIVEN back to back, what kh_walk_orient
                                     is given, and walk_labels / walk_orient / walk_emit around the device calls -> Walked, the paths
                                     of every tree of the call; post.paths_many and utility._xs_occurrences_many are written on it

The library allocates nothing: every output and scratch buffer is sized here."""
from __future__ import annotations

import time

import numpy as np

from .. import _abi
from ..skeleton import Skeleton

LIMIT = 2 ** 31                   # vertices and edges of one device call stay below this
HOST_DUST_EDGES = 2 ** 20         # a component of this many edges has its dust decision made by the host sum


class Forest:
    """xyz f32 [V, 3], radii f32 [V], vertex_types u8 [V], edges u32 [M, 2] (call-wide numbering, rows (lo, hi) ascending),
    vstart / estart i64 [S + 1]: skeleton k owns the vertices [vstart[k], vstart[k + 1]) and the edges [estart[k], estart[k + 1]);
    skeletons: the packed Skeletons (their id, transform and space go to what is unpacked)."""

    def __init__(self, xyz, radii, vertex_types, edges, vstart, estart, skeletons):
        self.xyz, self.radii, self.vertex_types, self.edges = xyz, radii, vertex_types, edges
        self.vstart, self.estart, self.skeletons = vstart, estart, skeletons

    @property
    def nverts(self):
        return int(self.vstart[-1])

    @property
    def nedges(self):
        return int(self.estart[-1])

    def skeleton_of_vertex(self, v):
        """the skeleton every vertex of `v` belongs to (empty skeletons own nothing and are never named)"""
        return np.searchsorted(self.vstart, v, side="right") - 1


def consolidated(skel):
    """skel.consolidate() -- and `skel` itself where that would only copy it: float32 vertices in strictly ascending lexicographic order,
    uint32 edge rows (lo, hi) in strictly ascending order, every vertex named by an edge.  The check is a few passes over the arrays;
    consolidate() sorts the vertex rows.  The stages of postprocess_many hand each other skeletons that are in this form already."""
    v, e = skel.vertices, skel.edges
    n = v.shape[0]
    if n == 0 or e.size == 0 or v.dtype != np.float32 or e.dtype != np.uint32 or v.ndim != 2 or e.ndim != 2:
        return skel.consolidate()
    a, b = v[:-1], v[1:]
    rising = (b[:, 0] > a[:, 0]) | ((b[:, 0] == a[:, 0]) & ((b[:, 1] > a[:, 1]) | ((b[:, 1] == a[:, 1]) & (b[:, 2] > a[:, 2]))))
    lo, hi = e[:, 0].astype(np.int64), e[:, 1].astype(np.int64)
    key = (lo << 32) | hi
    if not rising.all() or not (lo < hi).all() or int(hi.max()) >= n or not (key[1:] > key[:-1]).all():
        return skel.consolidate()
    used = np.zeros(n, dtype=bool)
    used[lo] = True
    used[hi] = True
    return skel if used.all() else skel.consolidate()


def sizes(skeletons):
    """(vertices, edges) per skeleton as i64 arrays; a skeleton without edges occupies nothing"""
    nv = np.array([0 if s.edges.size == 0 else s.vertices.shape[0] for s in skeletons], dtype=np.int64)
    ne = np.array([s.edges.shape[0] if s.edges.size else 0 for s in skeletons], dtype=np.int64)
    return nv, ne


def batches(skeletons, limit=None):
    """the list cut between skeletons into slices whose vertices and edges each stay below `limit` (default LIMIT): one device call
    per slice.  ValueError for a single skeleton at or beyond it."""
    limit = LIMIT if limit is None else int(limit)
    nv, ne = sizes(skeletons)
    out, first, v, e = [], 0, 0, 0
    for k in range(len(skeletons)):
        if nv[k] >= limit or ne[k] >= limit:
            raise ValueError("skeleton %d has %d vertices and %d edges: one device call takes fewer than %d of each" % (k, nv[k], ne[k], limit))
        if v + nv[k] >= limit or e + ne[k] >= limit:
            out.append(slice(first, k))
            first, v, e = k, 0, 0
        v += int(nv[k])
        e += int(ne[k])
    out.append(slice(first, len(skeletons)))
    return out


def pack(skeletons, limit=None):
    """skeletons: CONSOLIDATED Skeletons (vertices unique and sorted, edge rows (lo, hi) sorted and unique, as consolidate() leaves
    them).  ValueError: a skeleton whose edge rows are not ascending pairs in ascending order, an edge that names a vertex outside
    its skeleton (it would cross into the next one), V or M at or beyond `limit` (default LIMIT; see batches)."""
    limit = LIMIT if limit is None else int(limit)
    skeletons = list(skeletons)
    nv, ne = sizes(skeletons)
    vstart = np.concatenate([[0], np.cumsum(nv)]).astype(np.int64)
    estart = np.concatenate([[0], np.cumsum(ne)]).astype(np.int64)
    if int(vstart[-1]) >= limit or int(estart[-1]) >= limit:
        raise ValueError("the forest holds %d vertices and %d edges: one device call takes fewer than %d of each" % (vstart[-1], estart[-1], limit))
    full = [s for s, n in zip(skeletons, ne) if n]
    if not full:
        return Forest(np.zeros((0, 3), np.float32), np.zeros(0, np.float32), np.zeros(0, np.uint8), np.zeros((0, 2), np.uint32),
                      vstart, estart, skeletons)
    local = np.concatenate([np.asarray(s.edges, dtype=np.int64).reshape(-1, 2) for s in full])
    owner = np.repeat(np.arange(len(skeletons)), ne)
    if local.min() < 0 or np.any(local[:, 1] >= nv[owner]):
        k = int(owner[np.flatnonzero((local[:, 1] >= nv[owner]) | (local[:, 0] < 0))[0]])
        raise ValueError("skeleton %d: an edge names a vertex outside its %d vertices (no edge may cross two skeletons)" % (k, nv[k]))
    if np.any(local[:, 0] >= local[:, 1]):
        raise ValueError("an edge row is not (lo, hi) with lo < hi: pack takes consolidated skeletons")
    edges = local + vstart[owner][:, None]
    key = (edges[:, 0] << 32) | edges[:, 1]
    if np.any(key[1:] <= key[:-1]):
        raise ValueError("edge rows are not sorted and unique: pack takes consolidated skeletons")
    return Forest(np.ascontiguousarray(np.concatenate([s.vertices for s in full]), dtype=np.float32),
                  np.ascontiguousarray(np.concatenate([s.radii for s in full]), dtype=np.float32),
                  np.ascontiguousarray(np.concatenate([s.vertex_types for s in full]), dtype=np.uint8),
                  np.ascontiguousarray(edges, dtype=np.uint32), vstart, estart, skeletons)


# ---- the device calls -------------------------------------------------------------------------------------------------------------
class Measures:
    """what kh_forest_components and kh_forest_measure say about a Forest, as host arrays: comp u32 [V]; nv, ne u32 [V] and cable f64
    [V] at the roots (0 elsewhere); degree u32 [V].  d_xyz: the forest's vertices on the device, which kh_forest_ticks reads again."""

    def __init__(self, comp, nv, ne, cable, degree, d_xyz=None):
        self.comp, self.nv, self.ne, self.cable, self.degree, self.d_xyz = comp, nv, ne, cable, degree, d_xyz


def _up(eng, arr):
    """a host array of 32-bit or wider words -> a flat device tensor"""
    arr = np.ascontiguousarray(arr).reshape(-1)
    if arr.dtype == np.uint32:
        arr = arr.view(np.int32)
    return eng.torch.from_numpy(arr).to(eng.device)


def labels(eng, forest):
    """kh_forest_components: comp u32 [V] (host), the smallest vertex connected to each vertex"""
    t, P = eng.torch, eng.ptr
    n, m = forest.nverts, forest.nedges
    if n == 0:
        return np.zeros(0, dtype=np.uint32)
    d_edges = _up(eng, forest.edges)
    d_comp = eng.empty(n, t.int32)
    _abi.check(eng.lib.kh_forest_components(P(d_edges), n, m, P(d_comp), eng.stream()))
    return d_comp.cpu().numpy().view(np.uint32)


def measure(eng, forest):
    """kh_forest_components + kh_forest_measure -> Measures"""
    t, P = eng.torch, eng.ptr
    n, m = forest.nverts, forest.nedges
    if n == 0:
        z = np.zeros(0, dtype=np.uint32)
        return Measures(z, z, z, np.zeros(0, dtype=np.float64), z)
    d_xyz = _up(eng, forest.xyz)
    d_edges = _up(eng, forest.edges)
    d_comp, d_nv, d_ne, d_deg = (eng.empty(n, t.int32) for _ in range(4))
    d_cable = eng.empty(n, t.float64)
    _abi.check(eng.lib.kh_forest_components(P(d_edges), n, m, P(d_comp), eng.stream()))
    _abi.check(eng.lib.kh_forest_measure(P(d_xyz), P(d_edges), P(d_comp), n, m, P(d_cable), P(d_nv), P(d_ne), P(d_deg), eng.stream()))
    words = t.stack([d_comp, d_nv, d_ne, d_deg]).cpu().numpy().view(np.uint32)
    return Measures(words[0], words[1], words[2], d_cable.cpu().numpy(), words[3], d_xyz)


def adjacency(edges, nverts):
    """the CSR adjacency kh_forest_ticks reads: (row_start u32 [V + 1], nbr u32 [2M], neighbours ascending, upper bool [2M]).  `upper`
    marks the slots whose neighbour is the larger end: in slot order they are the rows of `edges` in their (sorted) order."""
    e = np.asarray(edges, dtype=np.uint64).reshape(-1, 2)
    key = np.sort(np.concatenate([(e[:, 0] << np.uint64(32)) | e[:, 1], (e[:, 1] << np.uint64(32)) | e[:, 0]]))
    own = (key >> np.uint64(32)).astype(np.int64)
    nbr = (key & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    row_start = np.concatenate([[0], np.cumsum(np.bincount(own, minlength=int(nverts)))]).astype(np.uint32)
    return row_start, nbr, nbr > own


def critical_lists(comp, nv, ne, degree):
    """the components kh_forest_ticks is given: trees (ne == nv - 1) with at least one vertex of degree >= 3, each by its critical
    vertices (degree 1 or >= 3) in ascending order -> (crit u32 [C], crit_start u32 [K + 1]), components by ascending root"""
    comp = np.asarray(comp).astype(np.int64)
    degree = np.asarray(degree).astype(np.int64)
    tree = (nv.astype(np.int64) - 1 == ne.astype(np.int64)) & (ne > 0)           # at the roots
    branched = np.zeros(comp.size, dtype=bool)
    branched[comp[degree >= 3]] = True
    listed = tree & branched
    crit = np.flatnonzero((degree != 2) & (degree > 0) & listed[comp])
    crit = crit[np.argsort(comp[crit], kind="stable")]
    counts = np.unique(comp[crit], return_counts=True)[1]
    return crit.astype(np.uint32), np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)


def ticks(eng, forest, measures, threshold):
    """kh_forest_ticks on every tree of the forest that has a branch point: bool [M], False for the edges on removed paths"""
    t, P = eng.torch, eng.ptr
    n, m = forest.nverts, forest.nedges
    if m == 0:
        return np.zeros(0, dtype=bool)
    row_start, nbr, upper = adjacency(forest.edges, n)
    crit, crit_start = critical_lists(measures.comp, measures.nv, measures.ne, measures.degree)
    ncrit, ncomps, nslots = int(crit.size), int(crit_start.size) - 1, int(nbr.size)
    if ncomps == 0:
        return np.ones(m, dtype=bool)
    d_xyz = measures.d_xyz if measures.d_xyz is not None else _up(eng, forest.xyz)
    d_row, d_nbr, d_crit, d_cstart = _up(eng, row_start), _up(eng, nbr), _up(eng, crit), _up(eng, crit_start)
    d_slots = eng.empty(4 * nslots, t.int32)
    d_arity = eng.empty(n, t.int32)
    d_recs = eng.empty(5 * ncrit, t.int32)
    d_len = eng.empty(ncrit, t.float64)
    d_flag = eng.empty(ncrit, t.uint8)
    d_alive = eng.empty(nslots, t.uint8)
    _abi.check(eng.lib.kh_forest_ticks(P(d_xyz), P(d_row), P(d_nbr), P(d_crit), P(d_cstart), n, nslots, ncrit, ncomps, float(threshold),
                                       P(d_slots), P(d_arity), P(d_recs), P(d_len), P(d_flag), P(d_alive), eng.stream()))
    return d_alive.cpu().numpy()[upper] != 0


# ---- the path walk (csrc/walk.hip) --------------------------------------------------------------------------------
VOX_LIMIT = 2 ** 23               # |voxel coordinate| below this: a difference of two is an exact float32, as kh_walk_emit takes it


class Walk:
    """Skeletons AS GIVEN, back to back: vstart i64 [S + 1] counts every vertex of every skeleton (the numbers are the caller's; a
    vertex without an edge stays where it is), edges u32 [M, 2] the distinct (lo, hi) rows without self loops in call-wide numbering,
    ascending -- what Skeleton._neighbours makes of repeated, reversed, shuffled rows and self loops -- and their CSR adjacency
    row_start u32 [V + 1], nbr u32 [2M].  dev: what the device calls keep for each other between walk_labels, walk_orient and
    walk_emit."""

    def __init__(self, skeletons, limit=None):
        limit = LIMIT if limit is None else int(limit)
        self.skeletons = list(skeletons)
        nv = np.array([np.asarray(s.vertices).reshape(-1, 3).shape[0] for s in self.skeletons], dtype=np.int64)
        ne = np.array([np.asarray(s.edges).reshape(-1, 2).shape[0] for s in self.skeletons], dtype=np.int64)
        self.vstart = np.concatenate([[0], np.cumsum(nv)]).astype(np.int64)
        if int(self.vstart[-1]) >= limit or 2 * int(ne.sum()) >= limit:
            raise ValueError("the walk holds %d vertices and %d edge rows: one device call takes fewer than %d vertices and %d rows"
                             % (self.vstart[-1], ne.sum(), limit, limit // 2))
        rows = [np.asarray(s.edges, dtype=np.int64).reshape(-1, 2) for s in self.skeletons if np.asarray(s.edges).size]
        local = np.concatenate(rows) if rows else np.zeros((0, 2), dtype=np.int64)
        owner = np.repeat(np.arange(len(self.skeletons)), ne)
        if local.size and (local.min() < 0 or np.any(local.max(axis=1) >= nv[owner])):
            k = int(owner[np.flatnonzero((local.max(axis=1) >= nv[owner]) | (local.min(axis=1) < 0))[0]])
            raise ValueError("skeleton %d: an edge names a vertex outside its %d vertices" % (k, nv[k]))
        keep = local[:, 0] != local[:, 1]
        e = local[keep] + self.vstart[owner[keep]][:, None]
        key = np.unique((e.min(axis=1) << 32) | e.max(axis=1))
        self.edges = np.stack([key >> 32, key & 0xFFFFFFFF], axis=1).astype(np.uint32)
        self.row_start, self.nbr, _ = adjacency(self.edges, self.nverts)
        self.degree = np.diff(self.row_start.astype(np.int64))
        self.dev = {}

    @property
    def nverts(self):
        return int(self.vstart[-1])

    def skeleton_of_vertex(self, v):
        return np.searchsorted(self.vstart, v, side="right") - 1


def walk_batches(skeletons, limit=None):
    """the list cut between skeletons into slices of fewer than `limit` (default LIMIT) vertices and adjacency slots each; ValueError
    for a single skeleton at or beyond it"""
    limit = LIMIT if limit is None else int(limit)
    out, first, v, e = [], 0, 0, 0
    for k, s in enumerate(skeletons):
        nv, ns = int(np.asarray(s.vertices).reshape(-1, 3).shape[0]), 2 * int(np.asarray(s.edges).reshape(-1, 2).shape[0])
        if nv >= limit or ns >= limit:
            raise ValueError("skeleton %d has %d vertices and %d edge rows: one device call takes fewer than %d vertices and %d rows"
                             % (k, nv, ns // 2, limit, limit // 2))
        if v + nv >= limit or e + ns >= limit:
            out.append(slice(first, k))
            first, v, e = k, 0, 0
        v, e = v + nv, e + ns
    out.append(slice(first, len(skeletons)))
    return out


class WalkTables:
    """What kh_walk_orient is given beside the adjacency, from comp and the degrees (numpy): host bool [S], the skeletons with a
    cyclic component (they are walked by the host whole and none of their components is listed); root i64 [K], the smallest vertex of
    every listed component -- the trees of two vertices or more of the other skeletons, ascending; crit u32 [C], crit_start u32
    [K + 1]: their critical vertices (degree 1 or >= 3, and the smallest vertex whatever its degree), ascending; leaf_start u32
    [K + 1]: the prefix sum of their paths, (vertices of degree 1) - 1 each."""

    def __init__(self, walk, comp):
        comp = np.asarray(comp).astype(np.int64)
        n, degree = comp.size, walk.degree
        nv = np.bincount(comp, minlength=n)
        slots = np.bincount(comp, weights=degree, minlength=n).astype(np.int64)       # twice the edges, exact below 2^53
        proper = nv >= 2
        tree = proper & (slots == 2 * (nv - 1))
        self.host = np.zeros(len(walk.skeletons), dtype=bool)
        self.host[walk.skeleton_of_vertex(np.flatnonzero(proper & ~tree))] = True
        listed = tree.copy()
        at = np.flatnonzero(tree)
        listed[at] = ~self.host[walk.skeleton_of_vertex(at)]
        self.root = np.flatnonzero(listed)
        crit = np.flatnonzero(listed[comp] & ((degree != 2) | (comp == np.arange(n))))
        crit = crit[np.argsort(comp[crit], kind="stable")]
        index = np.cumsum(listed) - 1                                                  # at a listed root: its place in the list
        of = index[comp[crit]]
        self.crit = crit.astype(np.uint32)
        self.crit_start = np.concatenate([[0], np.cumsum(np.bincount(of, minlength=self.root.size))]).astype(np.uint32)
        leaves = np.bincount(of[degree[crit] == 1], minlength=self.root.size) - 1
        self.leaf_start = np.concatenate([[0], np.cumsum(leaves)]).astype(np.uint32)

    @property
    def npaths(self):
        return int(self.leaf_start[-1])


def walk_labels(eng, walk):
    """kh_forest_components on a Walk -> comp u32 [V] (host); the device copy and the adjacency stay in walk.dev"""
    t, P = eng.torch, eng.ptr
    n, m = walk.nverts, int(walk.edges.shape[0])
    if n == 0:
        return np.zeros(0, dtype=np.uint32)
    d_edges = _up(eng, walk.edges) if m else None
    d_comp = eng.empty(n, t.int32)
    _abi.check(eng.lib.kh_forest_components(eng.optr(d_edges), n, m, P(d_comp), eng.stream()))
    walk.dev["comp"] = d_comp
    return d_comp.cpu().numpy().view(np.uint32)


def walk_orient(eng, walk, tables):
    """kh_walk_orient -> path_len u32 [npaths] (host): the vertices of every path, the components' in the order of `tables`.  parent and
    path_leaf stay on the device, in walk.dev, for walk_emit."""
    t, P = eng.torch, eng.ptr
    n, ns, nc, k, npaths = walk.nverts, int(walk.nbr.size), int(tables.crit.size), int(tables.root.size), tables.npaths
    if k == 0:
        return np.zeros(0, dtype=np.uint32)
    d_row, d_nbr, d_crit, d_cstart, d_lstart = (_up(eng, a) for a in (walk.row_start, walk.nbr, tables.crit, tables.crit_start,
                                                                         tables.leaf_start))
    d_slots, d_recs = eng.empty(3 * ns, t.int32), eng.empty(8 * nc, t.int32)
    d_parent, d_depth = eng.empty(n, t.int32), eng.empty(n, t.int32)
    d_leaf, d_len = eng.empty(npaths, t.int32), eng.empty(npaths, t.int32)
    _abi.check(eng.lib.kh_walk_orient(P(d_row), P(d_nbr), P(walk.dev["comp"]), P(d_crit), P(d_cstart), P(d_lstart), n, ns, nc, k, npaths,
                                      P(d_slots), P(d_recs), P(d_parent), P(d_depth), P(d_leaf), P(d_len), eng.stream()))
    walk.dev["parent"], walk.dev["leaf"] = d_parent, d_leaf
    return d_len.cpu().numpy().view(np.uint32)


def walk_emit(eng, walk, first, last, pstart, vox, window):
    """kh_walk_emit for the paths [first, last): pstart i64 [last - first + 1] from 0; vox i32 [V, 3] or None with window 0 ->
    (occ_vertex u32 [m], normal f64 [m, 3] or None), host arrays"""
    t, P = eng.torch, eng.ptr
    m = int(pstart[-1])
    if last == first or m == 0:
        return np.zeros(0, dtype=np.uint32), (np.zeros((0, 3), dtype=np.float64) if window else None)
    key = "vox"
    if window and key not in walk.dev:
        walk.dev[key] = eng.torch.from_numpy(np.ascontiguousarray(vox, dtype=np.int32).reshape(-1)).to(eng.device)
    d_pstart = eng.torch.from_numpy(np.ascontiguousarray(pstart, dtype=np.int64)).to(eng.device)
    d_occ = eng.empty(m, t.int32)
    d_normal = eng.empty(3 * m, t.float64) if window else None
    d_first = eng.empty(3 * m, t.float64) if window > 1 else None
    _abi.check(eng.lib.kh_walk_emit(P(walk.dev["parent"]), P(walk.dev["leaf"][first:last]), P(d_pstart), eng.optr(walk.dev.get(key)),
                                    walk.nverts, last - first, m, int(window), P(d_occ), eng.optr(d_normal), eng.optr(d_first),
                                    eng.stream()))
    occ = d_occ.cpu().numpy().view(np.uint32)
    return occ, (d_normal.cpu().numpy().reshape(-1, 3) if window else None)


class Walked:
    """The paths of a call: host bool [S] (the skeletons with a cyclic component: not walked); pcut i64 [S + 1], the paths of skeleton
    k are [pcut[k], pcut[k + 1]), in the order of Skeleton.paths(); pstart i64 [P + 1], path p is occ[pstart[p]:pstart[p + 1]], root
    first; occ i64 [m] in call-wide numbering (vstart i64 [S + 1]); normal f64 [m, 3] or None; degree i64 [V], the distinct
    neighbours of every vertex."""

    def __init__(self, host, pcut, pstart, occ, normal, vstart, degree):
        self.host, self.pcut, self.pstart, self.occ, self.normal, self.vstart, self.degree = host, pcut, pstart, occ, normal, vstart, degree

    def paths(self, k):
        """Skeleton.paths(return_indices=True) of skeleton k"""
        cut = self.pstart[self.pcut[k]:self.pcut[k + 1] + 1]
        own = self.occ[cut[0]:cut[-1]] - self.vstart[k]
        return np.split(own, cut[1:-1] - cut[0]) if cut.size > 1 else []


def walk(eng, skeletons, vox=None, window=0, stats=None, limit=None):
    """The paths of every skeleton of the list in one pass (walk_batches cuts a list too long for it) -> Walked.  vox: with
    window >= 1 the voxel of every vertex of the call, int64 [V, 3], |coordinate| < VOX_LIMIT wherever a path runs; the normals are
    kh_walk_emit's.  ValueError for a skeleton whose occurrences alone reach `limit` (default LIMIT).  stats: walk_s (the device
    calls with their copies), pack_s (the numpy around them) and walk_host are added to."""
    limit = LIMIT if limit is None else int(limit)
    t0 = time.perf_counter()
    w = Walk(skeletons, limit)
    nskel = len(w.skeletons)
    t1 = time.perf_counter()
    comp = walk_labels(eng, w)
    t2 = time.perf_counter()
    tables = WalkTables(w, comp)
    t3 = time.perf_counter()
    path_len = walk_orient(eng, w, tables).astype(np.int64)
    device_s = (t2 - t1) + (time.perf_counter() - t3)
    # the paths of a skeleton are consecutive: its components are, by smallest vertex
    paths_of = np.zeros(nskel, dtype=np.int64)
    np.add.at(paths_of, w.skeleton_of_vertex(tables.root), np.diff(tables.leaf_start.astype(np.int64)))
    pcut = np.concatenate([[0], np.cumsum(paths_of)]).astype(np.int64)
    pstart = np.concatenate([[0], np.cumsum(path_len)]).astype(np.int64)
    occ_of = pstart[pcut[1:]] - pstart[pcut[:-1]]
    if window:
        vox = np.asarray(vox, dtype=np.int64).reshape(-1, 3)
        assert vox.shape[0] == w.nverts
    # the emit calls: skeletons [a, b) with fewer than `limit` occurrences together
    occ_parts, normal_parts, a = [], [], 0
    while a < nskel:
        b, m = a, 0
        while b < nskel and m + int(occ_of[b]) < limit:
            m += int(occ_of[b])
            b += 1
        if b == a:
            raise ValueError("skeleton %d has %d vertices on its paths: one device call takes fewer than %d" % (a, occ_of[a], limit))
        first, last = int(pcut[a]), int(pcut[b])
        t4 = time.perf_counter()
        occ, normal = walk_emit(eng, w, first, last, pstart[first:last + 1] - pstart[first], vox, window)
        device_s += time.perf_counter() - t4
        occ_parts.append(occ.astype(np.int64))
        normal_parts.append(normal)
        a = b
    if not occ_parts:
        occ_parts, normal_parts = [np.zeros(0, dtype=np.int64)], [np.zeros((0, 3), dtype=np.float64)]
    occ = np.concatenate(occ_parts) if len(occ_parts) != 1 else occ_parts[0]
    normal = None
    if window:
        normal = np.concatenate(normal_parts) if len(normal_parts) != 1 else normal_parts[0]
    if stats is not None:
        stats["walk_s"] = stats.get("walk_s", 0.0) + device_s
        stats["pack_s"] = stats.get("pack_s", 0.0) + (time.perf_counter() - t0) - device_s
        stats["walk_host"] = stats.get("walk_host", 0) + int(tables.host.sum())
    return Walked(tables.host, pcut, pstart, occ, normal, w.vstart, w.degree)


# ---- back to Skeletons ------------------------------------------------------------------------------------------------------------
class Groups:
    """The vertices and edges of a Forest grouped by component, from comp alone (vectorised): `order` lists the vertices component
    after component (components by ascending root, which is skeleton after skeleton; a component's vertices ascending), `vcut` [K + 1]
    cuts it; `index` [V] is the component of every vertex, `root` [K] its smallest vertex, `local` [V] a vertex's rank within its
    component; `eorder` / `ecut` do the same for the edge rows, `ecomp` [M] is the component of every edge."""

    def __init__(self, forest, comp):
        comp = np.asarray(comp).astype(np.int64)
        n = comp.size
        self.order = np.argsort(comp, kind="stable")
        by = comp[self.order]
        head = np.ones(n, dtype=bool)
        head[1:] = by[1:] != by[:-1]
        self.root = by[head]
        first = np.flatnonzero(head)
        self.vcut = np.concatenate([first, [n]])
        self.index = np.empty(n, dtype=np.int64)
        self.index[self.order] = np.cumsum(head) - 1
        rank = np.empty(n, dtype=np.int64)
        rank[self.order] = np.arange(n)
        self.local = rank - first[self.index] if n else rank
        e = forest.edges.astype(np.int64)
        self.ecomp = self.index[e[:, 0]] if e.size else np.zeros(0, dtype=np.int64)
        self.eorder = np.argsort(self.ecomp, kind="stable")
        self.ecut = np.searchsorted(self.ecomp[self.eorder], np.arange(self.root.size + 1))


def _skeleton(like, vertices, edges, radii, vertex_types):
    return Skeleton(vertices, edges, radii, vertex_types, like.id, like.transform, like.space)


def unpack_components(forest, comp, groups=None):
    """per skeleton of the forest the list Skeleton.components() returns for it: its components by smallest vertex, each with its
    vertices in order and its edges as sorted unique rows in its own numbering (a vertex without an edge is no component)"""
    g = Groups(forest, comp) if groups is None else groups
    out = [[] for _ in forest.skeletons]
    if g.root.size == 0:
        return out
    xyz, radii, vtypes = forest.xyz[g.order], forest.radii[g.order], forest.vertex_types[g.order]
    edges = g.local[forest.edges.astype(np.int64)[g.eorder]].astype(np.uint32)
    owner = forest.skeleton_of_vertex(g.root)
    for k in np.flatnonzero(np.diff(g.ecut) > 0).tolist():
        a, b, c, d = g.vcut[k], g.vcut[k + 1], g.ecut[k], g.ecut[k + 1]
        out[owner[k]].append(_skeleton(forest.skeletons[owner[k]], xyz[a:b], edges[c:d], radii[a:b], vtypes[a:b]))
    return out


def component_cable(forest, groups, k):
    """Skeleton.cable_length() of component k: the float32 lengths of its edges, in their order, in numpy's float32 sum"""
    e = forest.edges[groups.eorder[groups.ecut[k]:groups.ecut[k + 1]]].astype(np.int64)
    d = (forest.xyz[e[:, 1]] - forest.xyz[e[:, 0]]).astype(np.float32)
    d *= d
    return float(np.sum(np.sqrt(np.sum(d, axis=1))))


def unpack_dust(forest, groups, keep):
    """keep: bool per component of `groups`.  Per skeleton what remove_dust returns: Skeleton.simple_merge of the kept components --
    vertices component by component, edges likewise -- and a bare Skeleton() where none is kept."""
    g = groups
    nskel = len(forest.skeletons)
    if g.root.size == 0:
        return [Skeleton() for _ in range(nskel)]
    keep = np.asarray(keep, dtype=bool)
    vsel = g.order[keep[g.index[g.order]]]                                  # the kept vertices in output order
    skel_of = forest.skeleton_of_vertex(vsel)
    vcut = np.searchsorted(skel_of, np.arange(nskel + 1))
    place = np.full(forest.nverts, -1, dtype=np.int64)
    place[vsel] = np.arange(vsel.size) - vcut[skel_of]                      # the rank among its skeleton's kept vertices
    esel = g.eorder[keep[g.ecomp[g.eorder]]]
    edges = place[forest.edges.astype(np.int64)[esel]].astype(np.uint32)
    ecut = np.searchsorted(forest.skeleton_of_vertex(forest.edges[esel, 0].astype(np.int64)), np.arange(nskel + 1))
    xyz, radii, vtypes = forest.xyz[vsel], forest.radii[vsel], forest.vertex_types[vsel]
    out = []
    for k, like in enumerate(forest.skeletons):
        a, b, c, d = vcut[k], vcut[k + 1], ecut[k], ecut[k + 1]
        out.append(_skeleton(like, xyz[a:b], edges[c:d], radii[a:b], vtypes[a:b]) if d > c else Skeleton())
    return out


def unpack_ticks(forest, alive):
    """alive: bool per edge row.  Per skeleton what remove_ticks returns: every vertex kept, the edges that are left in their order; a
    skeleton that keeps no edge comes back as consolidate() leaves an empty one."""
    alive = np.asarray(alive, dtype=bool)
    left = np.concatenate([[0], np.cumsum(alive)])[forest.estart]
    owner = np.repeat(np.arange(len(forest.skeletons)), np.diff(forest.estart))
    edges = (forest.edges.astype(np.int64) - forest.vstart[owner][:, None])[alive].astype(np.uint32)
    out = []
    for k, like in enumerate(forest.skeletons):
        a, b, c, d = forest.vstart[k], forest.vstart[k + 1], left[k], left[k + 1]
        if d == c:
            out.append(Skeleton(segid=like.id, transform=like.transform, space=like.space))
        else:
            out.append(_skeleton(like, forest.xyz[a:b], edges[c:d], forest.radii[a:b], forest.vertex_types[a:b]))
    return out
