"""A reference for the predecessor walk of csrc/backtrack.h (backtrack<RAILS>) that shares nothing with it or with the oracle's
ko_walk: the rule of the header comment, restated voxel by voxel in Python on (x, y, z) tuples.  No lanes, no ballots, no marks in
shared bytes, no capacities: a list is the queue, a set the visited marks.

Volumes are (x, y, z), Fortran order, linear index = x + sx * (y + sy * z); distances are those of search_ref.field_fixpoint.

u is an ACHIEVING PREDECESSOR of v when u is a 26-neighbour of v inside the volume, field[u] and dist[u] are finite,
fl32(dist[u] + field[v]) == dist[v], the step u -> v is allowed (with a graph: the bit of the direction from u to v in u's word,
voxel_graphs.GRAPH_BIT) and, on a railroad, field[u] != 0 (a rail is entered, never left)."""
import numpy as np

from voxel_graphs import DIRS, GRAPH_BIT

F32 = np.float32
OPPOSITE = [DIRS.index((-d[0], -d[1], -d[2])) for d in DIRS]


class WalkError(RuntimeError):
    pass


def _as3(a, dtype):
    a = np.asarray(a, dtype=dtype)
    while a.ndim < 3:
        a = a[..., np.newaxis]
    return a


def _lin(p, shape):
    return p[0] + shape[0] * (p[1] + shape[1] * p[2])


def predecessors(f, d, g, v, rails=False):
    """the achieving predecessors of v, in the order of DIRS (u = v + DIRS[k])"""
    shape = f.shape
    dv, fv = d[v], f[v]
    out = []
    for k, e in enumerate(DIRS):
        u = (v[0] + e[0], v[1] + e[1], v[2] + e[2])
        if min(u) < 0 or u[0] >= shape[0] or u[1] >= shape[1] or u[2] >= shape[2]:
            continue
        if not (np.isfinite(f[u]) and np.isfinite(d[u])):
            continue
        if rails and f[u] == 0:
            continue
        if g is not None and not (int(g[u]) >> GRAPH_BIT[OPPOSITE[k]]) & 1:        # u steps to v in the direction opposite to k
            continue
        if F32(d[u] + fv) != dv:
            continue
        out.append(u)
    return out


def _smallest(f, d, cands):
    return min(cands, key=lambda u: (float(d[u]), _lin(u, f.shape)))


def walk(field, dist, start, stop, rails=False, graph=None):
    """(the path from `start` back to `stop`, the search's source, as (x, y, z) tuples; stats).  stats: `plateaus` (plateau searches
    run), `maxq` (the longest queue of one), `maxroute` (the longest route one appended).  WalkError("no rail") / ("plateau")."""
    f = _as3(field, F32)
    d = _as3(dist, F32)
    g = None if graph is None else _as3(graph, np.uint32)
    start, stop = tuple(int(c) for c in start), tuple(int(c) for c in stop)
    stats = dict(plateaus=0, maxq=0, maxroute=0)
    path = [start]
    v = start
    while v != stop:
        if len(path) > f.size:
            raise WalkError("the walk does not end")
        preds = predecessors(f, d, g, v, rails)
        if rails and v == start:                 # the rail end: f[v] == 0, so every achieving predecessor lies at d[v]
            if not preds:
                raise WalkError("no rail")
            v = _smallest(f, d, preds)
            path.append(v)
            continue
        lower = [u for u in preds if d[u] < d[v]]
        if lower:
            v = _smallest(f, d, lower)
            path.append(v)
            continue
        # plateau: every achieving predecessor lies at d[v]
        stats["plateaus"] += 1
        queue, parent, seen = [v], [-1], {v}
        head, found = 0, -1
        while head < len(queue):
            x = queue[head]
            px = predecessors(f, d, g, x, rails)
            if head > 0 and (x == stop or any(d[u] < d[x] for u in px)):
                found = head
                break
            for u in px:
                if d[u] == d[x] and u not in seen:
                    seen.add(u)
                    queue.append(u)
                    parent.append(head)
            head += 1
        stats["maxq"] = max(stats["maxq"], len(queue))
        if found < 0:
            raise WalkError("plateau")
        route = []
        i = found
        while i > 0:
            route.append(queue[i])
            i = parent[i]
        route.reverse()
        stats["maxroute"] = max(stats["maxroute"], len(route))
        path.extend(route)
        v = queue[found]
    return path, stats


def check_path(field, dist, path, graph=None, rails=False, stop=None):
    """a property of any right answer, whatever the tie rule: every step of `path` (start first, as walk returns it) goes to an
    achieving predecessor over an allowed edge, no voxel comes twice, and the path ends at the voxel of distance 0 (`stop`, the
    search's source, when given)"""
    f = _as3(field, F32)
    d = _as3(dist, F32)
    g = None if graph is None else _as3(graph, np.uint32)
    path = [tuple(int(c) for c in p) for p in path]
    assert len(path) >= 1 and len(set(path)) == len(path), "a voxel comes twice"
    for v, u in zip(path, path[1:]):
        assert u in predecessors(f, d, g, v, rails), "%r is no achieving predecessor of %r" % (u, v)
        assert d[u] <= d[v]
    end = path[-1]
    assert d[end] == 0, "the path ends at %r, distance %r" % (end, d[end])
    if stop is not None:                         # (zero weights around the source: more than one voxel lies at distance 0)
        assert end == tuple(int(c) for c in stop)
    if rails:
        assert f[path[0]] == 0 and all(f[p] != 0 for p in path[1:-1])
