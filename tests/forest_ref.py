"""The numpy / Python statement of csrc/forest.hip, call for call: labels = kh_forest_components, measure =
kh_forest_measure, ticks = kh_forest_ticks with the kernel's own tables (slots, twins, the oriented queue, the superedge records).
No GPU, no library.  host_engine() puts them in the place of the device calls of kimimaro_amd.forest, so that the *_many functions
of kimimaro_amd.post run whole on the CPU; and the skeleton generators of the forest tests."""
import contextlib

import numpy as np

from kimimaro_amd import forest, ops
from kimimaro_amd.skeleton import Skeleton

NONE = 0xFFFFFFFF
LIVE, REMOVABLE = 1, 2


def labels(edges, nverts):
    """comp[v] = the smallest vertex connected to v"""
    comp = np.arange(nverts, dtype=np.int64)
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    while True:
        before = comp.copy()
        np.minimum.at(comp, e[:, 0], before[e[:, 1]])
        np.minimum.at(comp, e[:, 1], before[e[:, 0]])
        comp = comp[comp]
        if np.array_equal(comp, before):
            return comp.astype(np.uint32)


def edge_lengths(xyz, edges):
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    d = (xyz[e[:, 1]] - xyz[e[:, 0]]).astype(np.float32)
    d = d * d
    return np.sqrt(((d[:, 0] + d[:, 1]) + d[:, 2]).astype(np.float32))


def measure(f):
    """forest.Measures as kh_forest_measure fills them (the f64 sum in edge order)"""
    n = f.nverts
    comp = labels(f.edges, n)
    e = f.edges.astype(np.int64)
    nv = np.bincount(comp, minlength=n).astype(np.uint32)
    ne = np.bincount(comp[e[:, 0]], minlength=n).astype(np.uint32)
    cable = np.zeros(n, dtype=np.float64)
    np.add.at(cable, comp[e[:, 0]], edge_lengths(f.xyz, e).astype(np.float64))
    degree = np.bincount(e.reshape(-1), minlength=n).astype(np.uint32)
    return forest.Measures(comp, nv, ne, cable, degree)


def ticks(f, m, threshold):
    """kh_forest_ticks: bool per edge row"""
    if f.nedges == 0:
        return np.zeros(0, dtype=bool)
    row, nbr, upper = forest.adjacency(f.edges, f.nverts)
    crit, crit_start = forest.critical_lists(m.comp, m.nv, m.ne, m.degree)
    row, nbr = row.astype(np.int64), nbr.astype(np.int64)
    xyz = f.xyz
    ns = nbr.size
    alive = np.ones(ns, dtype=bool)
    deg = np.diff(row)
    arity = np.where(deg >= 3, deg, 0).astype(np.int64)
    far, twin, rec = np.zeros(ns, np.int64), np.zeros(ns, np.int64), np.zeros(ns, np.int64)
    len32 = np.zeros(ns, np.float32)

    def step(a, b):
        d = xyz[b] - xyz[a]
        d = d * d
        return np.sqrt(np.float32(np.float32(d[0] + d[1]) + d[2]))

    for c in crit.tolist():                       # forest_chains_kernel
        for s in range(row[c], row[c + 1]):
            prev, cur = c, nbr[s]
            dist = np.float32(np.float32(0.0) + step(prev, cur))
            while deg[cur] == 2:
                n0, n1 = nbr[row[cur]], nbr[row[cur] + 1]
                nxt = n1 if n0 == prev else n0
                dist = np.float32(dist + step(cur, nxt))
                prev, cur = cur, nxt
            far[s], len32[s] = cur, dist
            twin[s] = next(q for q in range(row[cur], row[cur + 1]) if nbr[q] == prev)
    nc = crit.size
    queue, ea, eb, sa, sb = (np.zeros(nc, np.int64) for _ in range(5))
    length = np.zeros(nc, np.float64)
    flag = np.zeros(nc, np.int64)

    def delete_path(frm, slot, to):
        prev = frm
        while True:
            cur = nbr[slot]
            alive[slot] = False
            nxt = None
            for q in range(row[cur], row[cur + 1]):
                if nbr[q] == prev:
                    alive[q] = False
                elif alive[q]:
                    nxt = q
            if cur == to or nxt is None:
                return
            prev, slot = cur, nxt

    def fuse(x):
        left = [q for q in range(row[x], row[x + 1]) if alive[q]]
        arity[x] = 0
        if len(left) != 2:
            return False
        k1, k2 = rec[left[0]], rec[left[1]]
        p, sp = (eb[k1], sb[k1]) if ea[k1] == x else (ea[k1], sa[k1])
        q, sq = (eb[k2], sb[k2]) if ea[k2] == x else (ea[k2], sa[k2])
        ea[k1], sa[k1], eb[k1], sb[k1] = p, sp, q, sq
        length[k1] = (0.0 + length[k1]) + length[k2]
        flag[k1], flag[k2] = LIVE | REMOVABLE, 0
        rec[sq] = k1
        return True

    for c in range(crit_start.size - 1):          # forest_ticks_kernel, one wave each
        cs, ce = int(crit_start[c]), int(crit_start[c + 1])
        if ce < cs + 2:
            continue
        terminals = [k for k in range(cs, ce) if deg[crit[k]] == 1]
        if not terminals:
            continue
        queue[cs], sb[cs] = crit[terminals[0]], NONE
        head, tail = cs, cs + 1
        while head < tail:
            u, via = queue[head], sb[head]
            for s in range(row[u], row[u + 1]):
                if s == via:
                    continue
                child, back = far[s], twin[s]
                queue[tail], ea[tail], eb[tail], sa[tail], sb[tail] = child, u, child, s, back
                length[tail] = np.float64(len32[s])
                flag[tail] = LIVE | (REMOVABLE if deg[u] == 1 or deg[child] == 1 else 0)
                rec[s] = rec[back] = tail
                tail += 1
            head += 1
        nlive = tail - cs - 1
        while nlive > 1:
            cand = [(length[i], max(ea[i], eb[i]), min(ea[i], eb[i]), i) for i in range(cs + 1, tail) if flag[i] == (LIVE | REMOVABLE)]
            if not cand:
                break
            ln, a, b, i = min(cand)
            if (arity[a] == 1 and arity[b] == 1) or ln >= threshold:
                break
            delete_path(ea[i], sa[i], eb[i])
            flag[i] = 0
            arity[a] -= 1
            arity[b] -= 1
            nlive -= 1
            if arity[a] == 2 and fuse(a):
                nlive -= 1
            if arity[b] == 2 and fuse(b):
                nlive -= 1
    return alive[upper]


class _Host:
    """stands where an Engine stands in kimimaro_amd.forest's device calls"""


@contextlib.contextmanager
def host_engine():
    """kimimaro_amd.forest's three device calls and ops.engine replaced by the statements above"""
    saved = forest.labels, forest.measure, forest.ticks, ops.engine
    forest.labels = lambda eng, f: labels(f.edges, f.nverts)
    forest.measure = lambda eng, f: measure(f)
    forest.ticks = lambda eng, f, m, threshold: ticks(f, m, threshold)
    ops.engine = lambda: _Host()
    try:
        yield
    finally:
        forest.labels, forest.measure, forest.ticks, ops.engine = saved


# ---- generators -------------------------------------------------------------------------------------------------------------------
def random_tree(rng, n, denom=1024, extent=64, segid=1):
    """a random-attachment tree of n >= 2 vertices: vertex k hangs on a uniformly drawn earlier one; coordinates integer / denom,
    distinct; radii uniform in [0.5, 3]"""
    while True:
        v = (rng.integers(0, extent * denom, size=(n, 3)) / denom).astype(np.float32)
        if np.unique(v, axis=0).shape[0] == n:
            break
    e = np.stack([np.array([int(rng.integers(0, k)) for k in range(1, n)]), np.arange(1, n)], axis=1)
    return Skeleton(v, e, rng.uniform(0.5, 3, size=n).astype(np.float32), segid=segid)


def forest_of(rng, ntrees, nmax, **kw):
    """ntrees random trees of 2..nmax vertices merged into one skeleton (kept apart in space so that no vertices coincide)"""
    trees = []
    for k in range(ntrees):
        t = random_tree(rng, int(rng.integers(2, nmax + 1)), **kw)
        t.vertices = t.vertices + np.float32(1000 * k)
        trees.append(t)
    return Skeleton.simple_merge(trees)


def same(a, b):
    """join_ref.same plus id, space and transform"""
    return (a.vertices.shape == b.vertices.shape and np.array_equal(a.vertices, b.vertices) and np.array_equal(a.radii, b.radii)
            and a.edges.shape == b.edges.shape and np.array_equal(a.edges, b.edges) and a.edges.dtype == b.edges.dtype
            and a.id == b.id and a.space == b.space and np.array_equal(a.transform, b.transform))


def star(arms, centre=(100.0, 100.0, 100.0), segid=1):
    """a branch point with arms: each arm a (k, 3) array of offsets from the centre, in walk order from the centre outward"""
    v = [np.asarray(centre, dtype=np.float64)[None]]
    e = []
    n = 1
    for arm in arms:
        arm = np.asarray(arm, dtype=np.float64).reshape(-1, 3)
        v.append(arm + v[0])
        ids = np.concatenate([[0], np.arange(n, n + arm.shape[0])])
        e.append(np.stack([ids[:-1], ids[1:]], axis=1))
        n += arm.shape[0]
    return Skeleton(np.concatenate(v).astype(np.float32), np.concatenate(e), np.ones(n, np.float32), segid=segid)


def straight(axis, sign, count, step=1.0):
    """`count` offsets along an axis, `step` apart"""
    out = np.zeros((count, 3))
    out[:, axis] = sign * step * np.arange(1, count + 1)
    return out


def wobbly(rng, axis, sign, count, denom=1024):
    """`count` offsets that advance one unit along an axis and wander in the other two by integer / denom: float32 sums of the edge
    lengths depend on the direction they are accumulated in"""
    out = rng.integers(-denom, denom + 1, size=(count, 3)) / denom
    out[:, axis] = 0
    out = np.cumsum(out, axis=0)
    out[:, axis] = sign * np.arange(1, count + 1)
    return out


def directed_sums(skel_path):
    """the float32 sums of a vertex path's edge lengths accumulated from its first vertex and from its last"""
    v = np.asarray(skel_path, dtype=np.float32)
    steps = edge_lengths(v, np.stack([np.arange(len(v) - 1), np.arange(1, len(v))], axis=1))
    fwd = bwd = np.float32(0.0)
    for s in steps:
        fwd = np.float32(fwd + s)
    for s in steps[::-1]:
        bwd = np.float32(bwd + s)
    return float(fwd), float(bwd)


def comb(teeth, end=5.0, segid=1):
    """a backbone along x, one unit between its nodes, `end` long at both ends; tooth k, of teeth[k] edges of length teeth_len[k],
    hangs on backbone node k + 1.  teeth: a list of (edges, edge length)."""
    n = len(teeth)
    xs = np.concatenate([[0.0], end + np.arange(n), [end + n - 1 + end]])
    v = [np.stack([xs, np.zeros_like(xs), np.zeros_like(xs)], axis=1)]
    e = [np.stack([np.arange(n + 1), np.arange(1, n + 2)], axis=1)]
    nxt = n + 2
    for k, (count, length) in enumerate(teeth):
        ys = length * np.arange(1, count + 1)
        v.append(np.stack([np.full(count, xs[k + 1]), ys, np.zeros(count)], axis=1))
        ids = np.concatenate([[k + 1], np.arange(nxt, nxt + count)])
        e.append(np.stack([ids[:-1], ids[1:]], axis=1))
        nxt += count
    return Skeleton(np.concatenate(v).astype(np.float32), np.concatenate(e), np.ones(nxt, np.float32), segid=segid)


def tick_cases():
    """name -> (skeleton, thresholds): the trees of the tick tests"""
    rng = np.random.default_rng(11)
    cases = {}
    cases["y_1_2_3"] = (star([straight(0, 1, 1), straight(1, 1, 2), straight(2, 1, 3)]), (0.5, 1.5, 2.5, 10.0))
    cases["equal_ticks"] = (star([straight(0, 1, 2), straight(1, 1, 2), straight(2, 1, 5), straight(0, -1, 5)]), (1.0, 2.5, 10.0))
    # the short tooth goes first; the backbone superedge fused there (length 2) is then the shortest and its removal cuts the backbone
    cases["fused_next"] = (comb([(1, 3.0), (1, 3.0), (1, 0.5), (1, 3.0), (1, 3.0)]), (1.0, 2.5, 3.5, 100.0))
    for name, sign in (("wobbly_start_arm", -1), ("wobbly_other_arm", 1)):
        while True:                               # (a draw whose two sums coincide is drawn again)
            skel = star([wobbly(rng, 0, sign, 400), straight(0, -sign, 2, 300.0), straight(1, 1, 2, 300.0)])
            fwd, bwd = directed_sums(skel.vertices[:401])
            if fwd != bwd:
                break
        cases[name] = (skel, (0.5 * (fwd + bwd), min(fwd, bwd), max(fwd, bwd)))
    cases["comb_4100"] = (comb([(1, 0.5 if k % 41 == 0 else 3.0) for k in range(4100)]), (0.75,))
    cases["tick_10000"] = (star([straight(0, 1, 10000), straight(1, 1, 1, 20000.0), straight(2, 1, 1, 30000.0)]), (15000.0,))
    return cases
