"""The numpy / Python statement of csrc/forest.hip, call for call: labels = kh_forest_components, measure =
kh_forest_measure, ticks = kh_forest_ticks with the kernel's own tables (slots, twins, the oriented queue, the superedge records).
No GPU, no library.  host_engine() puts them in the place of the device calls of kimimaro_amd.forest, so that the *_many functions
of kimimaro_amd.post run whole on the CPU; and the skeleton generators of the forest tests.  tick_tables hands out every table of
kh_forest_ticks with the device's dtypes, grown from a sentinel; exact_cable / cable_is_exact state when the f64 cable has one value
in every order of summation (tests/test_gpu_forest_calls.py compares the device with both, word for word)."""
import contextlib
import functools
import math

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


class TickTables:
    """the buffers of kh_forest_ticks after a call, with the device's dtypes: far, twin, rec u32 [2M] and len32 f32 [2M] per slot (the
    four quarters of slot_scratch); arity i32 [V]; queue, ea, eb, sa, sb u32 [C] (the five fifths of rec_scratch), len f64 [C] and
    flag u8 [C] per record; alive u8 [2M].  Beside them what the call was given (row, nbr, upper, crit, crit_start) and, the model's
    own, tail [K]: one past the last record the orientation of each listed component wrote."""
    SLOT = ("far", "twin", "len32", "rec")
    RECORD = ("queue", "ea", "eb", "sa", "sb", "len", "flag")


def filled(n, dtype, fill):
    """n elements of dtype, every byte of them `fill`"""
    return np.full(n * np.dtype(dtype).itemsize, fill, dtype=np.uint8).view(dtype)


def tick_tables(f, m, threshold, fill=0):
    """kh_forest_ticks, write for write -> TickTables.  Every table but arity and alive (which forest_ticks_init_kernel writes whole)
    starts with every byte equal to `fill`, so a word no kernel writes still holds it afterwards: the slots of the vertices that are
    not critical or belong to no listed component, and ea / eb / sa / len of the first record of a component (its queue entry holds
    the start, its sb NONE, its flag 0)."""
    T = TickTables()
    row, nbr, upper = forest.adjacency(f.edges, f.nverts)
    crit, crit_start = forest.critical_lists(m.comp, m.nv, m.ne, m.degree)
    T.row, T.nbr, T.upper, T.crit, T.crit_start = row, nbr, upper, crit, crit_start
    row, nbr = row.astype(np.int64), nbr.astype(np.int64)
    xyz = f.xyz
    ns, nc = nbr.size, crit.size
    deg = np.diff(row)
    T.alive = alive = np.ones(ns, dtype=np.uint8)
    T.arity = arity = np.where(deg >= 3, deg, 0).astype(np.int32)
    T.far, T.twin, T.rec = far, twin, rec = [filled(ns, np.uint32, fill) for _ in range(3)]
    T.len32 = len32 = filled(ns, np.float32, fill)
    T.queue, T.ea, T.eb, T.sa, T.sb = queue, ea, eb, sa, sb = [filled(nc, np.uint32, fill) for _ in range(5)]
    T.len = length = filled(nc, np.float64, fill)
    T.flag = flag = filled(nc, np.uint8, fill)
    T.tail = np.zeros(crit_start.size - 1, dtype=np.int64)

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

    def delete_path(frm, slot, to):
        prev = frm
        while True:
            cur = nbr[slot]
            alive[slot] = 0
            nxt = None
            for q in range(row[cur], row[cur + 1]):
                if nbr[q] == prev:
                    alive[q] = 0
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
        k1, k2 = int(rec[left[0]]), int(rec[left[1]])
        p, sp = (int(eb[k1]), int(sb[k1])) if ea[k1] == x else (int(ea[k1]), int(sa[k1]))
        q, sq = (int(eb[k2]), int(sb[k2])) if ea[k2] == x else (int(ea[k2]), int(sa[k2]))
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
        queue[cs], sb[cs], flag[cs] = crit[terminals[0]], NONE, 0
        head, tail = cs, cs + 1
        while head < tail:
            u, via = int(queue[head]), int(sb[head])
            for s in range(row[u], row[u + 1]):
                if s == via:
                    continue
                child, back = int(far[s]), int(twin[s])
                queue[tail], ea[tail], eb[tail], sa[tail], sb[tail] = child, u, child, s, back
                length[tail] = np.float64(len32[s])
                flag[tail] = LIVE | (REMOVABLE if deg[u] == 1 or deg[child] == 1 else 0)
                rec[s] = rec[back] = tail
                tail += 1
            head += 1
        T.tail[c] = tail
        nlive = tail - cs - 1
        while nlive > 1:
            cand = [(float(length[i]), max(int(ea[i]), int(eb[i])), min(int(ea[i]), int(eb[i])), i)
                    for i in range(cs + 1, tail) if flag[i] == (LIVE | REMOVABLE)]
            if not cand:
                break
            ln, a, b, i = min(cand)
            if (arity[a] == 1 and arity[b] == 1) or ln >= threshold:
                break
            delete_path(int(ea[i]), int(sa[i]), int(eb[i]))
            flag[i] = 0
            arity[a] -= 1
            arity[b] -= 1
            nlive -= 1
            if arity[a] == 2 and fuse(a):
                nlive -= 1
            if arity[b] == 2 and fuse(b):
                nlive -= 1
    return T


def ticks(f, m, threshold):
    """kh_forest_ticks: bool per edge row"""
    if f.nedges == 0:
        return np.zeros(0, dtype=bool)
    T = tick_tables(f, m, threshold)
    return T.alive[T.upper] != 0


def record_lengths(T, fill):
    """the f64 lengths the records of T hold, ascending and distinct; T made with the byte `fill`, which marks the words never written"""
    bits = T.len.view(np.uint64)
    return np.unique(T.len[bits != filled(1, np.uint64, fill)[0]])


def stepwise_thresholds(f, m, fill=0xA5):
    """every midpoint between two successive distinct lengths among the records the model holds after the run at threshold 0 (the
    superedges as the orientation leaves them) and after the run at inf (the fused ones with them)"""
    both = np.unique(np.concatenate([record_lengths(tick_tables(f, m, t, fill), fill) for t in (0.0, np.inf)]))
    return [float(0.5 * (a + b)) for a, b in zip(both[:-1], both[1:])]


# ---- the exact cable ----------------------------------------------------------------------------------------------------------------
def cable_is_exact(lengths):
    """Whether the f64 sum of these float32 lengths is the same number in every order of summation: sum < 2^30 * 2^floor(log2(min)).

    Let e = floor(log2(the smallest length)).  A float32 that is at least 2^e is a whole multiple of its own ulp, which is at least
    u = 2^(e - 23); so every term, and every sum of some of the terms, is a whole multiple k * u.  Such a partial sum is at most the
    whole sum < 2^30 * 2^e = 2^53 * u, so k < 2^53 and k * u is an f64 (53 significant bits; the exponents are far from the ends of
    the f64 range).  Every addition of two partial sums is therefore exact whatever tree or order it is made in -- a scan over
    lanes, atomics in any order, np.add.at -- and each of them ends at math.fsum's result."""
    lengths = np.asarray(lengths, dtype=np.float32).astype(np.float64)
    if lengths.size == 0:
        return True
    smallest = float(lengths.min())
    if not smallest > 0.0 or not np.all(np.isfinite(lengths)):
        return False
    return math.fsum(lengths.tolist()) < 2.0 ** 30 * 2.0 ** (math.frexp(smallest)[1] - 1)


def lengths_by_root(f, comp):
    """{root: the float32 lengths of its edges as f64, in edge order}; an edge belongs to the component of its ends"""
    e = f.edges.astype(np.int64).reshape(-1, 2)
    if e.shape[0] == 0:
        return {}
    root = np.asarray(comp).astype(np.int64)[e[:, 0]]
    order = np.argsort(root, kind="stable")
    lengths = edge_lengths(f.xyz, e).astype(np.float64)[order]
    roots, first = np.unique(root[order], return_index=True)
    return dict(zip(roots.tolist(), np.split(lengths, first[1:])))


def exact_cable(f, comp):
    """f64 [V]: at every root math.fsum (the correctly rounded exact sum) of its component's float32 edge lengths widened to f64; 0
    elsewhere"""
    out = np.zeros(f.nverts, dtype=np.float64)
    for root, lengths in lengths_by_root(f, comp).items():
        out[root] = math.fsum(lengths.tolist())
    return out


def wave_runs(keys):
    """how many runs wave_run_totals forms of these keys laid over waves of 64 lanes: neighbouring equal keys within one wave"""
    keys = np.asarray(keys)
    if keys.size == 0:
        return 0
    head = np.ones(keys.size, dtype=bool)
    head[1:] = keys[1:] != keys[:-1]
    head[::64] = True
    return int(head.sum())


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
    cases["wide_round"] = (wide_round(), (1.5, 2.5, 5.0, 25.0, np.inf))
    cases["hub_100"] = (hub_100(), (25.5, 50.5, 99.5, np.inf))
    # 130 teeth of one length: the `ends` key alone orders them, and every removal fuses the backbone on
    cases["comb_130_equal"] = (comb([(1, 0.5)] * 130), (0.75, np.inf))
    cases["nested_ties"] = (nested_ties(), (20.0, 26.0, np.inf))
    return cases


STEPWISE = ("y_1_2_3", "equal_ticks", "fused_next", "wobbly_start_arm", "wobbly_other_arm", "nested_ties")      # run at every stepwise_thresholds
TABLE_CASES = STEPWISE + ("wide_round", "hub_100", "comb_130_equal")      # the cases whose tables are compared (the model is quick)


def wide_round(arms=70):
    """a hub with `arms` arms, each two edges long and ending in a fork with two leaves, 1 + a / 64 and 3 + a / 64 long: 1 + 4 * arms
    vertices.  The orientation starts at a leaf and reaches the hub in its third round; the fourth holds the arms - 1 other forks
    (for 70 arms: a chunk of 64 lanes and one of 5), whose 2 * (arms - 1) children are placed by the scan over the lanes."""
    v, e = [(0.0, 0.0, 0.0)], []
    for a in range(arms):
        mid, fork = len(v), len(v) + 1
        v += [(10.0, 4.0 * a, 0.0), (20.0, 8.0 * a, 0.0), (20.0, 8.0 * a, 1 + a / 64), (20.0, 8.0 * a, -(3 + a / 64))]
        e += [(0, mid), (mid, fork), (fork, fork + 1), (fork, fork + 2)]
    return Skeleton(np.array(v, dtype=np.float32) + np.float32(100), np.array(e), np.ones(len(v), np.float32), segid=1)


def nested_ties():
    """two ticks of length 25 exactly, the shortest, whose ends nest: (1, 6) around (2, 3).  The key (larger end, smaller end) takes
    (2, 3) first, a key (smaller end, larger end) would take (1, 6) -- teeth in a row (comb) cannot tell the two, their ends ascend
    together.  Taking (2, 3) first fuses the backbone pieces 1-2 and 2-4 (4: a branch with two leaves 200 away) to 10 + 5 = 15,
    the next to go: the backbone is cut there.  Taking (1, 6) first fuses 0-1 and 1-2 to 110, and the backbone stays."""
    v = [(0, 0, 0), (100, 0, 0), (110, 0, 0), (110, 25, 0), (115, 0, 0), (115, 0, 200), (124, 7, 0), (315, 0, 0)]
    e = [(0, 1), (1, 2), (2, 3), (2, 4), (1, 6), (4, 5), (4, 7)]
    return Skeleton(np.array(v, dtype=np.float32), np.array(e), np.ones(8, np.float32), segid=1)


def hub_100(arms=100):
    """one branch point with `arms` arms of one edge, arm k of length k + 1: one lane writes arms - 1 children, and the minimum over
    the records strides past lane 63"""
    out = []
    for k in range(arms):
        arm = np.zeros((1, 3))
        arm[0, k % 3] = (k + 1) * (1 if (k // 3) % 2 == 0 else -1)
        out.append(arm)
    return star(out, centre=(200.0, 200.0, 200.0))


def tick_forest():
    """-> (skeletons, thresholds): 20 random trees of 2..300 vertices for ONE call (many blocks, components whose critical vertices
    start anywhere in the lists), with a path between every five of them: a path has no branch, is not listed, and none of its words
    is written"""
    rng = np.random.default_rng(14)
    skels = []
    for k in range(20):
        skels.append(random_tree(rng, int(rng.integers(2, 301)), extent=16, segid=k))
        if k % 5 == 2:
            skels.append(grid_path(rng, 40 + k, segid=100 + k))
    return skels, (4.0, 12.0, 40.0, np.inf)


# ---- the shapes of the measure tests ----------------------------------------------------------------------------------------------------
def grid_path(rng, nedges, denom=1024, segid=1):
    """a path of nedges edges whose vertices advance along x by about 1 and jump in y and z within [0, 64), all by integer / denom:
    the y and z differences of an edge have up to sixteen significant bits, so their squares round in float32 (a contracted
    multiply-add or a root taken in f64 would show).  Vertex k is the k-th in lexicographic order."""
    n = nedges + 1
    v = np.stack([np.arange(n) * denom + rng.integers(0, denom, size=n), rng.integers(0, 64 * denom, size=n),
                  rng.integers(0, 64 * denom, size=n)], axis=1) / denom
    return Skeleton(v.astype(np.float32), np.stack([np.arange(n - 1), np.arange(1, n)], axis=1), np.ones(n, np.float32), segid=segid)


def pairs(rng, count, denom=1024, extent=64, segid=1):
    """`count` components of two vertices each, in one skeleton: every edge is a component of its own"""
    while True:
        v = rng.integers(0, extent * denom, size=(2 * count, 3)) / denom
        if np.unique(v, axis=0).shape[0] == 2 * count:
            break
    return Skeleton(v.astype(np.float32), np.arange(2 * count).reshape(count, 2), np.ones(2 * count, np.float32), segid=segid)


def braid(rng, nverts=700, denom=1024, segid=1):
    """three paths of nverts vertices side by side: they share every x, their ys lie in [0, 1), [8, 9) and [16, 17).  In
    lexicographic order the vertices of the three alternate, so the edge rows sorted by their smaller vertex alternate between the
    three components: no two neighbouring rows share a root"""
    x = np.arange(nverts) * denom + rng.integers(0, denom, size=nverts)
    v = np.empty((nverts, 3, 3))
    v[:, :, 0] = x[:, None]
    v[:, :, 1] = 8 * denom * np.arange(3)[None, :] + rng.integers(0, denom, size=(nverts, 3))
    v[:, :, 2] = rng.integers(0, 64 * denom, size=(nverts, 3))
    ids = np.arange(3 * nverts).reshape(nverts, 3)
    e = np.stack([ids[:-1].reshape(-1), ids[1:].reshape(-1)], axis=1)
    return Skeleton((v.reshape(-1, 3) / denom).astype(np.float32), e, np.ones(3 * nverts, np.float32), segid=segid)


def hub(rng, leaves=5000, denom=1024, extent=64, segid=1):
    """a hub with `leaves` leaves, the hub in the middle of the lexicographic order: every union and every degree add of the call
    lands on the hub's word, and the root of the component (its smallest vertex) is a leaf"""
    while True:
        v = rng.integers(0, extent * denom, size=(leaves + 1, 3))
        if np.unique(v, axis=0).shape[0] == leaves + 1:
            break
    v = v[np.lexsort((v[:, 2], v[:, 1], v[:, 0]))] / denom
    mid = leaves // 2
    others = np.concatenate([np.arange(mid), np.arange(mid + 1, leaves + 1)])
    return Skeleton(v.astype(np.float32), np.stack([np.full(leaves, mid), others], axis=1), np.ones(leaves + 1, np.float32), segid=segid)


def ring_and_tree(rng, nring=64, ntree=40, denom=1024, segid=1):
    """a ring of nring vertices (on a circle of radius 20, coordinates rounded to integer / denom) and a random tree beside it, in one
    skeleton: ne == nv at the ring's root, ne == nv - 1 at the tree's"""
    t = 2 * np.pi * np.arange(nring) / nring
    ring = np.round(np.stack([20 * np.cos(t), 20 * np.sin(t), np.sin(3 * t)], axis=1) * denom) / denom + 30
    tree = random_tree(rng, ntree, denom=denom, extent=16)
    v = np.concatenate([ring.astype(np.float32), tree.vertices + np.float32(1000)])
    e = np.concatenate([np.stack([np.arange(nring), (np.arange(nring) + 1) % nring], axis=1), tree.edges.astype(np.int64) + nring])
    return Skeleton(v, e, np.ones(v.shape[0], np.float32), segid=segid)


def three_hundred_forests():
    """the skeletons of tests/test_gpu_forest.py's test_three_hundred_random_forests"""
    rng = np.random.default_rng(10)
    return [forest_of(rng, int(rng.integers(1, 7)), 30) for _ in range(300)]


PATH_EDGES = (63, 64, 65, 127, 128, 129, 255, 256, 257)      # runs that end on, before and after a wave (64) and a block (256)


def measure_shapes():
    """name -> the list of skeletons of one kh_forest_measure call, each shape the smallest that reaches its regime"""
    rng = np.random.default_rng(15)
    shapes = {"path_%d" % n: [grid_path(rng, n, segid=n)] for n in PATH_EDGES}
    shapes["pairs_5000"] = [pairs(rng, 5000)]
    shapes["braid_3x700"] = [braid(rng)]
    shapes["hub_5000"] = [hub(rng)]
    shapes["forests_300"] = three_hundred_forests()
    shapes["ring_and_tree"] = [ring_and_tree(rng)]
    shapes["one_edge"] = [Skeleton(np.array([[1.5, 2.25, 3.0], [2.0, 4.5, 3.125]], dtype=np.float32), [[0, 1]], segid=1)]
    return shapes


TREE_SHAPES = tuple("path_%d" % n for n in PATH_EDGES) + ("pairs_5000", "braid_3x700", "hub_5000", "forests_300", "one_edge")


def packed(skeletons):
    """forest.pack of the consolidated skeletons"""
    return forest.pack([s.consolidate() for s in skeletons])


@functools.lru_cache(maxsize=None)
def measure_call(name):
    """-> (forest, measure(forest), exact_cable): one of measure_shapes(), or "all": every shape in one call, so that the runs of a
    shape start at an arbitrary offset of a wave.  Made once; nobody writes to them."""
    shapes = measure_shapes()
    f = packed([s for shape in shapes.values() for s in shape] if name == "all" else shapes[name])
    m = measure(f)
    return f, m, exact_cable(f, m.comp)


@functools.lru_cache(maxsize=None)
def table_call(name):
    """-> (forest, measure(forest), thresholds) of a kh_forest_ticks call whose tables are compared: one of TABLE_CASES, or
    "tick_forest".  Thresholds: 0 (the loop breaks before its first removal: the orientation alone), inf, those of the case, and for
    the STEPWISE cases stepwise_thresholds."""
    skels, thresholds = tick_forest() if name == "tick_forest" else ([tick_cases()[name][0]], tick_cases()[name][1])
    f = packed(skels)
    m = measure(f)
    extra = stepwise_thresholds(f, m) if name in STEPWISE else []
    return f, m, tuple(sorted({0.0, float(np.inf)} | {float(t) for t in thresholds} | set(extra)))


def dust_threshold(f, m):
    """a dust threshold that lies outside the band of every component, twice over (remove_dust_many decides on the device where
    |cable - T| > cable * ne * 2^-23), with components on both sides where there are two different cables: from the host's sums"""
    roots = np.flatnonzero(m.ne)
    cable, ne = m.cable[roots], m.ne[roots].astype(np.float64)
    cuts = np.unique(cable)
    tries = [0.5 * (a + b) for a, b in zip(cuts[:-1], cuts[1:])]
    tries = sorted(tries, key=lambda t: abs(t - float(np.median(cable)))) + [0.5 * float(cuts[0])]
    for t in tries:
        if np.all(np.abs(cable - t) > 2 * cable * ne * 2.0 ** -23):
            return float(t)
    raise AssertionError("no threshold outside every band")
