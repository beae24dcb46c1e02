"""The numpy / Python statement of csrc/walk.hip, call for call and table for table: orient_tables = kh_walk_orient with
the kernels' own tables (the slots of the critical vertices, the queue of the contracted tree oriented twice, the leaf counts and
offsets, parent / depth), emit_tables = kh_walk_emit (the paths' vertices, the first moving average, the normals -- the second moving
average as the difference of two SEQUENTIAL running sums).  Every table is grown from a sentinel byte, so a word no kernel writes
still holds it.  No GPU, no library.  host_engine() puts the statements in the place of kimimaro_amd.forest's device calls; the
cases of the walk tests are below."""
import contextlib

import numpy as np

from kimimaro_amd import forest, ops
from kimimaro_amd.skeleton import Skeleton
from forest_ref import filled, labels

NONE = 0xFFFFFFFF


class Tables:
    SLOT = ("far", "twin", "hops")
    RECORD = ("qv", "qvia", "qdep", "qcb", "qcc", "qbatch", "qcnt", "qoff")


def orient_tables(w, comp, T, fill=0):
    """kh_walk_orient, write for write.  w: forest.Walk, comp: u32 [V], T: forest.WalkTables -> Tables with far, twin, hops u32
    [nslots] (the thirds of slot_scratch), the eight u32 [ncrit] of rec_scratch, parent, depth u32 [V], path_leaf, path_len u32
    [npaths]"""
    row, nbr = w.row_start.astype(np.int64), w.nbr.astype(np.int64)
    comp = np.asarray(comp).astype(np.int64)
    n, ns, nc, npaths = w.nverts, int(nbr.size), int(T.crit.size), T.npaths
    out = Tables()
    for k in Tables.SLOT:
        setattr(out, k, filled(ns, np.uint32, fill))
    for k in Tables.RECORD:
        setattr(out, k, filled(nc, np.uint32, fill))
    # walk_init_kernel
    out.parent, out.depth = np.full(n, NONE, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
    out.path_leaf, out.path_len = np.full(npaths, NONE, dtype=np.uint32), np.zeros(npaths, dtype=np.uint32)
    out.qv[:] = NONE
    if T.root.size == 0:
        return out
    critical = lambda v: row[v + 1] - row[v] != 2 or comp[v] == v
    # walk_chains_kernel
    for c in T.crit.astype(np.int64).tolist():
        for s in range(row[c], row[c + 1]):
            prev, cur, h = c, int(nbr[s]), 1
            while not critical(cur):
                n0, n1 = int(nbr[row[cur]]), int(nbr[row[cur] + 1])
                prev, cur, h = cur, (n1 if n0 == prev else n0), h + 1
            out.far[s], out.hops[s] = cur, h
            out.twin[s] = [q for q in range(row[cur], row[cur + 1]) if nbr[q] == prev][-1]

    def orient(start, cs, ce):
        out.qv[cs], out.qvia[cs], out.qdep[cs] = start, NONE, 0
        head, tail, nbatch = cs, cs + 1, 0
        while head < tail:
            cnt = min(tail - head, 64)
            out.qbatch[cs + nbatch] = head
            pos = tail
            for i in range(head, head + cnt):                     # lanes in order: the exclusive prefix sum of their children
                u, via = int(out.qv[i]), int(out.qvia[i])
                out.qcb[i] = pos
                for s in range(row[u], row[u + 1]):
                    if s != via:
                        out.qv[pos], out.qvia[pos], out.qdep[pos] = out.far[s], out.twin[s], int(out.qdep[i]) + int(out.hops[s])
                        pos += 1
                out.qcc[i] = pos - int(out.qcb[i])
            nbatch, head, tail = nbatch + 1, head + cnt, pos
        return tail, nbatch

    cstart, lstart = T.crit_start.astype(np.int64), T.leaf_start.astype(np.int64)
    # walk_orient_kernel
    for c in range(T.root.size):
        cs, ce = int(cstart[c]), int(cstart[c + 1])
        tail, _ = orient(int(T.crit[cs]), cs, ce)
        assert tail == ce
        ends = [(int(out.qdep[i]), -int(out.qv[i])) for i in range(cs, ce) if row[int(out.qv[i]) + 1] - row[int(out.qv[i])] == 1]
        root = -max(ends)[1]
        tail, nbatch = orient(root, cs, ce)
        rounds = [(int(out.qbatch[cs + b]), int(out.qbatch[cs + b + 1]) if b + 1 < nbatch else tail) for b in range(nbatch)]
        for lo, hi in reversed(rounds):
            for i in range(lo, hi):
                c0, cc = int(out.qcb[i]), int(out.qcc[i])
                out.qcnt[i] = 1 if cc == 0 else int(out.qcnt[c0:c0 + cc].astype(np.int64).sum())
        out.qoff[cs] = 0
        for lo, hi in rounds:
            for i in range(lo, hi):
                c0, cc, off = int(out.qcb[i]), int(out.qcc[i]), int(out.qoff[i])
                for j in range(c0, c0 + cc):
                    out.qoff[j] = off
                    off += int(out.qcnt[j])
                if cc == 0 and i != cs:
                    out.path_leaf[lstart[c] + off], out.path_len[lstart[c] + off] = out.qv[i], int(out.qdep[i]) + 1
    # walk_fill_kernel
    for i in range(nc):
        cur, slot, d = int(out.qv[i]), int(out.qvia[i]), int(out.qdep[i])
        if cur == NONE or slot == NONE:
            continue
        while True:
            nxt = int(nbr[slot])
            out.parent[cur], out.depth[cur] = nxt, d
            if critical(nxt):
                break
            slot = row[nxt] + 1 if nbr[row[nxt]] == cur else row[nxt]
            cur, d = nxt, d - 1
    return out


def reflect(j, length):
    """np.pad(mode="symmetric"): the index in [0, length) that position j of the endless reflection holds"""
    r = j % (2 * length)
    return r if r < length else 2 * length - 1 - r


def differences(vox, path):
    """d_j = vox[next] - vox[this] along the path, the last one repeated: int64 [L, 3]"""
    pts = vox[path]
    d = pts[1:] - pts[:-1]
    return np.concatenate([d, d[-1:]])


def first_pass(d, n):
    """the first moving average: f64 [L, 3], sums of integers"""
    L = d.shape[0]
    out = np.zeros((L, 3), dtype=np.float64)
    for i in range(L):
        total = np.zeros(3, dtype=np.int64)
        for j in range(i + 1 - n, i + 1):
            total += d[reflect(j, L)]
        out[i] = total.astype(np.float64) / np.float64(n)
    return out


def second_pass(first, n, window_sum=False):
    """the second moving average, over the reversed first and reversed back: R the sequential running sum of the padded input, one
    rounding per addition, out = (R[i + n] - R[i]) / n.  window_sum=True: the sum over the window itself instead -- NOT what numpy
    computes (the tests show the difference)."""
    L = first.shape[0]
    b = first[::-1]
    padded = np.array([b[reflect(q - n, L)] for q in range(L + 2 * n)], dtype=np.float64)
    out = np.zeros((L, 3), dtype=np.float64)
    if window_sum:
        for i in range(L):
            total = np.zeros(3, dtype=np.float64)
            for q in range(i + 1, i + n + 1):
                total = total + padded[q]
            out[i] = total / np.float64(n)
    else:
        running = np.zeros_like(padded)
        acc = padded[0].copy()
        running[0] = acc
        for q in range(1, padded.shape[0]):
            acc = acc + padded[q]
            running[q] = acc
        for i in range(L):
            out[i] = (running[n + i] - running[i]) / np.float64(n)
    return out[::-1]


def unit(v):
    with np.errstate(invalid="ignore", divide="ignore"):
        return v / np.sqrt(((v[:, 0] * v[:, 0]) + (v[:, 1] * v[:, 1])) + (v[:, 2] * v[:, 2]))[:, None]


def emit_tables(parent, path_leaf, pstart, vox, window, fill=0):
    """kh_walk_emit, write for write -> (occ_vertex u32 [m], normal f64 [m, 3] or None, first f64 [m, 3] or None)"""
    pstart = np.asarray(pstart, dtype=np.int64)
    m = int(pstart[-1])
    occ = filled(m, np.uint32, fill)
    for p in range(pstart.size - 1):
        cur = int(path_leaf[p])
        for k in range(int(pstart[p + 1]) - 1, int(pstart[p]) - 1, -1):
            occ[k] = cur
            cur = int(parent[cur]) if cur != NONE else NONE
    if not window:
        return occ, None, None
    normal = filled(3 * m, np.float64, fill).reshape(-1, 3)
    first = filled(3 * m, np.float64, fill).reshape(-1, 3) if window > 1 else None
    vox = np.asarray(vox, dtype=np.int64).reshape(-1, 3)
    for p in range(pstart.size - 1):
        a, b = int(pstart[p]), int(pstart[p + 1])
        d = differences(vox, occ[a:b].astype(np.int64))
        if window == 1:
            normal[a:b] = unit(d.astype(np.float32)).astype(np.float64)
        else:
            first[a:b] = first_pass(d, window)
            normal[a:b] = unit(second_pass(first[a:b], window))
    return occ, normal, first


# ---- in the device's place ------------------------------------------------------------------------------------------------------------
class _Host:
    """stands where an Engine stands in kimimaro_amd.forest's device calls"""


def _labels(eng, w):
    w.dev["comp"] = labels(w.edges, w.nverts)
    return w.dev["comp"]


def _orient(eng, w, tables):
    T = orient_tables(w, w.dev["comp"], tables)
    w.dev["parent"], w.dev["leaf"] = T.parent, T.path_leaf
    return T.path_len


def _emit(eng, w, first, last, pstart, vox, window):
    occ, normal, _ = emit_tables(w.dev["parent"], w.dev["leaf"][first:last], pstart, vox, window)
    return occ, normal


@contextlib.contextmanager
def host_engine():
    """kimimaro_amd.forest's walk_labels, walk_orient and walk_emit, and ops.engine, replaced by the statements above"""
    saved = forest.walk_labels, forest.walk_orient, forest.walk_emit, ops.engine
    forest.walk_labels, forest.walk_orient, forest.walk_emit, ops.engine = _labels, _orient, _emit, lambda: _Host()
    try:
        yield
    finally:
        forest.walk_labels, forest.walk_orient, forest.walk_emit, ops.engine = saved


# ---- the cases ----------------------------------------------------------------------------------------------------------------------
def skeleton(vertices, edges, **kw):
    return Skeleton(np.asarray(vertices, dtype=np.float32).reshape(-1, 3), np.asarray(edges, dtype=np.uint32).reshape(-1, 2), **kw)


def line(n, order=None):
    """a chain of n vertices along x; order: the vertex numbers along the chain (default 0 .. n-1)"""
    order = np.arange(n) if order is None else np.asarray(order)
    v = np.zeros((n, 3), dtype=np.float32)
    v[order, 0] = np.arange(n)
    return skeleton(v, np.stack([order[:-1], order[1:]], axis=1))


def star(arms):
    """vertex 0 in the middle, arms 1 .. arms around it"""
    ang = 2 * np.pi * np.arange(arms) / arms
    v = np.concatenate([[[50, 50, 0]], np.stack([50 + 40 * np.cos(ang), 50 + 40 * np.sin(ang), 1 + np.arange(arms) % 5], axis=1)])
    return skeleton(v, [[0, k] for k in range(1, arms + 1)])


def comb(teeth):
    """a spine of `teeth` vertices along x with a tooth of one vertex on every one of them: teeth - 2 branch points and teeth leaves
    in one component"""
    v = [[k, 0, 0] for k in range(teeth)] + [[k, 1, 0] for k in range(teeth)]
    e = [[k, k + 1] for k in range(teeth - 1)] + [[k, teeth + k] for k in range(teeth)]
    return skeleton(v, e)


def random_walk(rng, n):
    """a chain of n vertices, each one voxel step (any of the 26) from the last"""
    steps = rng.integers(-1, 2, size=(n - 1, 3))
    steps[np.all(steps == 0, axis=1), 0] = 1
    v = np.concatenate([[[30, 30, 30]], 30 + np.cumsum(steps, axis=0)])
    return skeleton(v, [[k, k + 1] for k in range(n - 1)])


def interleaved(rng, ncomp, nmax, isolated):
    """ncomp random trees whose vertex numbers are shuffled together, `isolated` vertices without an edge in between"""
    sizes = [int(rng.integers(2, nmax + 1)) for _ in range(ncomp)]
    total = sum(sizes) + isolated
    number = rng.permutation(total)
    v = rng.integers(0, 60, size=(total, 3)).astype(np.float32)
    e, at = [], 0
    for size in sizes:
        mine = number[at:at + size]
        e += [[mine[int(rng.integers(0, k))], mine[k]] for k in range(1, size)]
        at += size
    return skeleton(v, e)


def order_tree():
    """ascending-neighbour order differs from depth order: from the root 5 the walk meets the branch 1, whose neighbours ascend as
    0 (a long arm), 2 (a short one), 5 (the way back); and the branch's parent is its LARGEST neighbour"""
    v = [[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 2, 0], [0, 3, 0], [9, 0, 0], [0, 4, 0], [3, 0, 0], [5, 0, 0], [7, 0, 0]]
    e = [[1, 0], [0, 3], [3, 4], [4, 6], [1, 2], [1, 7], [7, 8], [8, 9], [9, 5]]
    return skeleton(v, e)


def middle_chain():
    """a chain whose smallest vertex is in the middle, both ends equally far: 3 - 1 - 0 - 2 - 4; the root is the smaller end"""
    return line(5, [3, 1, 0, 2, 4])


def untidy(rng):
    """non-consolidated rows: repeated, reversed, shuffled, with self loops; vertex 0 has no edge"""
    base = interleaved(rng, 3, 12, 2)
    e = base.edges.astype(np.int64)
    n = base.vertices.shape[0]
    e = np.concatenate([e, e[::2, ::-1], e[:3], [[k, k] for k in range(0, n, 3)]])
    return skeleton(base.vertices, e[rng.permutation(e.shape[0])])


def ring_and_tree():
    """one cyclic component (a ring of 6) and one tree (a fork) in one skeleton"""
    ring = [[k, (k + 1) % 6] for k in range(6)]
    fork = [[6, 7], [7, 8], [7, 9]]
    v = [[10 + 3 * np.cos(k), 10 + 3 * np.sin(k), 2] for k in range(6)] + [[20, 20, 5], [21, 20, 5], [22, 21, 5], [22, 19, 5]]
    return skeleton(v, ring + fork)


def path_cases():
    """name -> list of skeletons, for paths_many against Skeleton.paths"""
    rng = np.random.default_rng(23)
    cases = {
        "one_edge": [skeleton([[0, 0, 0], [1, 0, 0]], [[0, 1]])],
        "middle_chain": [middle_chain()],
        "chain_65": [line(65)], "chain_257": [line(257, np.random.default_rng(1).permutation(257))], "chain_1000": [line(1000)],
        "star_3": [star(3)], "star_70": [star(70)],
        "comb_130": [comb(130)],
        "order_tree": [order_tree()],
        "three_interleaved": [interleaved(rng, 4, 40, 3), interleaved(rng, 3, 90, 5), interleaved(rng, 5, 20, 1)],
        "empty_in_the_middle": [star(4), Skeleton(), skeleton([[1, 2, 3], [4, 5, 6]], np.zeros((0, 2))), order_tree()],
        "untidy": [untidy(rng), untidy(rng)],
        "ring_and_tree": [star(3), ring_and_tree(), line(4)],
    }
    return cases


TREE_CASES = ("one_edge", "middle_chain", "chain_65", "chain_257", "chain_1000", "star_3", "star_70", "comb_130", "order_tree",
              "three_interleaved", "empty_in_the_middle", "untidy")


def same_paths(got, want):
    return len(got) == len(want) and all(a.dtype == b.dtype and np.array_equal(a, b) for a, b in zip(got, want))


def zigzag(n):
    """+x, -x, ...: at window 2 the smoothing cancels to zero"""
    v = np.zeros((n, 3), dtype=np.float32)
    v[:, 0] = 10 + np.arange(n) % 2
    v[:, 1] = 10
    return skeleton(v, [[k, k + 1] for k in range(n - 1)])


SHAPE = (48, 40, 44)


def occurrence_cases():
    """name -> (jobs, anisotropy f32 [3], shape, windows, steps): jobs of (skeleton, word, offset) for _xs_occurrences_many against
    _xs_occurrences"""
    rng = np.random.default_rng(29)
    one = np.ones(3, dtype=np.float32)
    aniso = np.array([16, 16, 40], dtype=np.float32)
    job = lambda *skels, offset=(0, 0, 0): [(s, k + 1, offset) for k, s in enumerate(skels)]
    windows = (1, 2, 3, 5, 7)
    twin = skeleton([[5, 5, 5], [6, 5, 5], [6.2, 5.1, 5], [7, 5, 5]], [[0, 1], [1, 2], [2, 3]])          # vertices 1 and 2 share a voxel
    shared = skeleton([[5, 5, 5], [6, 5, 5], [7, 6, 5], [7, 4, 5], [7.3, 6.2, 5.1], [8, 7, 5]],          # 4 hangs on 3 and lies in the voxel
                      [[0, 1], [1, 2], [1, 3], [3, 4], [2, 5]])                                           # of 2: two paths, one voxel
    outside = skeleton([[-2, 5, 5], [-1, 5, 5], [0, 5, 5], [1, 5, 5], [1, -1, 5], [1, 40, 5], [48, 5, 5], [1, 5, -1], [1, 5, 44], [1, 6, 5]],
                       [[0, 1], [1, 2], [2, 3], [3, 4], [3, 9], [9, 5], [3, 6], [3, 7], [3, 8]])
    physical = random_walk(rng, 40)
    physical.vertices = physical.vertices * aniso
    physical.space = "physical"
    cases = {
        "twin_voxel": (job(twin), one, SHAPE, windows, (1,)),
        "zigzag": (job(zigzag(9)), one, SHAPE, (1, 2, 3), (1,)),
        "shared_voxel": (job(shared), one, SHAPE, (1, 3), (1, 2)),
        "outside": (job(outside), one, SHAPE, (1, 2), (1, 2, 3)),
        "lengths": (job(*[line(L) for L in (2, 3, 4, 6, 7)]), one, SHAPE, (1, 2), (1, 2, 3)),
        "short_wide": (job(line(2), line(3), order_tree()), one, SHAPE, windows, (1,)),
        "random_walk_60": (job(random_walk(rng, 60)), one, SHAPE, windows, (1, 3)),
        "physical": (job(physical, random_walk(rng, 30), offset=(2, 1, 3)), aniso, SHAPE, (1, 3), (1, 2)),
        "trees": (job(star(5), comb(9), interleaved(rng, 3, 30, 2)), one, (101, 101, 61), (1, 3), (1, 3)),
        "cyclic_between": (job(star(3), ring_and_tree(), line(4)), one, SHAPE, (1, 3), (1,)),
    }
    return cases


def bits(a):
    """an f64 array with every NaN made the same word: NaNs compare by position"""
    a = np.array(a, dtype=np.float64)
    a[np.isnan(a)] = np.nan
    return a.view(np.uint64)
