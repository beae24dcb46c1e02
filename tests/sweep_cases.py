"""The calls of kh_invalidate_ball that tests/test_sweep_model_host.py classifies with the abstract machine (tests/sweep_ref.py)
and tests/test_gpu_sweep_calls.py runs on the device: test infrastructure.

A case is a Case(name, mask, an, path, dbf, scale, const, graph): one call of roll_invalidation_ball_inside_component.
`judge(case)` runs the oracle and the model on it ONCE per process and keeps the verdict (neither input nor verdict is changed by
anybody afterwards)."""
import os
from types import SimpleNamespace

import numpy as np

import sweep_ref
from shapes import random_walk_tube

HERE = os.path.dirname(os.path.abspath(__file__))
ANISOTROPIES = ((1, 1, 1), (16, 16, 40), (4, 4, 40), (1, 2, 3), (0.5, 1.25, 3.0))
ALL_EDGES = (1 << 26) - 1
CORNER_BITS = sum(1 << b for b in sweep_ref.GRAPH_BIT[18:26])


def Case(name, mask, an, path, dbf, scale=1.0, const=0.0, graph=None):
    mask = np.asfortranarray(mask, dtype=np.uint8)
    path = np.asarray(path, dtype=np.int64).reshape(-1, 3)
    return SimpleNamespace(name=name, mask=mask, an=tuple(float(v) for v in an), path=path,
                           dbf=np.asfortranarray(dbf, dtype=np.float32), scale=float(scale), const=float(const),
                           graph=None if graph is None else np.asfortranarray(graph, dtype=np.uint32))


def locs_of(case):
    sx, sy = case.mask.shape[0], case.mask.shape[1]
    return case.path[:, 0] + sx * (case.path[:, 1] + sy * case.path[:, 2])


def radii_of(case):
    return sweep_ref.ball_radii(case.dbf, locs_of(case), case.scale, case.const)


def with_radii(name, mask, an, path, radii, graph=None):
    """a case whose ball radii are given per path vertex (scale 1, const 0); a voxel named twice takes its last radius"""
    dbf = np.zeros(mask.shape, np.float32, order="F")
    path = np.asarray(path, dtype=np.int64).reshape(-1, 3)
    dbf[path[:, 0], path[:, 1], path[:, 2]] = np.asarray(radii, dtype=np.float32)
    return Case(name, mask, an, path, dbf, graph=graph)


def integral(an):
    return all(float(v) == int(v) and v >= 1 for v in an)


_verdicts = {}


def judge(case):
    """Verdict of oracle and model on a case: after (the oracle's mask), count, dead (the oracle's dead set), model, cls"""
    got = _verdicts.get(case.name)
    if got is None:
        import oracle
        after = case.mask.copy(order="F")
        count, _ = oracle.roll_invalidation_ball_inside_component(after, case.dbf, case.scale, case.const, case.an,
                                                                  [tuple(int(v) for v in p) for p in case.path],
                                                                  voxel_connectivity_graph=case.graph)
        model = sweep_ref.sweep_model(case.mask, case.an, case.path, radii_of(case), graph=case.graph)
        dead = np.flatnonzero((case.mask.reshape(-1, order="F") != 0) & (after.reshape(-1, order="F") == 0))
        got = _verdicts[case.name] = SimpleNamespace(after=after, count=int(count), dead=dead, model=model,
                                                     cls=sweep_ref.classify(model))
        assert got.count == dead.size
    return got


def check_soundness(case):
    """D <= the oracle's dead set <= D u M; certified: D is the oracle's dead set.  Returns the verdict."""
    v = judge(case)
    D, M = set(v.model.D.tolist()), set(v.model.M.tolist())
    dead = set(v.dead.tolist())
    assert D <= dead, (case.name, "the model kills voxels the reference keeps", sorted(D - dead)[:8])
    assert dead <= D | M, (case.name, "the reference kills voxels the model never reached", sorted(dead - D - M)[:8])
    if v.model.certified:
        assert D == dead and v.model.count == v.count, case.name
    return v


# ---- the recorded vectors of the compiled reference ------------------------------------------------------------------------------
def _unpack(b, shape):
    return np.unpackbits(b)[: int(np.prod(shape))].reshape(shape, order="F").astype(np.uint8)


_golden = {}


def goldens(graph):
    """the vectors of tests/golden/invalidation_ball.npz (graph=False: 60) or invalidation_ball_graph.npz (53) as cases, with the
    recorded result: [(case, after, count)]"""
    if graph not in _golden:
        fn = "invalidation_ball_graph.npz" if graph else "invalidation_ball.npz"
        z = np.load(os.path.join(HERE, "golden", fn))
        out = []
        for i in range(int(z["n"])):
            shape = tuple(int(v) for v in z["shape_%d" % i])
            path = z["path_%d" % i].astype(np.int64)
            dbf = np.zeros(shape, np.float32, order="F")
            dbf[path[:, 0], path[:, 1], path[:, 2]] = z["dbfpath_%d" % i]
            scale, const = (float(v) for v in z["sc_%d" % i])
            vcg = z["graph_%d" % i].reshape(shape, order="F") if graph else None
            c = Case("golden%s_%d" % ("_graph" if graph else "", i), _unpack(z["mask_%d" % i], shape), z["an_%d" % i], path, dbf,
                     scale, const, vcg)
            out.append((c, _unpack(z["after_%d" % i], shape), int(z["count_%d" % i])))
        _golden[graph] = out
    return _golden[graph]


# ---- random tubes -------------------------------------------------------------------------------------------------------------------
def _edt(mask, an):
    import oracle
    return np.asfortranarray(oracle.edt(mask, an, black_border=bool(np.all(mask))), dtype=np.float32)


TUBE_SPECS = (
    # (seed, anisotropy, path kind, scale, const in units of the smallest spacing, special)
    (1500, 0, "run", 1.5, 2.0, None), (1501, 1, "scat", 3.0, 0.0, None), (1502, 2, "run", 0.5, 6.0, None),
    (1503, 3, "scat", 2.0, 0.7, None), (1504, 4, "run", 1.5, 2.0, None), (1505, 0, "scat", 3.0, 2.0, None),
    (1506, 1, "run", 1.5, 2.0, None), (1507, 2, "scat", 2.0, 0.0, None), (1508, 3, "run", 1.5, 6.0, None),
    (1509, 4, "scat", 0.5, 6.0, None),
    # seeds found by search: the model leaves voxels in M on these
    (1515, 0, "run", 1.5, 2.0, None), (1526, 0, "scat", 1.5, 2.0, None), (1523, 3, "run", 1.5, 2.0, None),
    (1510, 0, "run", 1.5, 2.0, "dup"), (1511, 1, "scat", 1.5, 2.0, "dup"), (1512, 2, "run", 1.5, 2.0, "deadvertex"),
    (1513, 3, "scat", 1.5, 2.0, "deadvertex"), (1514, 1, "run", 1.0, -2.0, "nonpositive"), (1516, 4, "scat", 1.5, 2.0, "dup"),
)


def tubes():
    """tubes of sides 14-30 as make_golden.gen_ball draws them, under five anisotropies (the last one is not integral: table mode
    only); paths are contiguous runs of the voxel list and scattered voxels; some carry a vertex twice, a vertex the mask has lost
    already, or vertices with a radius of 0 and below 0"""
    out = []
    for seed, ai, kind, scale, cu, special in TUBE_SPECS:
        an = ANISOTROPIES[ai]
        rng = np.random.default_rng(seed)
        shape = (int(rng.integers(14, 31)), int(rng.integers(14, 31)), int(rng.integers(14, 27)))
        m = random_walk_tube(shape, seed, steps=30, step=2.5, radius=(1.2, 4.0))
        dbf = _edt(m, an)
        idx = np.flatnonzero(m.reshape(-1, order="F"))
        k = int(rng.integers(4, 12))
        start = int(rng.integers(0, max(1, idx.size - k)))
        scat = rng.choice(idx, k, replace=False)
        sel = idx[start:start + k] if kind == "run" else scat
        sx, sy = shape[0], shape[1]
        path = np.stack([sel % sx, (sel // sx) % sy, sel // (sx * sy)], axis=1)
        const = cu * min(an)
        if special == "dup":                      # a vertex twice (not next to each other in the list)
            path = np.concatenate([path, path[:1]])
        elif special == "deadvertex":             # a vertex the mask has lost already
            m = m.copy(order="F")
            m[tuple(path[len(path) // 2])] = 0
        elif special == "nonpositive":            # scale * dbf + const = 0 for one vertex, below 0 for another
            dbf = dbf.copy(order="F")
            dbf[tuple(path[0])] = np.float32(2.0 * min(an))
            dbf[tuple(path[-1])] = np.float32(0.5 * min(an))
            dbf[tuple(path[1])] = np.float32(8.0 * min(an))
        out.append(Case("tube_%d_%s_%s" % (seed, kind, special or "plain"), m, an, path, dbf, scale, const))
    return out


# ---- many owners ------------------------------------------------------------------------------------------------------------------
RING = ((5, 0), (-5, 0), (0, 5), (0, -5), (3, 4), (-3, -4), (4, 3), (-4, -3), (3, -4), (-3, 4), (4, -3), (-4, 3))


def many_owners(n, radius=5.5, an=(1, 1, 1), thick=3):
    """a solid block, the first n path vertices of RING (all at distance 5 of the block's middle voxel in its middle plane), equal
    radii: the middle voxel (and others) can be owned by every one of them"""
    m = np.ones((23, 23, thick), np.uint8, order="F")
    path = [(11 + a, 11 + b, thick // 2) for a, b in RING[:n]]
    return with_radii("owners_%d_r%g_t%d" % (n, radius, thick), m, an, path, [radius] * n)


def owners():
    return [many_owners(n) for n in (2, 3, 4, 5, 6, 8, 9, 12)] + [many_owners(6, 7.0, thick=1), many_owners(8, 6.5, thick=1)]


# ---- radii on key values ---------------------------------------------------------------------------------------------------------------
KEY_OFFSETS = {(1, 1, 1): ((3, 0, 0), (1, 2, 3), (4, 1, 0), (3, 4, 0), (1, 0, 0)),
               (16, 16, 40): ((1, 0, 0), (0, 0, 1), (2, 0, 1), (3, 4, 0), (5, 0, 2))}


def key_radius_cases():
    """one source in the middle of a solid block, its radius exactly the key of a reachable offset, the float32 below it and the
    float32 above it: [(case, T offset, which)] with which = -1, 0, +1"""
    out = []
    for an, offs in KEY_OFFSETS.items():
        m = np.ones((15, 15, 9), np.uint8, order="F")
        K = sweep_ref.key_table(m.shape, an)
        for off in offs:
            r0 = K[off]
            for which, r in ((-1, np.nextafter(r0, np.float32(0))), (0, r0), (1, np.nextafter(r0, np.float32(np.inf)))):
                c = with_radii("keyradius_%g_%g_%g_%d%d%d_%+d" % (an + off + (which,)), m, an, [(7, 7, 4)], [r])
                out.append((c, off, which))
    return out


def shell(case, off):
    """the voxels of the case's mask whose key from the (single) source equals the key of offset `off`"""
    K = sweep_ref.key_table(case.mask.shape, case.an)
    p = case.path[0]
    g = np.meshgrid(*[np.abs(np.arange(n) - int(c)) for n, c in zip(case.mask.shape, p)], indexing="ij")
    return np.asfortranarray(K[g[0], g[1], g[2]] == K[off])


# ---- array edges ------------------------------------------------------------------------------------------------------------------
EDGE_SHAPES = ((1, 9, 9), (2, 7, 5), (3, 3, 3), (64, 1, 1), (1, 1, 40), (5, 1, 6))


Z_STEP_ENTRIES = (4, 5, 10, 11, 12, 13, 14, 15, 16, 17)       # the entries with dz != 0 that are no corner entries
Z_STEP_BITS = sum(1 << sweep_ref.GRAPH_BIT[i] for i in Z_STEP_ENTRIES)
EDGE_GRAPHS = ("none", "corneronly", "nocorner")


def edge_graph(shape, gname):
    """the voxel graph of an array-edge case.  Every voxel keeps every edge, except the voxels of the two x faces:
    corneronly   they lose every entry that changes z but the eight corner entries: a voxel of an x face gets to another z through a
                 corner entry alone -- a true corner (x +- 1) or, where the entry points out of the array in x, the yz diagonal it
                 degenerates into there (gated by the corner's bit: the gate of kh_apply_voxel_graph)
    nocorner     they lose the corner entries as well: from a voxel of an x face no z but its own can be reached"""
    if gname == "none":
        return None
    g = np.full(shape, ALL_EDGES, np.uint32, order="F")
    cut = Z_STEP_BITS | (CORNER_BITS if gname == "nocorner" else 0)
    g[0] &= np.uint32(~cut & 0xFFFFFFFF)
    g[-1] &= np.uint32(~cut & 0xFFFFFFFF)
    return g


def edge_cases():
    """masks that are all ones and fill their array; a source on a corner, on an x face and in the middle; without a graph and with
    the two graphs of edge_graph.  In the arrays of one or two voxels in x every voxel lies on an x face: there the corner entries
    (corneronly) or nothing (nocorner) lead to another z."""
    out = []
    for shape in EDGE_SHAPES:
        m = np.ones(shape, np.uint8, order="F")
        mid = tuple(s // 2 for s in shape)
        spots = {"corner": (0, 0, 0), "far": tuple(s - 1 for s in shape), "xface": (shape[0] - 1, mid[1], mid[2]), "middle": mid}
        for gname in EDGE_GRAPHS:
            g = edge_graph(shape, gname)
            for sname, p in spots.items():
                for an, r in (((1, 1, 1), 3.5), ((4, 4, 40), 41.0)):
                    out.append(with_radii("edge_%dx%dx%d_%s_%s_%g" % (shape + (gname, sname, an[2])), m, an, [p], [r], graph=g))
        # two sources on opposite corners whose balls meet: ties across the whole array
        out.append(with_radii("edge_%dx%dx%d_two" % shape, m, (1, 1, 1), [(0, 0, 0), tuple(s - 1 for s in shape)], [30.0, 30.0]))
    return out


# ---- sequences --------------------------------------------------------------------------------------------------------------------
def sequences():
    """[(name, mask, an, [(path, radii)])]: consecutive calls on one context and one alive mask"""
    out = []
    # A tie gadget in front of a 3x3 tube.  Sources A = (0, 1, 1) and B = (2, 1, 1) reach w = (1, 1, 1) at the same key; only A covers
    # q = (2, 2, 2), whose only way in is through w: whether q (and the stub and tube behind it) dies depends on which node of w pops
    # first -- the machine leaves them in M (call 1).  Before it a certified call at the far end, after it certified calls whose
    # balls overlap what the earlier ones killed, one of them from a vertex that is dead by then.
    m = np.zeros((40, 6, 6), np.uint8, order="F")
    m[4:, 2:5, 2:5] = 1
    for p in ((0, 1, 1), (1, 1, 1), (2, 1, 1), (2, 2, 2), (3, 3, 3)):
        m[p] = 1
    out.append(("tie_gadget", m, (1, 1, 1), [
        ([(33, 3, 3)], [3.0]),
        ([(0, 1, 1), (2, 1, 1)], [7.0, 1.2]),
        ([(9, 3, 3)], [5.0]),
        ([(20, 3, 3), (3, 3, 3)], [6.5, 4.0]),
        ([(37, 2, 2), (29, 4, 4)], [9.0, 2.0]),
    ]))
    # a blobby tube under (4, 4, 40): runs of a path, as the path loop hands them over
    t = random_walk_tube((30, 26, 20), 1601, steps=30, step=2.5, radius=(1.5, 4.0))
    dbf = _edt(t, (4, 4, 40))
    idx = np.flatnonzero(t.reshape(-1, order="F"))
    calls = []
    for a, n in ((idx.size // 10, 6), (7 * idx.size // 10, 8), (4 * idx.size // 10, 9), (9 * idx.size // 10, 4), (8 * idx.size // 10, 7),
                 (17 * idx.size // 20, 5)):
        sel = idx[a:a + n]
        path = np.stack([sel % 30, (sel // 30) % 26, sel // (30 * 26)], axis=1)
        # (a voxel two calls name has the same radius in both: the context has one distance field)
        calls.append((path, (np.float32(1.0) * dbf.reshape(-1, order="F")[sel] + np.float32(44.0)).astype(np.float32)))
    out.append(("tube_4_4_40", t, (4, 4, 40), calls))
    return out


def sequence_cases(seq):
    """the calls of a sequence as cases, each on the mask the oracle left after the one before"""
    name, mask, an, calls = seq
    cur = np.asfortranarray(mask, dtype=np.uint8).copy(order="F")
    out = []
    for j, (path, radii) in enumerate(calls):
        c = with_radii("seq_%s_%d" % (name, j), cur, an, path, radii)
        out.append(c)
        cur = judge(c).after
    return out


def sequence_dbf(seq):
    """one distance field for the whole sequence (a context has one): every call's radii at its vertices"""
    name, mask, an, calls = seq
    dbf = np.zeros(mask.shape, np.float32, order="F")
    for path, radii in calls:
        p = np.asarray(path, dtype=np.int64).reshape(-1, 3)
        dbf[p[:, 0], p[:, 1], p[:, 2]] = np.asarray(radii, dtype=np.float32)
    return dbf


# ---- bails after commits ------------------------------------------------------------------------------------------------------------
BIG_BALL_ARENA_DIVISOR = 8


def big_ball():
    """one source in the corner of a solid block with a ball that nearly fills it: 735 levels, class U"""
    m = np.ones((24, 24, 24), np.uint8, order="F")
    return with_radii("bigball", m, (1, 1, 1), [(0, 0, 0)], [30.0])


def big_ball_follow_up():
    """the next call on the context of big_ball(), on the mask that call leaves: a small ball in the opposite corner, which fits
    the capacities the bail tests cut big_ball() down to"""
    c = big_ball()
    return with_radii("bigball_then_small", judge(c).after, c.an, [(23, 23, 23)], [6.0])
