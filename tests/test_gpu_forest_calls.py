"""kh_forest_components, kh_forest_measure and kh_forest_ticks call by call against tests/forest_ref.py.

The entry points are called directly with buffers sized as kimimaro_amd.forest sizes them, and everything they write is read back:
comp, nv, ne and degree equal the numpy statement word for word, cable equals math.fsum of the float32 edge lengths BIT FOR BIT (the
shapes satisfy forest_ref.cable_is_exact, under which no order of summation can give another f64: tests/test_forest_host.py shows
that on the CPU), and every table of kh_forest_ticks -- the chains, the oriented queue, the superedge records with their fusions,
arity, alive -- equals forest_ref.tick_tables.  Threshold 0 breaks the removal loop before its first removal and so shows the
orientation alone; the *_many functions of post never pass it.

Every output and scratch buffer is handed over with all its bytes 0xA5 and with 64 elements more than the call owns.  Afterwards
the 64 still hold the sentinel, and so does every word the model says no kernel writes.  Every forest comes from forest.pack on
consolidated skeletons: the device never sees a malformed adjacency."""
import numpy as np
import pytest

import forest_ref as R

pytestmark = pytest.mark.gpu

FILL = 0xA5
GUARD = 64


class Guarded:
    """a device buffer of n elements of `dtype` and GUARD more behind them, every byte FILL"""

    def __init__(self, eng, n, dtype):
        self.n, self.dtype = int(n), np.dtype(dtype)
        self.t = eng.torch.full(((self.n + GUARD) * self.dtype.itemsize,), FILL, dtype=eng.torch.uint8, device=eng.device)
        self.ptr = eng.ptr(self.t)

    def down(self):
        """the n elements, once the GUARD behind them is seen to be untouched"""
        host = self.t.cpu().numpy()
        assert np.all(host[self.n * self.dtype.itemsize:] == FILL), "the call wrote behind its %d elements" % self.n
        return host[:self.n * self.dtype.itemsize].view(self.dtype).copy()


def up(eng, a):
    a = np.ascontiguousarray(a).reshape(-1)
    return eng.torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(eng.device)


def same_bits(a, b):
    """np.array_equal on the integer views: signed zeros and sentinels count"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    word = {4: np.uint32, 8: np.uint64}.get(a.dtype.itemsize, a.dtype) if a.dtype.kind == "f" else a.dtype
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(word), b.view(word))


def device_measure(f):
    """kh_forest_components + kh_forest_measure -> {comp, nv, ne, degree, cable}"""
    from kimimaro_amd import _abi, ops
    eng = ops.engine()
    n, m = f.nverts, f.nedges
    d_xyz, d_edges = up(eng, f.xyz), up(eng, f.edges)
    out = {k: Guarded(eng, n, np.uint32) for k in ("comp", "nv", "ne", "degree")}
    out["cable"] = Guarded(eng, n, np.float64)
    _abi.check(eng.lib.kh_forest_components(eng.ptr(d_edges), n, m, out["comp"].ptr, eng.stream()))
    _abi.check(eng.lib.kh_forest_measure(eng.ptr(d_xyz), eng.ptr(d_edges), out["comp"].ptr, n, m, out["cable"].ptr, out["nv"].ptr,
                                         out["ne"].ptr, out["degree"].ptr, eng.stream()))
    eng.sync()
    return {k: g.down() for k, g in out.items()}


def check_measures(got, f, m, exact):
    assert np.array_equal(got["comp"], m.comp)
    roots = np.flatnonzero(m.nv)
    for k in ("nv", "ne", "degree"):
        assert got[k].dtype == np.uint32 and np.array_equal(got[k], getattr(m, k)), k
    outside = np.ones(f.nverts, dtype=bool)
    outside[roots] = False
    assert not got["nv"][outside].any() and not got["ne"][outside].any() and not got["cable"][outside].view(np.uint64).any()
    assert same_bits(got["cable"], exact), np.flatnonzero(got["cable"] != exact)[:8]


# ---- 1. components and measures ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.measure_shapes()) + ["all"])
def test_components_and_measures(name):
    f, m, exact = R.measure_call(name)
    assert all(R.cable_is_exact(lengths) for lengths in R.lengths_by_root(f, m.comp).values())      # a condition on the input
    check_measures(device_measure(f), f, m, exact)


def test_measures_do_not_depend_on_edge_order():
    from kimimaro_amd import forest
    f, m, exact = R.measure_call("forests_300")
    first = device_measure(f)
    check_measures(first, f, m, exact)
    rng = np.random.default_rng(16)
    edges = f.edges[rng.permutation(f.nedges)]                                # rows shuffled after the checks of pack
    edges[::3] = edges[::3, ::-1]
    g = forest.Forest(f.xyz, f.radii, f.vertex_types, np.ascontiguousarray(edges), f.vstart, f.estart, f.skeletons)
    second = device_measure(g)
    for k in first:
        assert same_bits(first[k], second[k]), k                              # an exact sum has no order


# ---- 2. no silent host path -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.TREE_SHAPES)
def test_tree_shapes_take_no_host_path(name):
    from kimimaro_amd import post
    skels = R.measure_shapes()[name]
    f, m, _ = R.measure_call(name)
    threshold = R.dust_threshold(f, m)                                        # outside every band, by the host's own sums
    stats = {}
    got = post.remove_loops_many(skels, stats=stats)
    assert stats["loops_host"] == 0
    assert all(R.same(a, post.remove_loops(s)) for a, s in zip(got, skels))
    got = post.remove_dust_many(skels, threshold, stats=stats)
    assert stats["dust_host_decided"] == 0 and stats["components"] == np.count_nonzero(m.nv)
    assert all(R.same(a, post.remove_dust(s, threshold)) for a, s in zip(got, skels))


def test_the_ring_takes_the_host_path_and_the_tree_beside_it_is_counted():
    from kimimaro_amd import post
    skels = R.measure_shapes()["ring_and_tree"]
    stats = {}
    got = post.remove_loops_many(skels, stats=stats)
    assert stats["loops_host"] == 1 and R.same(got[0], post.remove_loops(skels[0]))


# ---- 3. the tables of kh_forest_ticks ---------------------------------------------------------------------------------------------------
class TickCall:
    """one forest's inputs of kh_forest_ticks on the device; run(threshold) -> {table: host array}, guards checked"""

    def __init__(self, f, m):
        from kimimaro_amd import ops
        self.eng = eng = ops.engine()
        self.f = f
        self.model = R.tick_tables(f, m, 0.0, fill=FILL)
        T = self.model
        self.n, self.ns, self.nc, self.ncomps = f.nverts, int(T.nbr.size), int(T.crit.size), int(T.crit_start.size) - 1
        self.inputs = [up(eng, a) for a in (f.xyz, T.row, T.nbr, T.crit, T.crit_start)]

    def run(self, threshold):
        from kimimaro_amd import _abi
        eng, P = self.eng, self.eng.ptr
        slots = Guarded(eng, 4 * self.ns, np.uint32)
        arity = Guarded(eng, self.n, np.int32)
        recs = Guarded(eng, 5 * self.nc, np.uint32)
        length = Guarded(eng, self.nc, np.float64)
        flag = Guarded(eng, self.nc, np.uint8)
        alive = Guarded(eng, self.ns, np.uint8)
        _abi.check(eng.lib.kh_forest_ticks(*[P(t) for t in self.inputs], self.n, self.ns, self.nc, self.ncomps, float(threshold),
                                           slots.ptr, arity.ptr, recs.ptr, length.ptr, flag.ptr, alive.ptr, eng.stream()))
        eng.sync()
        s, r = slots.down().reshape(4, self.ns), recs.down().reshape(5, self.nc)
        out = {"far": s[0], "twin": s[1], "len32": s[2].view(np.float32), "rec": s[3], "arity": arity.down(), "len": length.down(),
               "flag": flag.down(), "alive": alive.down()}
        out.update(zip(("queue", "ea", "eb", "sa", "sb"), r))
        return out


TABLES = R.TickTables.SLOT + ("arity",) + R.TickTables.RECORD + ("alive",)


@pytest.mark.parametrize("name", R.TABLE_CASES + ("tick_forest",))
def test_tick_tables(name):
    f, m, thresholds = R.table_call(name)
    call = TickCall(f, m)
    assert call.ncomps >= 1 and thresholds[0] == 0.0 and thresholds[-1] == np.inf
    removed = []
    for threshold in thresholds:
        want = R.tick_tables(f, m, threshold, fill=FILL)
        got = call.run(threshold)
        for table in TABLES:
            assert same_bits(got[table], getattr(want, table)), (name, threshold, table, np.flatnonzero(
                np.ascontiguousarray(got[table]).view(np.uint8).reshape(got[table].size, -1)
                != np.ascontiguousarray(getattr(want, table)).view(np.uint8).reshape(got[table].size, -1))[:8])
        removed.append(int(np.count_nonzero(got["alive"] == 0)))
    assert removed[0] == 0 < removed[-1]                                      # threshold 0 removes nothing: the orientation alone
    if name == "tick_forest":
        # the paths between the trees are not listed: their slots hold the sentinel after every kind of call (here: the last one)
        row = call.model.row.astype(np.int64)
        paths = [k for k, s in enumerate(f.skeletons) if s.id >= 100]
        assert len(paths) >= 1 and call.ncomps > 1
        for k in paths:
            a, b = row[f.vstart[k]], row[f.vstart[k + 1]]
            assert b - a == 2 * (f.estart[k + 1] - f.estart[k]) > 0
            assert not np.any((call.model.crit >= f.vstart[k]) & (call.model.crit < f.vstart[k + 1]))
            for table in R.TickTables.SLOT:
                assert np.all(np.ascontiguousarray(got[table][a:b]).view(np.uint8) == FILL), (k, table)
            assert np.all(got["alive"][a:b] == 1)
