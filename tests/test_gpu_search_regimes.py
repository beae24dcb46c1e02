"""The searches of csrc/sssp.h (sssp<MODE>) on their own, in the regimes the whole-product tests do not show they reach: the
combine table full (an offer finds no slot, the frontier voxel is relaxed again), the near lists beyond their LDS part, hundreds
of far-list splits, and the rows27 loads at the first and last word of the array.  Inputs come from tests/search_cases.py; every
case first asserts, from the kernels' own counters (kh_label_t.stat_search_*), that it was in the regime it is built for, then
compares float32 bits, paths and parents with tests/search_ref.py (numpy Bellman fixpoint) and the oracle.  No tolerances.

The ladder rows of search_cases (SPILL_ROWS, RETRY_ROWS) sit one ladder block above the smallest block at which the counter was
nonzero on an MI355X; the values seen stand beside each row there."""
import functools

import numpy as np
import pytest

import search_cases as SC
import search_ref as R

pytestmark = pytest.mark.gpu

INF_BITS = 0x7F800000
COUNTERS = ("stat_search_retries", "stat_search_spills", "stat_search_splits")


@pytest.fixture(scope="module")
def eng():
    from kimimaro_amd import ops
    from kimimaro_amd.engine import Engine
    e = Engine()
    ops._engine = e
    try:
        yield e
    finally:
        ops._engine = None


# ---- references: computed once per (case, source), shared, never changed ------------------------------------------------------
@functools.lru_cache(maxsize=None)
def edf_reference(name, i):
    import oracle
    case = SC.EDF_BY_NAME[name]
    mask = case["mask"]()
    graph = case["graph"]() if case["graph"] else None
    src = case["sources"][i]
    with oracle.voxel_graph(graph):
        want, wloc = oracle.euclidean_distance_field(mask, src, case["an"], free_space_radius=case["fsr"])
    ref = R.edf_fixpoint(mask, src, case["an"], graph=graph, free_space_radius=case["fsr"])
    for a in (want, ref):
        a.setflags(write=False)
    return want, R.lin(wloc, mask.shape), ref


class EdfObject:
    """one mask on the device and kh_edf_batch on it, the way ops.euclidean_distance_field drives it, at a thread count of the test's"""

    def __init__(self, eng, case):
        self.eng, self.case = eng, case
        self.mask = case["mask"]()
        self.graph = case["graph"]() if case["graph"] else None
        self.ctx = eng.single_object(self.mask, case["an"], voxel_graph=self.graph)

    def run(self, src, threads):
        from kimimaro_amd import _abi
        eng, ctx, an = self.eng, self.ctx, self.case["an"]
        t, P = eng.torch, eng.ptr
        shape, nvox = ctx["shape"], ctx["nvox"]
        task = ctx["task"].copy()
        task["root"] = R.lin(src, shape)
        task["fsr"] = np.float32(self.case["fsr"])
        d_task = t.from_numpy(task.view(np.uint8).reshape(-1).copy()).to(eng.device)
        d_field = t.full((nvox + 4,), float("inf"), dtype=t.float32, device=eng.device)
        _abi.check(eng.lib.kh_edf_batch(P(d_task), 1, 2 | (threads << 8), P(ctx["d_lists"]), P(ctx["d_nbr"]), shape[0], shape[1], shape[2],
                                        float(an[0]), float(an[1]), float(an[2]), P(d_field), P(ctx["d_qstate"]), P(ctx["d_queues"]),
                                        eng.stream()))
        rec = d_task.cpu().numpy().view(_abi.LABEL_T)[0]
        field = d_field.cpu().numpy()
        assert int(ctx["d_qstate"].count_nonzero()) == 0, "membership bytes left set"
        assert np.all(field[nvox:].view(np.uint32) == INF_BITS), "the padding behind the field was written"
        return field[:nvox].reshape(shape, order="F"), rec


def check_edf_case(eng, name):
    case = SC.EDF_BY_NAME[name]
    obj = EdfObject(eng, case)
    for i, src in enumerate(case["sources"]):
        want, wloc, ref = edf_reference(name, i)
        loc, val = R.farthest(ref)
        assert loc == wloc
        for threads in case["threads"]:
            recs = []
            for _ in range(case["runs"]):
                got, rec = obj.run(src, threads)
                recs.append(rec)
                print("%s src %s threads %d: retries %d spills %d splits %d" % ((name, src, threads) + tuple(int(rec[c]) for c in COUNTERS)))
                assert int(rec["status"]) == 0
                for counter, least in case["expect"].items():
                    assert int(rec[counter]) >= least, "%s at %d threads left its regime: %s = %d < %d" % (
                        name, threads, counter, int(rec[counter]), least)
                np.testing.assert_array_equal(got.view(np.uint32), ref.view(np.uint32))
                np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
                assert int(rec["max_loc"]) == loc
                assert np.float32(rec["max_val"]).view(np.uint32) == np.float32(val).view(np.uint32)
            for counter, least in case["expect_once"].items():
                seen = [int(r[counter]) for r in recs]
                assert max(seen) >= least, "%s at %d threads never reached its regime: %s = %r" % (name, threads, counter, seen)


# ---- a. volume edges, rows27, far-list passes ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c["name"] for c in SC.TINY + SC.EDGES + SC.STICKS])
def test_edf_volume_edges(eng, name):
    check_edf_case(eng, name)


# ---- b. near-list spill and combine-table retry --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c["name"] for c in SC.LADDER_CASES])
def test_edf_spill_and_retry(eng, name):
    check_edf_case(eng, name)


# ---- c. ties, unreachable voxels, seeds ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c["name"] for c in SC.TIES + SC.SEEDS])
def test_edf_ties_unreachable_and_seeds(eng, name):
    check_edf_case(eng, name)
    case = SC.EDF_BY_NAME[name]
    want, wloc, _ = edf_reference(name, 0)
    if name.startswith("tie_"):
        assert wloc == 0
    if name == "two_blocks":
        assert np.all(want[7:].view(np.uint32) == INF_BITS) and wloc % 13 < 6     # (checked on the device result by equality above)
    if case["fsr"] >= 1000:
        assert np.isfinite(want[case["mask"]() != 0]).all()


# ---- d. weighted searches ------------------------------------------------------------------------------------------------------
def record(s):
    from kimimaro_amd import _abi
    return s.ctx["d_task"].cpu().numpy().view(_abi.LABEL_T)[0].copy()


def counted(s, call):
    """(result of call(), the counters the call added to the object's task record); status 0 before and after"""
    before = record(s)
    out = call()
    after = record(s)
    assert int(before["status"]) == 0 and int(after["status"]) == 0
    delta = {c: int(after[c]) - int(before[c]) for c in COUNTERS}
    print("   counters added:", delta)
    return out, delta


def device_distances(s):
    n = int(np.prod(s.shape))
    return s.d_dist[:n].cpu().numpy().reshape(s.shape, order="F")


@functools.lru_cache(maxsize=None)
def field_reference(name):
    import oracle
    make, src = SC.FIELD_CASES[name]
    field = make()
    want = oracle.field_distances(field, src)
    ref = R.field_fixpoint(field, src)
    for a in (field, want, ref):
        a.setflags(write=False)
    return field, want, ref


@pytest.mark.parametrize("name", sorted(SC.FIELD_CASES))
def test_weighted_distances_and_parents(eng, name):
    import oracle
    from kimimaro_amd import _abi, ops
    field, want, ref = field_reference(name)
    src = SC.FIELD_CASES[name][1]
    lin = R.lin(src, field.shape)
    s = ops._Search(field)
    _, delta = counted(s, lambda: s.run(1, lin))
    got = device_distances(s)
    if name == "random_24x20x12":
        assert delta["stat_search_spills"] > 0 or delta["stat_search_retries"] > 0, "the block left its regime: %r" % (delta,)
    np.testing.assert_array_equal(got.view(np.uint32), ref.view(np.uint32))
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
    # the predecessor walk on those distances, to the voxel farthest from the source and to the last voxel
    for tgt in (R.point(R.farthest(ref)[0], field.shape), tuple(v - 1 for v in field.shape)):
        walk, _ = counted(s, lambda: s.run(2, lin, R.lin(tgt, field.shape)))
        wpath = oracle.path_to_source(field, want, src, tgt)
        np.testing.assert_array_equal(walk, wpath)
        np.testing.assert_array_equal(ops.dijkstra(field, src, tgt), wpath)
    # the parents array: the oracle's, or a plateau in both
    try:
        wpar = oracle.parental_field(field, src)
    except oracle.OracleError as e:
        assert "plateau" in str(e)
        with pytest.raises(_abi.KimiHipError, match="plateau"):
            ops._Search(field).parents(lin)
        return
    s2 = ops._Search(field)
    par, _ = counted(s2, lambda: s2.parents(lin))
    np.testing.assert_array_equal(par, wpar)
    np.testing.assert_array_equal(ops.parental_field(field, src), wpar)
    np.testing.assert_array_equal(device_distances(s2).view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("name", sorted(SC.RAIL_CASES))
def test_railroad_cases(eng, name):
    import oracle
    from kimimaro_amd import _abi, ops
    make, src, rail = SC.RAIL_CASES[name]
    field = make()
    s = ops._Search(field)
    lin = R.lin(src, field.shape)
    if rail is None:
        with pytest.raises(_abi.KimiHipError, match="no rail"):
            s.run(0, lin)
        assert int(record(s)["status"]) == 8          # KH_ST_NO_RAIL and nothing else
        return
    got, _ = counted(s, lambda: s.run(0, lin))
    np.testing.assert_array_equal(got, oracle.railroad(field, src))
    assert tuple(got[0]) == rail and tuple(got[-1]) == src
    np.testing.assert_array_equal(ops.railroad(field, src), got)


def test_railroad_reuse_leaves_no_state(eng):
    """run(0, a), run(0, b), run(0, a) on one object: after each the distances are +inf again and no membership byte is set (the
    touched list, here far longer than the LDS part of the near lists, is what cleans up)"""
    import oracle
    from kimimaro_amd import ops
    make, a, b = SC.REUSE
    field = make()
    s = ops._Search(field)
    n = field.size
    results = []
    for src in (a, b, a):
        d = R.field_fixpoint(field, src, rails_absorb=True)
        best = R.nearest_rail(field, d, src)
        assert int((d <= best[1]).sum()) > 2 * 256, "fewer voxels settled than the LDS part of a list holds"
        got, _ = counted(s, lambda: s.run(0, R.lin(src, field.shape)))
        np.testing.assert_array_equal(got, oracle.railroad(field, src))
        assert np.all(s.d_dist[:n].cpu().numpy().view(np.uint32) == INF_BITS)
        assert int(s.ctx["d_qstate"].count_nonzero()) == 0
        results.append(got)
    np.testing.assert_array_equal(results[0], results[2])


# ---- e. the fused kernel: the search shares its LDS with the heap and the sweep ------------------------------------------------
@pytest.mark.parametrize("fuse", [True, False])
def test_path_loop_searches_reach_the_regimes(fuse):
    import oracle
    from oracle import pipeline as P
    from kimimaro_amd.engine import Engine
    from kimimaro_amd.trace import trace
    eng2 = Engine()
    eng2.trace_threads = 64
    eng2.fuse_edf = fuse
    m = np.ones((16, 16, 12), dtype=np.uint8, order="F")
    dbf = oracle.edt(m, (1, 1, 1), black_border=True)          # (a solid block that fills the volume has no border of its own)
    params = dict(scale=1.5, const=2, pdrf_scale=100000, pdrf_exponent=4)
    got = trace(m, dbf, anisotropy=(1, 1, 1), return_paths=True, _engine=eng2, **params)
    tk = eng2.last_tasks
    print("fuse_edf %s:" % fuse, {c: int(tk[c].sum()) for c in COUNTERS})
    assert int(tk["status"].sum()) == 0
    assert int(tk["stat_search_retries"].sum()) > 0 or int(tk["stat_search_spills"].sum()) > 0
    want = P.trace(m, dbf, anisotropy=(1, 1, 1), return_paths=True, **params)
    assert len(got) == len(want) and len(got) > 0
    for a, b in zip(got, want):
        np.testing.assert_array_equal(a, np.asarray(b, dtype=np.int64))
