"""trace_paths_kernel's ghosts and roll-backs against the model of them (tests/ghost_ref.py, which imports
nothing of the product).  Every case of tests/ghost_cases.py is traced with ghosts, with every ghost call rolled back at once
(paranoid) and without ghosts; with the integer levels and with the table of ranks; with 256 threads per label and with 64 (one
wave per label: what the lanes run).  Each run is held to (1) the oracle's paths, vertex for vertex, (2) status 0, (3) the model's
counters as exact integers: n_paths, n_vertices, stat_ghost_calls, stat_rollbacks, stat_sweep_calls, stat_sweep_bails,
stat_sweep_why -- one roll-back or one ghost call too many or too few fails --, and (4) the exit state include/kimi_hip.h promises
for the launch's buffers: cstate and qstate all zero, dist all +inf.  Which reasons of a roll-back the cases reach is established on
the CPU (tests/test_ghost_model_host.py)."""
import numpy as np
import pytest

import ghost_cases as GC
import sweep_cases as S

pytestmark = pytest.mark.gpu

SW_BAIL_M, SW_BAIL_LEVEL = 1, 8
COUNTERS = ("n_paths", "n_vertices", "stat_ghost_calls", "stat_rollbacks", "stat_sweep_calls", "stat_sweep_bails")
CASES = GC.cases()
PARAMS = [pytest.param(c, mode, keys, threads, id="%s-%s-%s-%d" % (c.name, mode, keys, threads))
          for c in CASES for mode in ("ghosts", "paranoid", "off") for keys in ("int", "table") for threads in (256, 64)
          if keys == "table" or S.integral(c.kw["anisotropy"])]


def fresh_engine(mode, keys="int", threads=256, **knobs):
    from kimimaro_amd.engine import Engine
    e = Engine()
    e.ghosts = mode != "off"
    e.ghost_paranoid = mode == "paranoid"
    e.int_keys = keys == "int"
    e.trace_threads = threads
    for k, v in knobs.items():
        assert hasattr(e, k), k
        setattr(e, k, v)
    return e


def keep_runs(eng):
    """the launches of the engine's next calls stay reachable (their device buffers with them): the list _trace_group's runs go to"""
    runs = []
    inner = eng._trace_group

    def group(*args, **kwargs):
        run = inner(*args, **kwargs)
        runs.append(run)
        return run
    eng._trace_group = group
    return runs


def check_exit_state(eng, run):
    """include/kimi_hip.h, kh_trace_paths: cstate and qstate all zero and dist all +inf on exit, as on entry"""
    t, b = eng.torch, run.b
    eng.sync()
    assert run.p.sweep_on and b["cstate"].numel() == run.nvox
    assert int(t.count_nonzero(b["cstate"])) == 0, "candidate words left behind"
    assert int(t.count_nonzero(b["qstate"])) == 0, "queue flags left behind"
    assert bool(t.isposinf(b["dist"]).all()), "distances left behind"


def check_record(rec, want, name, eng, why_extra=0):
    assert int(rec["status"]) == 0, (name, int(rec["status"]))
    got = {k: int(rec[k]) for k in COUNTERS}
    print(name, "record", got, "why", int(rec["stat_sweep_why"]), "model", {k: want.counters[k] for k in COUNTERS})
    # the label gets the sweep at all (test_gpu_sweep_calls.sweep_runs) and its spill table holds every voxel with a fifth owner
    nlev, win = int(rec["nlev"]), int(rec["lev_window"])
    assert nlev > 0 and ((win >= 64 and win & (win - 1) == 0 and win <= eng.sweep_lds_levels) or nlev <= eng.sweep_lds_levels), (name, nlev, win)
    assert int(rec["ev_spill"]) >= want.max_n_many
    assert got == {k: want.counters[k] for k in COUNTERS}, name
    assert int(rec["stat_sweep_why"]) == want.counters["stat_sweep_why"] | why_extra, (name, int(rec["stat_sweep_why"]))


@pytest.mark.parametrize("case,mode,keys,threads", PARAMS)
def test_case_against_the_model(case, mode, keys, threads):
    from kimimaro_amd.trace import trace
    want = GC.model(case, mode)
    eng = fresh_engine(mode, keys, threads, **case.knob)
    runs = keep_runs(eng)
    got = trace(case.mask, case.dbf, voxel_graph=case.graph, return_paths=True, _engine=eng, **case.kw)
    paths = GC.oracle_paths(case)
    assert len(got) == len(paths), (case.name, len(got), len(paths))
    for k, (a, b) in enumerate(zip(got, paths)):
        np.testing.assert_array_equal(np.asarray(a), np.asarray(b), err_msg="%s path %d" % (case.name, k))
    assert eng.last_retries == 0 and len(eng.last_tasks) == 1 and len(runs) == 1
    rec = eng.last_tasks[0]
    # the forced bail: the knob's bit is in the record, and the bails are the model's given that the knob's call was abandoned
    # every time it was tried (in mode "ghosts": once with a ghost alive -- the roll-back -- and once after the redo)
    check_record(rec, want, case.name, eng, why_extra=SW_BAIL_LEVEL if case.abandon else 0)
    if case.abandon:
        assert int(rec["lev_window"]) == case.knob["window_cap"]
    check_exit_state(eng, runs[0])


@pytest.mark.parametrize("threads", [256, 64])
def test_forced_bail_case_without_its_knob_is_certified(threads):
    """the same label with the planner's full window: the wide call is certified, so no roll-back for an abandoned call -- the bail
    of test_case_against_the_model is the knob's"""
    case = GC.by_name("comb_forced_bail")
    from kimimaro_amd.trace import trace
    import ghost_ref
    want = ghost_ref.trace_model(case.mask, case.dbf, mode="ghosts", **case.kw)
    assert "sweep abandoned" not in [rb.reason for rb in want.rollbacks]
    eng = fresh_engine("ghosts", "int", threads)
    got = trace(case.mask, case.dbf, return_paths=True, _engine=eng, **case.kw)
    assert len(got) == len(GC.oracle_paths(case))
    check_record(eng.last_tasks[0], want, case.name + " (no knob)", eng)


def _pool_volume():
    lab, dbf, whole = GC.side_by_side(GC.POOL_LABELS)
    return lab, dbf, whole


def _run_pool(eng, lab, dbf, whole):
    """the labels of the volume in ONE launch through Engine.run_labels, roots and targets as the cases dictate them.
    Returns {label: (paths, record)}."""
    from kimimaro_amd.assemble import paths_of
    from kimimaro_amd.plan import LabelSet
    from kimimaro_amd.volume import linear_index
    shape, n = lab.shape, len(whole)
    an = whole[0].kw["anisotropy"]
    d_cc, d_dbf = eng.to_device(np.asfortranarray(lab)), eng.to_device(np.asfortranarray(dbf))
    stats = eng.label_stats(d_cc, 4, d_dbf, shape, n)
    loc = lambda p: linear_index(p, shape)
    labels = LabelSet(np.arange(1, n + 1), stats.counts[1:n + 1], stats.dbf_max[1:n + 1], stats.first_index[1:n + 1], [0] * n,
                      [shape[0] - 1] * n, [loc(c.kw["root"]) for c in whole],
                      [[loc(p) for p in c.kw.get("manual_targets_before") or []] for c in whole],
                      [[loc(p) for p in c.kw.get("manual_targets_after") or []] for c in whole])
    kw = whole[0].kw
    params = dict(scale=kw["scale"], const=kw["const"], pdrf_scale=kw["pdrf_scale"], pdrf_exponent=kw["pdrf_exponent"])
    res = eng.run_labels(d_cc, 4, d_dbf, shape, an, n, labels, params, fix_branching=True)
    segids = [int(s) for s in res["tasks"]["segid"]]
    recs = {int(r["segid"]): r for r in eng.last_tasks}
    return {i: (paths_of(res, segids.index(i), shape), recs[i]) for i in range(1, n + 1)}, labels, params


@pytest.mark.parametrize("threads", [256, 64])
@pytest.mark.parametrize("pool", ["serves", "refuses"])
def test_pool_journal(pool, threads):
    """KH_TRACE_SCRATCH_POOL (four labels or more in a launch): heap and journal come out of one pool on demand.
    serves   the default pool.  A label's journal is taken at its first ghost and that call's log copied over from the first work
             list (trace.hip:365-372); every label's record is the model's in mode "ghosts".
    refuses  a pool of one node refuses every request.  A label that makes a ghost goes on without a journal (journal_off): the
             call is rolled back from its own log at the top of the next iteration.  The redo then asks the pool for the heap, is
             refused too and ends with KH_ST_HEAP_OVERFLOW: the engine traces the label again with scratch of its own, and the record
             is that attempt's (a slice for the journal: mode "ghosts").  Which labels those are follows from the model in mode
             "no_journal" -- the labels that need the heap at all: a redone or an uncertified call --, not from the run; a label that
             needs neither heap nor journal is never retried and carries the model's record from the first attempt."""
    import ghost_ref
    from kimimaro_amd.plan import plan_tasks
    lab, dbf, whole = _pool_volume()
    eng = fresh_engine("ghosts", "int", threads)
    if pool == "refuses":
        eng.scratch_pool_fraction = 0.0
    runs = keep_runs(eng)
    got, labels, params = _run_pool(eng, lab, dbf, whole)
    model = lambda c, mode: ghost_ref.trace_model(c.mask, c.dbf, mode=mode, **c.kw)
    first = runs[-1]                                 # (a retry is a nested group: it finishes first)
    assert first.p.use_pool and first.nl == len(whole) >= 4
    needs_heap = [i + 1 for i, c in enumerate(whole) if model(c, "no_journal").counters["stat_sweep_bails"] > 0]
    assert 0 < len(needs_heap) < len(whole)
    if pool == "serves":
        # from the plan: what the labels can ask for (a journal for a label with a ghost call, a heap for one with a redo) fits
        want = {i + 1: model(c, "ghosts") for i, c in enumerate(whole)}
        slot = {int(s): k for k, s in enumerate(first.p.tasks["segid"])}
        ask = sum(int(first.p.jnodes[slot[i]]) * (want[i].counters["stat_ghost_calls"] > 0) +
                  int(first.p.hcap[slot[i]]) * (want[i].counters["stat_sweep_bails"] > 0) for i in want)
        assert 1 + ask <= first.p.pool_nodes, (ask, first.p.pool_nodes)
        retried = []
    else:
        assert first.p.pool_nodes == 1
        retried = needs_heap
        want = {i + 1: model(c, "ghosts") for i, c in enumerate(whole)}
        for i, c in enumerate(whole):
            if i + 1 not in retried:
                nj = model(c, "no_journal").counters
                assert nj == want[i + 1].counters       # (no ghost, no heap: the same record in every mode)
    assert eng.last_retries == len(retried) and len(runs) == (2 if retried else 1)
    assert sum(w.counters["stat_ghost_calls"] > 0 for w in want.values()) >= 3
    assert sum(w.counters["stat_rollbacks"] > 0 for w in want.values()) >= 2
    from oracle import pipeline as P
    for i, c in enumerate(whole):
        paths, rec = got[i + 1]
        ref = P.trace(c.mask, c.dbf, return_paths=True, **c.kw)
        assert len(paths) == len(ref), c.name
        for a, b in zip(paths, ref):
            np.testing.assert_array_equal(np.asarray(a), np.asarray(b), err_msg=c.name)
        check_record(rec, want[i + 1], "%s (pool %s)" % (c.name, pool), eng)
    if pool == "serves":
        check_exit_state(eng, first)
        hdr = first.b["heap"][:1].cpu().numpy().view(np.uint32)
        assert int(hdr[0]) == 1 + ask and int(hdr[1]) == first.p.pool_nodes      # exactly the journals and heaps the model says were taken


def test_a_different_case_right_behind_on_the_same_engine():
    """one engine, a label with two roll-backs, then other labels right behind it: whatever a roll-back left in the engine (its
    cached blocks are handed out again) must not reach the next label"""
    from kimimaro_amd.trace import trace
    eng = fresh_engine("ghosts")
    for name in ("comb_two_then_one", "tube_3064_1_1_1_rail", "comb_valid0_after", "comb_two_then_one"):
        case = GC.by_name(name)
        got = trace(case.mask, case.dbf, return_paths=True, _engine=eng, **case.kw)
        paths = GC.oracle_paths(case)
        assert len(got) == len(paths)
        for a, b in zip(got, paths):
            np.testing.assert_array_equal(np.asarray(a), np.asarray(b), err_msg=name)
        check_record(eng.last_tasks[0], GC.model(case, "ghosts"), name, eng)
