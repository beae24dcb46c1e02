"""kh_invalidate_ball call by call against the abstract machine of its sweep (tests/sweep_ref.py).

Every call is checked three ways: (1) mask and count equal the oracle's heap flood bit for bit; (2) the task record says the sweep
was called once; (3) the sweep certified exactly the calls the machine certifies -- class U, K or S: no bail, events, not one heap
push; class M: one bail for SW_BAIL_M alone; class C: a bail that names SW_BAIL_CAND.  Which class a case is in, i.e. which handler
and which exit of csrc/sweep.h it reaches, is established on the CPU (tests/test_sweep_model_host.py).  Every family runs with the
integer levels and with the table of ranks (`int_keys = False`); a non-integral anisotropy has the table only.

Engine.single_object / Engine.invalidate_ball are called directly: ops.roll_invalidation_ball_inside_component drops the record."""
import numpy as np
import pytest

import sweep_cases as S

pytestmark = pytest.mark.gpu

SW_BAIL_M, SW_BAIL_CAND, SW_BAIL_ARENA, SW_BAIL_LEVEL = 1, 2, 4, 8
MODES = ["int", "table"]


@pytest.fixture(scope="module")
def engines():
    from kimimaro_amd.engine import Engine
    table = Engine()
    table.int_keys = False
    return {"int": Engine(), "table": table}


def wanted(case, mode):
    """does this case run in this mode: the integer levels need an integral anisotropy (the table engine takes every case)"""
    return mode == "table" or S.integral(case.an)


def context(eng, case, rmax=None, dbf=None, **knobs):
    rmax = float(S.radii_of(case).max()) if rmax is None else rmax
    return eng.single_object(case.mask, case.an, rmax=rmax, dbf=case.dbf if dbf is None else dbf, voxel_graph=case.graph, **knobs)


def call(eng, ctx, case, mask=None):
    """one kh_invalidate_ball of the case's path on `mask` (default: the case's own).  Returns (count, mask after, task record)."""
    m = case.mask if mask is None else mask
    d_alive = eng.torch.from_numpy(np.ascontiguousarray(m.reshape(-1, order="F"))).to(eng.device)
    cnt, task = eng.invalidate_ball(ctx, d_alive, S.locs_of(case), case.scale, case.const, case.an)
    return cnt, d_alive.cpu().numpy().reshape(m.shape, order="F"), task


def record(task):
    return {k: int(task[k][0]) for k in ("stat_sweep_calls", "stat_sweep_bails", "stat_sweep_events", "stat_sweep_levels",
                                         "stat_sweep_why", "stat_heap_pushes", "ev_spill", "ev_chunks", "lev_window")}


def check_result(case, cnt, after):
    v = S.judge(case)
    assert cnt == v.count, (case.name, cnt, v.count)
    np.testing.assert_array_equal(after, v.after, err_msg=case.name)


def sweep_runs(eng, task):
    """does the object of this record get the sweep at all?  Its level words live in LDS: a window of them, or all of them; an object
    whose balls have more levels than that (a large radius under a coarse anisotropy) runs on the heap emulation only, by design
    (invalidate.h, sweep_setup: "a label for which neither does runs without the sweep"; plan.plan_sweep says the same)."""
    nlev, win = int(task["nlev"][0]), int(task["lev_window"][0])
    windowed = win >= 64 and win & (win - 1) == 0 and win <= eng.sweep_lds_levels
    return nlev > 0 and (windowed or nlev <= eng.sweep_lds_levels)


# a solid block under (40, 32, 20) with a radius of 2 027: 256 705 integer levels, more than LDS holds, and no window.  (The table
# of ranks has one entry per offset inside the 16 x 23 x 15 array, at most 5 520 levels: in table mode the vector is swept.)
NO_SWEEP_WITH_INTEGER_LEVELS = ("golden_graph_39",)


def check_class(case, task, eng=None):
    """the task record against the machine's verdict.  The one object of these tests that gets no sweep
    (NO_SWEEP_WITH_INTEGER_LEVELS; sweep_runs must say so too) has a record that says "heap"; everywhere else the sweep has to
    have run, once."""
    v = S.judge(case)
    r = record(task)
    cls = v.cls
    if v.model.n_many > r["ev_spill"]:
        cls = "C"            # more voxels with a fifth owner than the spill table has entries: the same exit as a ninth owner
    if case.name in NO_SWEEP_WITH_INTEGER_LEVELS and eng is not None and eng.int_keys:
        assert not sweep_runs(eng, task), (case.name, r)
        assert r["stat_sweep_calls"] == 0 and r["stat_sweep_bails"] == 0 and r["stat_heap_pushes"] > 0, (case.name, r)
        return "heap"
    assert r["stat_sweep_calls"] == 1, (case.name, r)
    if cls in "UKS":
        assert r["stat_sweep_bails"] == 0 and r["stat_sweep_events"] > 0 and r["stat_heap_pushes"] == 0, (case.name, cls, r)
    elif cls == "M":
        assert r["stat_sweep_bails"] == 1 and r["stat_sweep_why"] == SW_BAIL_M, (case.name, cls, r)
    else:
        assert r["stat_sweep_bails"] == 1 and r["stat_sweep_why"] & SW_BAIL_CAND, (case.name, cls, r)
    return cls


def run_family(eng, cases, mode):
    seen = set()
    for case in cases:
        if not wanted(case, mode):
            continue
        cnt, after, task = call(eng, context(eng, case), case)
        check_result(case, cnt, after)
        seen.add(check_class(case, task))
    return seen


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("graph", [False, True])
def test_goldens_with_accounting(engines, graph, mode):
    """the recorded vectors of the compiled reference, now with the task record: which of them the sweep certified"""
    eng = engines[mode]
    seen = set()
    for case, after, count in S.goldens(graph):
        cnt, got, task = call(eng, context(eng, case), case)
        assert cnt == count, case.name
        np.testing.assert_array_equal(got, after, err_msg=case.name)
        check_result(case, cnt, got)
        seen.add(check_class(case, task, eng))
    assert seen == ({"U", "K"} | ({"heap"} if mode == "int" else set()) if graph else {"U", "K", "M"})


@pytest.mark.parametrize("mode", MODES)
def test_random_tubes(engines, mode):
    seen = run_family(engines[mode], S.tubes(), mode)
    assert {"U", "K", "M"} <= seen


@pytest.mark.parametrize("mode", MODES)
def test_many_owners(engines, mode):
    """2-4 owners of one voxel (the out-of-line deadline handler), 5-8 (the spill table), 9 and 12 (no room: SW_BAIL_CAND)"""
    seen = run_family(engines[mode], S.owners(), mode)
    assert seen == {"K", "S", "C"}


def spill_table(eng, ctx):
    """the bytes of the context's spill table: the front of its arena, ev_spill candidate words of 8 bytes, then ev_spill keys of 4
    (invalidate.h, sweep_setup: sw.spc, sw.spk)"""
    n = int(ctx["task"]["ev_spill"][0]) * 12
    off = int(ctx["arena_ptr"].value) - int(ctx["d_arena"].data_ptr())
    assert n > 0 and int(ctx["task"]["ev_offset"][0]) == 0
    return ctx["d_arena"].cpu().numpy().view(np.uint8)[off:off + n]


@pytest.mark.parametrize("mode", MODES)
def test_spill_table_is_left_clean(engines, mode):
    """a class-S call twice in a row on a fresh mask with the same context: the first call's candidate words, filter words and spill
    entries must be gone -- the table is all-free after each call (it was used: the machine has voxels with five owners and more),
    and the second call is certified and right like the first"""
    eng = engines[mode]
    for case in (S.many_owners(8), S.many_owners(5)):
        assert S.judge(case).cls == "S" and S.judge(case).model.n_many > 0
        ctx = context(eng, case, dbf=S.many_owners(8).dbf)       # (the radii of all eight vertices: `other` below has six)
        for _ in range(2):
            cnt, after, task = call(eng, ctx, case)
            check_result(case, cnt, after)
            assert check_class(case, task) == "S"
            assert not spill_table(eng, ctx).any()
        # ... and a call with other owners right behind it
        other = S.many_owners(6)
        cnt, after, task = call(eng, ctx, other)
        check_result(other, cnt, after)
        assert check_class(other, task) == "S"


@pytest.mark.parametrize("mode", MODES)
def test_radii_on_key_values(engines, mode):
    """a radius that is exactly a key, the float32 below it and the one above it: `key < r` is strict in sweep_slim's integer
    limit and in the table mode's float compare alike -- the shell at key == r survives"""
    eng = engines[mode]
    for case, off, which in S.key_radius_cases():
        cnt, after, task = call(eng, context(eng, case), case)
        check_result(case, cnt, after)
        assert check_class(case, task) == "U"
        shell = S.shell(case, off)
        assert (after[shell] != 0).all() if which <= 0 else not (after[shell] != 0).any(), case.name


@pytest.mark.parametrize("mode", MODES)
def test_array_edges(engines, mode):
    """objects that fill their array, down to one voxel in x: the rows of three filter words next to a row's ends, the first and the
    last voxel of the volume.  With the graphs of sweep_cases.edge_graph the voxels of the x faces reach another z through corner
    entries alone, in the (1, 9, 9) array through the yz diagonals they degenerate into (the gate of kh_apply_voxel_graph: without it
    the flood stays in the source's z), or not at all; which of these changes the result is asserted on the host."""
    seen = run_family(engines[mode], S.edge_cases(), mode)
    assert seen == {"U", "K"}


@pytest.mark.parametrize("mode", MODES)
def test_sequences_on_one_context(engines, mode):
    """consecutive calls on one context and one alive mask, as the path loop makes them; the oracle goes call by call on its own
    copy.  A class-M call (heap emulation, then sweep_reset_words) lies between certified ones, later balls reach into what earlier
    calls killed: stale candidate, filter or spill words would show as a wrong mask or a wrong class in the next call."""
    eng = engines[mode]
    for seq in S.sequences():
        cases = S.sequence_cases(seq)
        rmax = max(float(S.radii_of(c).max()) for c in cases)
        ctx = context(eng, cases[0], rmax=rmax, dbf=S.sequence_dbf(seq))
        cur = cases[0].mask
        classes = []
        for case in cases:
            np.testing.assert_array_equal(cur, case.mask)
            cnt, cur, task = call(eng, ctx, case, mask=cur)
            check_result(case, cnt, cur)
            classes.append(check_class(case, task))
        assert "M" in classes[1:-1]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("knob", ["arena", "window"])
def test_bail_after_commits(engines, knob, mode):
    """a call the machine certifies over hundreds of levels, with a capacity that runs out partway (the planner's own knobs): the
    levels committed so far are undone, the heap emulation runs on the restored mask (the oracle's mask and count), and the next
    call on the same context -- one that fits the capacity, on the mask as it stands -- is certified and right"""
    eng = engines[mode]
    case = S.big_ball()
    assert S.judge(case).cls == "U"
    small = S.big_ball_follow_up()
    dbf = np.maximum(case.dbf, small.dbf)
    knobs = dict(arena_divisor=S.BIG_BALL_ARENA_DIVISOR) if knob == "arena" else dict(window_cap=64, window_cap_always=True)
    ctx = context(eng, case, dbf=dbf, **knobs)
    cnt, after, task = call(eng, ctx, case)
    r = record(task)
    assert r["stat_sweep_calls"] == 1 and r["stat_sweep_bails"] == 1, r
    assert r["stat_sweep_why"] & (SW_BAIL_ARENA if knob == "arena" else SW_BAIL_LEVEL), r
    assert r["stat_sweep_levels"] >= 3 and r["stat_heap_pushes"] > 0, r          # levels had been committed when it gave up
    check_result(case, cnt, after)
    cnt, after2, task = call(eng, ctx, small, mask=after)
    check_result(small, cnt, after2)
    assert check_class(small, task) == "U"
    # the same big call with its full capacity is certified
    cnt, after, task = call(eng, context(eng, case), case)
    check_result(case, cnt, after)
    assert check_class(case, task) == "U"


@pytest.mark.parametrize("mode", MODES)
def test_entry_bails(engines, mode):
    """two ways into the heap emulation that need no knob: a radius above the one the context was planned for (SW_BAIL_LEVEL before
    any event) and more path vertices than the object has voxels (no sweep call at all)"""
    eng = engines[mode]
    case = S.many_owners(3)
    cnt, after, task = call(eng, context(eng, case, rmax=3.0), case)
    r = record(task)
    assert (r["stat_sweep_calls"], r["stat_sweep_bails"], r["stat_sweep_why"], r["stat_sweep_events"]) == (1, 1, SW_BAIL_LEVEL, 0), r
    check_result(case, cnt, after)
    m = np.zeros((5, 3, 3), np.uint8, order="F")
    m[1:4, 1, 1] = 1
    crowd = S.with_radii("crowd", m, (1, 1, 1), [(1, 1, 1), (2, 1, 1), (3, 1, 1), (2, 1, 1)], [1.5, 1.5, 1.5, 1.5])
    cnt, after, task = call(eng, context(eng, crowd), crowd)
    r = record(task)
    assert r["stat_sweep_calls"] == 0 and r["stat_sweep_bails"] == 0 and r["stat_heap_pushes"] > 0, r
    check_result(crowd, cnt, after)
