"""The abstract machine of the invalidation sweep (tests/sweep_ref.py) against the oracle's heap flood, and the
conditions on the inputs of tests/test_gpu_sweep_calls.py: which class of call (sweep_ref.classify) every family of
tests/sweep_cases.py contains.  No GPU: model and oracle alone.

Soundness, on every case: D <= the oracle's dead set <= D u M, and a certified call has D = the oracle's dead set with equal counts
(sweep_cases.check_soundness).  A violation would be a finding about the machine itself."""
import collections

import numpy as np
import pytest

import sweep_cases as S
import sweep_ref


def _tally(cases):
    t = collections.Counter()
    for c in cases:
        t[S.check_soundness(c).cls] += 1
    return t


def test_key_table_is_the_oracles_key():
    """the float32 operation order of ko_invalidate_ball_graph, against a scalar restatement of its eight lines"""
    f = np.float32
    for an in S.ANISOTROPIES + ((40, 32, 20),):
        K = sweep_ref.key_table((7, 6, 5), an)
        assert K.dtype == np.float32
        for off in ((0, 0, 0), (1, 0, 0), (3, 4, 0), (6, 5, 4), (2, 5, 1), (1, 2, 3)):
            a, b, c = (f(w) * f(o) for w, o in zip(an, off))
            s, t, u = f(a * a), f(b * b), f(c * c)
            s = f(s + t)
            s = f(s + u)
            assert K[off] == np.sqrt(s)


@pytest.mark.parametrize("graph", [False, True])
def test_goldens_soundness_and_classes(graph):
    """the recorded vectors of the compiled reference: the oracle reproduces them, the model is sound on them, and they contain
    certified calls and calls that leave voxels in M.  (The SURVEY B-8 shadow vectors -- a small ball shadowing a big one -- are
    class U: shadowing is decided by keys alone, every voxel has one possible owner.  The M calls are ties between overlapping
    balls on the random tubes.)"""
    tally = collections.Counter()
    for c, after, count in S.goldens(graph):
        v = S.check_soundness(c)
        assert v.count == count and np.array_equal(v.after, after), c.name
        tally[v.cls] += 1
    print("goldens%s: %s" % (" with graph" if graph else "", dict(tally)))
    assert tally["U"] > 0 and tally["K"] > 0
    if not graph:
        assert tally["M"] > 0
        shadow = [S.judge(c) for c, _, _ in S.goldens(False)[:4]]
        assert all(c.mask.shape == (40, 5, 5) for c, _, _ in S.goldens(False)[:4])
        assert [v.cls for v in shadow] == ["U"] * 4 and all(v.count == 99 for v in shadow)


def test_tubes_soundness_and_classes():
    cases = S.tubes()
    tally = _tally(cases)
    print("tubes:", dict(tally))
    assert tally["U"] > 0 and tally["K"] > 0 and tally["M"] > 0
    by = {c.name.rsplit("_", 1)[1]: c for c in cases}
    assert {"dup", "deadvertex", "nonpositive", "plain"} <= set(by)
    for c in cases:
        locs = S.locs_of(c)
        alive = c.mask.reshape(-1, order="F")[locs] != 0
        r = S.radii_of(c)
        if c.name.endswith("_dup"):
            assert len(set(locs.tolist())) < len(locs)
            # (the kernel counts a vertex named twice as two owners: stay inside what its eight slots hold)
            assert 2 * S.judge(c).model.max_cand <= 8
        if c.name.endswith("_deadvertex"):
            assert not alive.all() and alive.any()
        if c.name.endswith("_nonpositive"):
            assert (r == 0).any() and (r < 0).any() and (r > 0).any()
            # a vertex with a radius <= 0 dies itself and hands nothing on
            dead = set(S.judge(c).dead.tolist())
            assert all(int(l) in dead for l in locs[alive])
    assert {c.an for c in cases} == {tuple(float(v) for v in a) for a in S.ANISOTROPIES}
    assert any(not S.integral(c.an) for c in cases)


def test_many_owners_soundness_and_classes():
    """equal radii around one voxel: 2-4 owners die in the voxel's own word, 5-8 need the spill table, a ninth has no room"""
    cases = S.owners()
    want = {2: "K", 3: "K", 4: "K", 5: "S", 6: "S", 8: "S", 9: "C", 12: "C"}
    for c in cases:
        v = S.check_soundness(c)
        n = len(c.path)
        assert v.cls == want[n], (c.name, v.cls)
        assert v.model.max_cand == n == v.model.max_cand_at_death
        assert v.model.certified                           # (the machine itself has no limit: its verdict stands for 9 and 12 too)
        assert (v.model.n_many > 0) == (n >= 5) and v.model.n_many <= 256      # 256: the smallest spill table (plan.plan_spill)


def test_key_radius_soundness_and_shells():
    """a radius that IS a key value: the shell at key == r survives (strict <), with the float32 above it the shell dies"""
    for c, off, which in S.key_radius_cases():
        v = S.check_soundness(c)
        assert v.cls == "U"
        sh = S.shell(c, off)
        assert sh.sum() >= 2
        if off == (3, 4, 0) and c.an == (1.0, 1.0, 1.0):
            assert sh.sum() == 28              # two kinds of offset on one key: 4 of (5, 0, 0) and 24 of (3, 4, 0) fit the block
        survives = v.after[sh] != 0
        assert survives.all() if which <= 0 else not survives.any(), c.name


def test_array_edges_soundness_and_classes():
    cases = S.edge_cases()
    tally = _tally(cases)
    print("edges:", dict(tally))
    assert set(tally) == {"U", "K"}
    by = {c.name: c for c in cases}
    gate_needed = 0
    for c in cases:
        g = next((g for g in S.EDGE_GRAPHS[1:] if "_%s_" % g in c.name), None)
        if g is None:
            continue
        v = S.judge(c)
        plain = S.judge(by[c.name.replace("_%s_" % g, "_none_")])
        shape = c.mask.shape
        if shape[1] == 1 and shape[2] > 1 and shape[0] <= 2:
            # no y step, so no corner entry exists at all: from an x face no other z is reached under either graph
            assert v.count == 1 and plain.count > 1, c.name
        elif g == "corneronly" and min(shape[1:]) > 1:
            # the corner entries alone reach everything the full neighbourhood reaches
            assert np.array_equal(v.after, plain.after) and v.count > 1, c.name
            if shape[0] == 1:
                # ... and where the array is one voxel wide every one of them is a yz diagonal by the x-face rule of the reference:
                # a reading without that rule (a corner entry needs its x step) reaches no other z and is wrong
                other = sweep_ref.sweep_model(c.mask, c.an, c.path, S.radii_of(c), graph=c.graph, x_face_quirk=False)
                assert other.certified and other.count < v.count, c.name
                gate_needed += 1
        elif g == "nocorner" and shape[0] <= 2 and min(shape[1:]) > 1:
            # every voxel lies on an x face: without the corner entries the flood stays in the source's z
            assert v.count < plain.count, c.name
            src_z = int(c.path[0][2])
            assert (v.after[:, :, :src_z] == 1).all() and (v.after[:, :, src_z + 1:] == 1).all(), c.name
    assert gate_needed == 8


def test_sequences_soundness_and_classes():
    """a class-M call lies between certified ones, later balls overlap voxels an earlier call killed, and one call starts from a
    vertex that is dead by then"""
    for seq in S.sequences():
        cases = S.sequence_cases(seq)
        assert 4 <= len(cases) <= 6
        cls = [S.check_soundness(c).cls for c in cases]
        print("sequence %s: %s" % (seq[0], cls))
        start = cases[0].mask
        hits = []
        for c in cases[1:]:
            # does the ball reach into what an earlier call killed: a voxel that was alive at the start, is dead now, and lies inside
            K = sweep_ref.key_table(c.mask.shape, c.an)
            gone = np.argwhere((start != 0) & (c.mask == 0))
            hits.append(any((K[tuple(np.abs(gone - p).T)] < r).any() for p, r in zip(c.path, S.radii_of(c))))
        assert sum(hits) >= 2, (seq[0], hits)
        assert all(S.judge(c).count > 0 for c in cases)                     # every call has a live vertex: the sweep has events
        i = cls.index("M")
        assert 0 < i < len(cls) - 1 and set(cls[:i]) <= set("UK") and set(cls[i + 1:]) <= set("UK")
        bad = S.judge(cases[i])
        assert 0 < len(bad.model.M)
        if seq[0] == "tie_gadget":
            assert bad.count > bad.model.count                            # the heap run did kill voxels the machine left in M
        assert any((c.mask.reshape(-1, order="F")[S.locs_of(c)] == 0).any() for c in cases[i + 1:])      # a dead vertex afterwards


def test_big_ball_runs_out_of_a_capped_window_and_a_divided_arena():
    """the call of the bail-after-commit tests: certified by the machine, hundreds of levels; events lie more than 63 levels ahead
    of a level that is not the first (a window capped at 64 gives up after commits), and more levels are pending at one time than a
    divided arena has chunks (every pending level holds one at least)"""
    from kimimaro_amd.plan import int_key_mode, int_levels, plan_sweep
    c = S.big_ball()
    v = S.check_soundness(c)
    assert v.cls == "U" and v.model.levels > 300
    full = sweep_ref.sweep_model(c.mask, c.an, c.path, S.radii_of(c), trace=True)
    far = [(L, k) for L, k in full.ahead if round(k * k) - round(L * L) > 63]
    assert far and min(L for L, _ in far) > 4.0
    rmax = float(S.radii_of(c).max())
    gq = int_key_mode(c.an, rmax)[0]
    nlev, win = int_levels(c.an, gq, np.array([rmax]), 8192)
    lv = {"nlev": nlev, "win": win, "ok": np.array([True])}
    cnt = [int(c.mask.sum())]
    assert plan_sweep(cnt, np.array([rmax], np.float32), lv, keep_unfit=True).lev_window[0] > 64
    capped = plan_sweep(cnt, np.array([rmax], np.float32), lv, window_cap=64, window_cap_always=True, keep_unfit=True)
    assert capped.lev_window[0] == 64
    small = plan_sweep(cnt, np.array([rmax], np.float32), lv, arena_divisor=S.BIG_BALL_ARENA_DIVISOR, keep_unfit=True)
    assert 8 < small.ev_chunks[0] < full.peak_levels
    assert plan_sweep(cnt, np.array([rmax], np.float32), lv, keep_unfit=True).ev_chunks[0] > 4 * full.peak_levels
    # the call that follows on the same context fits both
    nxt = S.big_ball_follow_up()
    w = S.check_soundness(nxt)
    assert w.cls == "U" and w.count > 100 and not (nxt.mask[tuple(nxt.path[0])] == 0)
    after = sweep_ref.sweep_model(nxt.mask, nxt.an, nxt.path, S.radii_of(nxt), trace=True)
    assert 2 * after.peak_levels < small.ev_chunks[0] and max(round(k * k) - round(L * L) for L, k in after.ahead) < 64


def test_every_class_occurs():
    """the classes each family is there for (the per-family tests above assert the same and more), and all five together"""
    families = {"tubes": (S.tubes(), "UKM"), "owners": (S.owners(), "KSC"), "edges": (S.edge_cases(), "UK"),
                "radii": ([c for c, _, _ in S.key_radius_cases()], "U"),
                "sequence 0": (S.sequence_cases(S.sequences()[0]), "UM"), "sequence 1": (S.sequence_cases(S.sequences()[1]), "UKM")}
    seen = set()
    for name, (cases, want) in families.items():
        got = {S.judge(c).cls for c in cases}
        assert got == set(want), (name, got)
        seen |= got
    assert seen == set("UKSCM")
