"""The model of the path loop's ghosts and roll-backs (tests/ghost_ref.py) against the oracle, and the cases of tests/ghost_cases.py
as inputs: which reasons of a roll-back they reach is established here, by the model alone, before tests/test_gpu_ghost_calls.py
holds the device to the model's counters."""
import numpy as np
import pytest

import ghost_cases as GC
import ghost_ref
import sweep_cases as S
import sweep_ref

CASES = GC.cases()
IDS = [c.name for c in CASES]


def _same_paths(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    for k, (a, b) in enumerate(zip(got, want)):
        np.testing.assert_array_equal(np.asarray(a), np.asarray(b), err_msg="%s path %d" % (what, k))


@pytest.mark.parametrize("mode", ghost_ref.MODES)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_model_paths_equal_the_oracle_and_every_call_is_sound(case, mode):
    """ghosts never change a result: in every mode the model's paths are oracle.pipeline.trace's; and after every call of the loop
    certainly dead <= the oracle's dead set <= dead u ghosts (ghost_ref.trace_model(soundness=True) asserts it call by call)"""
    r = GC.model(case, mode, soundness=True)
    want = GC.oracle_paths(case)
    assert len(want) > 0
    _same_paths(r.paths, want, (case.name, mode))
    c = r.counters
    assert c["n_paths"] == len(want) and c["n_vertices"] == sum(len(p) for p in want)
    assert c["stat_rollbacks"] == len(r.rollbacks) <= c["stat_ghost_calls"]
    for rb in r.rollbacks:
        assert rb.reason in ghost_ref.REASONS and rb.to < rb.at and rb.journal > 0 and rb.ghost_calls_since >= 1
    if mode == "off":
        assert c["stat_ghost_calls"] == 0 and c["stat_rollbacks"] == 0 and r.ghosts_at_end == 0
        assert not any(len(call.made) for call in r.calls)
    if mode in ("paranoid", "no_journal"):
        # every call that makes a ghost is rolled back at the top of the next iteration -- unless max_paths ends the loop there
        assert c["stat_rollbacks"] == c["stat_ghost_calls"] - (1 if r.ghosts_at_end else 0)
        assert all(rb.reason == ("paranoid" if mode == "paranoid" else "no journal") and rb.ghost_calls_since == 1 for rb in r.rollbacks)
    if mode == "ghosts":
        assert c["stat_ghost_calls"] > 0, "a case of this file makes ghosts"


def test_every_reason_of_a_roll_back_is_reached_by_a_named_case():
    """the condition on the inputs: the reasons the cases reach (over all modes) are all five, each by the case REASON_CASES names"""
    reached = set()
    for case in CASES:
        for mode in ghost_ref.MODES:
            reached |= {rb.reason for rb in GC.model(case, mode).rollbacks}
    assert len(GC.UNREACHED) <= 1 and not set(GC.UNREACHED) & {"ghost target", "valid == 0", "paranoid"}
    assert reached == set(ghost_ref.REASONS) - set(GC.UNREACHED)
    assert set(GC.REASON_CASES) == set(ghost_ref.REASONS) - set(GC.UNREACHED)
    for reason, (name, mode) in GC.REASON_CASES.items():
        assert reason in {rb.reason for rb in GC.model(GC.by_name(name), mode).rollbacks}, (reason, name, mode)


def test_named_situations():
    g = lambda name: GC.model(GC.by_name(name), "ghosts")
    r = g(GC.NO_ROLLBACK)                         # every ghost killed for certain by later balls
    assert r.counters["stat_ghost_calls"] >= 2 and not r.rollbacks and r.ghosts_at_end == 0
    assert sum(len(c.killed_ghosts) for c in r.calls) == sum(len(c.made) for c in r.calls) > 0
    r = g(GC.TWO_THEN_ONE)                        # the journal grows over two calls, two later paths and more get their weights back
    first = r.rollbacks[0]
    assert first.ghost_calls_since >= 2 and first.rail_paths >= 2 and first.journal > max(len(c.made) + len(c.killed) for c in r.calls if c.path == first.to)
    r = g(GC.NOT_FIRST_PATH)
    assert any(rb.to > 0 for rb in r.rollbacks)
    r = g("comb_valid0_after")                    # after-targets taken because valid == 0
    case = GC.by_name("comb_valid0_after")
    assert [rb.reason for rb in r.rollbacks] == ["valid == 0"]
    tails = [tuple(int(v) for v in p[-1]) for p in r.paths[-2:]]
    assert sorted(tails) == sorted(case.kw["manual_targets_after"]) and len(r.calls) < len(r.paths) + len(r.rollbacks)
    r = g(GC.ENDS_WITH_GHOSTS)
    assert r.ghosts_at_end > 0 and r.counters["n_paths"] == GC.by_name(GC.ENDS_WITH_GHOSTS).kw["max_paths"]
    r = g(GC.SOMA)                                # the one-off call first, without ghosts allowed; ghosts later
    assert r.soma and r.calls[0].kind == "soma" and r.calls[0].certified and r.counters["stat_ghost_calls"] > 0
    r = g("comb_forced_bail")
    assert [rb.reason for rb in r.rollbacks] == ["sweep abandoned"]
    # the spread of the seeded tubes
    ans = {c.kw["anisotropy"] for c in CASES if c.name.startswith("tube")}
    assert {(1, 1, 1), (16, 16, 40), GC.NON_INTEGRAL} <= ans and not S.integral(GC.NON_INTEGRAL)
    assert {c.kw["fix_branching"] for c in CASES if c.name.startswith("tube")} == {True, False}
    graphs = [c for c in CASES if c.graph is not None]
    assert graphs and all(GC.model(c, "ghosts").counters["stat_ghost_calls"] > 0 for c in graphs)
    assert not any(call.cls == "C" for c in CASES for call in GC.model(c, "ghosts").calls)


def test_the_machine_without_ghosts_is_sweep_model():
    """`ghosts=` empty changes nothing: on every tube of sweep_cases the extended machine gives what the two-state one gives"""
    for case in S.tubes():
        a = sweep_ref.sweep_model(case.mask, case.an, case.path, S.radii_of(case))
        b = sweep_ref.sweep_model(case.mask, case.an, case.path, S.radii_of(case), ghosts=np.zeros(0, np.int64))
        for key in ("D", "M"):
            np.testing.assert_array_equal(getattr(a, key), getattr(b, key), err_msg=case.name)
        assert (a.count, a.max_cand, a.max_cand_at_death, a.n_many, a.levels, a.certified) == \
               (b.count, b.max_cand, b.max_cand_at_death, b.n_many, b.levels, b.certified), case.name
        assert b.KG.size == 0
        np.testing.assert_array_equal(b.made, b.M)
        assert S.judge(case).model.count == b.count


def test_three_state_rules_on_the_tie_gadget():
    """the rules one at a time, on the second call of sweep_cases' tie gadget (the one that leaves voxels undecided): the voxels
    left with candidates are the ghosts made; in the next call a ghost takes candidates, a deadline kills it and is counted apart,
    and a dying ghost sends no deadline: its neighbour that every owner covers stays undecided where an alive voxel's would die"""
    name, mask, an, calls = S.sequences()[0]
    cases = S.sequence_cases((name, mask, an, calls))
    c1 = cases[1]
    first = sweep_ref.sweep_model(c1.mask, c1.an, c1.path, S.radii_of(c1), ghosts=[])
    assert first.M.size > 0
    np.testing.assert_array_equal(first.made, first.M)
    after = c1.mask.copy(order="F").reshape(-1, order="F")
    after[first.D] = 0
    after = after.reshape(c1.mask.shape, order="F")
    ghosts = first.M
    sx, sy = mask.shape[0], mask.shape[1]
    lin = lambda p: p[0] + sx * (p[1] + sy * p[2])
    # a ball around the stub (3, 3, 3), itself a ghost: as a source it dies for certain (sweep.h:1078), and it is counted apart
    assert lin((3, 3, 3)) in set(ghosts.tolist())
    res = sweep_ref.sweep_model(after, an, [(3, 3, 3)], [1.8], ghosts=ghosts)
    assert lin((3, 3, 3)) in set(res.KG.tolist()) and set(res.KG.tolist()) <= set(res.D.tolist())
    plain = sweep_ref.sweep_model(after, an, [(3, 3, 3)], [1.8])
    # the same call with the ghosts taken for alive voxels kills the source's neighbours; with ghosts they only carry candidates
    assert set(res.D.tolist()) < set(plain.D.tolist())
    assert set(plain.D.tolist()) <= set(res.D.tolist()) | set(res.M.tolist())
    # an old ghost that was touched again and not killed stays one and is not made anew
    assert set(res.made.tolist()).isdisjoint(ghosts.tolist())
    assert set(res.M.tolist()) - set(res.made.tolist()) <= set(ghosts.tolist())


def test_side_by_side_volume_keeps_every_label_a_ghost_case():
    """the labels of the pool test (tests/test_gpu_ghost_calls.py) on their common volume: the model still equals the oracle there"""
    lab, dbf, whole = GC.side_by_side(GC.POOL_LABELS)
    assert len(whole) >= 4 and int(lab.max()) == len(whole)
    for case in whole:
        for mode in ("ghosts", "no_journal"):
            r = ghost_ref.trace_model(case.mask, case.dbf, mode=mode, soundness=True, **case.kw)
            from oracle import pipeline as P
            _same_paths(r.paths, P.trace(case.mask, case.dbf, return_paths=True, **case.kw), (case.name, mode))
