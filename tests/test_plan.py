"""The launch plan (kimimaro_amd.plan) on numbers alone: no GPU, no torch, nothing allocated."""
import numpy as np
import pytest

from kimimaro_amd import _abi
from kimimaro_amd.plan import (LabelSet, arena_units, int_key_mode, int_levels, plan_arena, plan_spill, plan_sweep, plan_tasks,
                               sweep_radii)

# ties, a one-voxel label, both sides of the 32 768 and 65 536 thresholds of plan_arena
COUNTS = np.array([5, 1, 70000, 5, 40000], dtype=np.int64)
SEGIDS = np.array([7, 3, 9, 2, 4], dtype=np.int64)
ORDER = np.array([2, 4, 0, 3, 1])           # stable: the two labels of 5 voxels keep the caller's order
PARAMS = {"scale": 4, "const": 500, "pdrf_exponent": 4, "pdrf_scale": 100000}
AN = (16, 16, 40)


def labels(counts=COUNTS, segids=SEGIDS, tb=None, ta=None, soma=None, dbf_max=None):
    n = len(counts)
    dbf_max = np.linspace(10, 400, n, dtype=np.float32) if dbf_max is None else dbf_max
    return LabelSet(segids, counts, dbf_max, np.arange(n) + 100, np.arange(n), np.arange(n) + 50,
                    [0xFFFFFFFF] * (n - 1) + [17], tb, ta, soma)


def exclusive(cap):
    return np.cumsum(cap) - cap


@pytest.mark.parametrize("scale,divisor", [(1, 1), (8, 1), (1, 64), (8, 64)])
def test_plan_tasks_order_offsets_and_capacities(scale, divisor):
    p = plan_tasks(labels(), PARAMS, None, nlabels=9, scratch_scale=scale, scratch_divisor=divisor)
    np.testing.assert_array_equal(p.order, ORDER)
    np.testing.assert_array_equal(p.slot_of_label[SEGIDS[ORDER]], np.arange(5))
    assert np.count_nonzero(p.slot_of_label >= 0) == 5 and p.slot_of_label.shape == (10,)
    cnt = COUNTS[ORDER]
    qcap = cnt + 64
    hcap = np.maximum(np.maximum((3 * cnt) // 2 + 4096, np.minimum(3 * cnt + 2048, 32768)) * scale // divisor, 64)
    pcap = np.maximum((cnt // 16 + 2048) * scale // divisor, 8)
    for got, want in ((p.qcap, qcap), (p.hcap, hcap), (p.pcap, pcap), (p.jnodes, (2 * qcap + 3) // 4)):
        np.testing.assert_array_equal(got, want)
    for off, cap, field in ((p.list_off, cnt, "list_offset"), (p.q_off, qcap, "q_offset"), (p.h_off, hcap, "heap_offset"),
                            (p.p_off, pcap, "path_offset")):
        np.testing.assert_array_equal(off, exclusive(cap))
        np.testing.assert_array_equal(p.tasks[field], off)
    assert p.total == int(COUNTS.sum())
    t = p.tasks
    np.testing.assert_array_equal(t["segid"], SEGIDS[ORDER])
    np.testing.assert_array_equal(t["count"], cnt)
    np.testing.assert_array_equal(t["source"], ORDER + 100)
    np.testing.assert_array_equal(t["xmin"], ORDER)
    np.testing.assert_array_equal(t["xmax"], ORDER + 50)
    np.testing.assert_array_equal(t["root"], np.where(ORDER == 4, 17, 0xFFFFFFFF))
    np.testing.assert_array_equal(t["heap_capacity"], hcap)
    np.testing.assert_array_equal(t["path_capacity"], pcap)
    np.testing.assert_array_equal(t["q_capacity"], qcap)
    assert (t["pdrf_log2e"] == 2).all() and (t["pdrf_scale"] == np.float32(100000)).all() and (t["max_paths"] == 0).all()
    assert not p.sweep_on and p.ev_total == 0 and p.max_nlev == 0 and not t["nlev"].any()


def test_plan_tasks_targets_table_and_soma_columns():
    tb = [[11, 12], [], [13], [], [14, 15, 16]]
    ta = [[], [21], [22, 23], [], []]
    soma = {"soma_mode": [0, 1, 0, 1, 0], "fsr": [1.5, 2.5, 3.5, 4.5, 5.5], "soma_radius": [10, 20, 30, 40, 50],
            "soma_scale": [0.5] * 5, "soma_const": [0, 1, 2, 3, 4]}
    p = plan_tasks(labels(tb=tb, ta=ta, soma=soma), PARAMS, None, nlabels=9, max_paths=3)
    # slot order 2, 4, 0, 3, 1: before-then-after per label, one closing word
    np.testing.assert_array_equal(p.tgt_arr, [13, 22, 23, 14, 15, 16, 11, 12, 21, 0])
    assert p.tgt_arr.dtype == np.uint32
    np.testing.assert_array_equal(p.tasks["n_before"], [1, 3, 2, 0, 0])
    np.testing.assert_array_equal(p.tasks["n_after"], [2, 0, 0, 0, 1])
    np.testing.assert_array_equal(p.tasks["tgt_offset"], [0, 3, 6, 8, 8])
    for key, col in soma.items():
        np.testing.assert_array_equal(p.tasks[key], np.asarray(col, dtype=_abi.LABEL_T[key])[ORDER])
    assert (p.tasks["max_paths"] == 3).all()
    for tb_, ta_ in ((None, None), ([[]] * 5, None), (None, [[]] * 5)):
        q = plan_tasks(labels(tb=tb_, ta=ta_), PARAMS, None, nlabels=9)
        np.testing.assert_array_equal(q.tgt_arr, [0])
        assert not q.tasks["n_before"].any() and not q.tasks["n_after"].any() and not q.tasks["tgt_offset"].any()
    # an exponent that is no power of two: compute_pdrf's parameters do not travel with the task
    q = plan_tasks(labels(), dict(PARAMS, pdrf_exponent=3), None, nlabels=9)
    assert not q.tasks["pdrf_log2e"].any() and not q.tasks["pdrf_scale"].any()


def test_label_set_take():
    tb = [[11], [12], [13], [14], [15]]
    full = labels(tb=tb, soma={k: np.arange(5) for k in LabelSet.SOMA_COLUMNS})
    sub = full.take([3, 0])
    assert len(sub) == 2 and sub.targets_before == [[14], [11]] and sub.targets_after is None
    np.testing.assert_array_equal(sub.segid, [2, 7])
    np.testing.assert_array_equal(sub.count, [5, 5])
    np.testing.assert_array_equal(sub.first_index, [103, 100])
    np.testing.assert_array_equal(sub.root, [0xFFFFFFFF] * 2)
    np.testing.assert_array_equal(sub.soma["fsr"], [3, 0])
    assert sub.dbf_max.dtype == np.float32 and sub.root.dtype == np.uint32
    assert len(full.take(np.zeros(0, dtype=np.int64))) == 0


def test_scratch_pool_rule_and_size():
    four = labels(COUNTS[:4], SEGIDS[:4])
    assert not plan_tasks(labels(COUNTS[:3], SEGIDS[:3]), PARAMS, None, nlabels=9).use_pool
    assert plan_tasks(four, PARAMS, None, nlabels=9).use_pool
    assert not plan_tasks(four, PARAMS, None, nlabels=9, scratch_scale=8).use_pool
    assert not plan_tasks(four, PARAMS, None, nlabels=9, scratch_divisor=64).use_pool
    off = plan_tasks(four, PARAMS, None, nlabels=9, scratch_pool=False)
    assert not off.use_pool and off.pool_nodes == 0
    for frac in (0.15, 0.001):
        p = plan_tasks(labels(), PARAMS, None, nlabels=9, scratch_pool_fraction=frac)
        need = p.hcap + p.jnodes
        want = int(max(frac * float(need.sum()), (2 if frac >= 0.05 else 0) * float(need.max()))) + 1
        assert p.use_pool and p.pool_nodes == want
    assert plan_tasks(labels(), PARAMS, None, nlabels=9, scratch_pool_fraction=0.001).pool_nodes < int(need.max())


def int_lv(rmax_t, lds_levels=8192):
    """what Engine.sweep_levels returns in integer-key mode (that mode needs no device)"""
    rmax_t = np.asarray(rmax_t, dtype=np.float32)
    gq = int_key_mode(AN, float(rmax_t.max()))[0]
    nlev, win = int_levels(AN, gq, rmax_t.astype(np.float64), lds_levels)
    ok = np.isfinite(rmax_t) & (rmax_t > 0) & (nlev <= _abi.SWEEP_MAX_LEVELS)
    return {"d_rank": None, "rdims": (1, 1, 1), "nlev": np.where(ok, nlev, 0), "win": np.where(ok, win, 0), "ok": ok}


def test_plan_sweep_arena_layout():
    cnt = COUNTS[ORDER]
    # radii: none (no sweep for that label), small (levels fit LDS, no window needed either way), large (a window)
    rmax = np.array([900, 0, 60, 2000, 300], dtype=np.float32)
    lv = int_lv(rmax)
    assert lv["nlev"][1] == 0 and (lv["nlev"][[0, 2, 3, 4]] > 0).all() and (lv["win"][[0, 3]] > 0).all()
    # a label whose levels fit neither a window nor LDS: the heap emulation only
    lv["nlev"][4], lv["win"][4] = 9000, 0
    s = plan_sweep(cnt, rmax, lv, lds_levels=8192)
    fit = np.array([True, False, True, True, False])
    shift, chunks = plan_arena(cnt, lv["nlev"], True, lv["win"])
    spill = plan_spill(cnt)
    units = np.where(fit, arena_units(chunks, shift, spill), 0)
    np.testing.assert_array_equal(s.ev_offset, exclusive(units))
    assert s.ev_offset[1] == s.ev_offset[2] and s.ev_total == int(units.sum()) and (units[fit] > 0).all()
    np.testing.assert_array_equal(s.ev_chunks, np.where(lv["nlev"] > 0, chunks, 0))
    np.testing.assert_array_equal(s.ev_shift, shift)
    np.testing.assert_array_equal(s.ev_spill, np.where(fit, spill, 0))
    np.testing.assert_array_equal(s.nlev, lv["nlev"])
    np.testing.assert_array_equal(s.lev_window, lv["win"])
    np.testing.assert_array_equal(s.sweep_rmax, np.where(lv["ok"], rmax, 0))
    # the largest LDS word count: a label's window, or all its levels when it has none and they fit
    assert s.sweep_on and s.max_nlev == int(max(lv["win"].max(), lv["nlev"][2]))
    lv["win"][[0, 3]] = 0
    lv["nlev"][[0, 3]] = [100, 7000]
    assert plan_sweep(cnt, rmax, lv, lds_levels=8192).max_nlev == 7000
    # a 64th of the arena: never fewer than 8 chunks
    tiny = plan_sweep(cnt, rmax, int_lv(rmax), arena_divisor=64)
    _, chunks = plan_arena(cnt, tiny.nlev, True, tiny.lev_window)
    np.testing.assert_array_equal(tiny.ev_chunks, np.where(tiny.nlev > 0, np.maximum(chunks // 64, 8), 0))
    assert (chunks // 64 < 8).any() and (chunks // 64 > 8).any()
    # no label can use the sweep
    for none in (None, dict(lv, nlev=np.zeros(5, dtype=np.int64))):
        off = plan_sweep(cnt, rmax, none)
        assert not off.sweep_on and off.ev_total == 0 and off.max_nlev == 0 and not off.ev_chunks.any() and not off.nlev.any()


def test_plan_sweep_window_cap():
    n = 400                                      # max(1, 0.5 %) of 400 labels = 2
    cnt = np.full(n, 1000, dtype=np.int64)

    def wins(n_wide, **kw):
        rmax = np.full(n, 60, dtype=np.float32)
        rmax[:n_wide] = 2000
        lv = int_lv(rmax)
        assert np.count_nonzero(lv["win"] > 128) == n_wide
        return lv["win"], plan_sweep(cnt, rmax, lv, **kw).lev_window
    for n_wide, capped in ((1, True), (2, True), (3, False)):
        win, got = wins(n_wide, window_cap=128)
        np.testing.assert_array_equal(got, np.where(win > 0, np.minimum(win, 128), win) if capped else win)
    win, got = wins(3, window_cap=128, window_cap_always=True)
    assert got.max() == 128 and win.max() == 4096 and (got[win == 0] == 0).all()
    win, got = wins(1, window_cap=0, window_cap_always=True)
    np.testing.assert_array_equal(got, win)
    # a single label: max(1, ...) lets the cap apply
    lv = int_lv(np.array([2000], dtype=np.float32))
    assert plan_sweep([1000], np.array([2000], dtype=np.float32), lv, window_cap=64).lev_window[0] == 64


@pytest.mark.parametrize("nlev,win", [(3000, 512), (3000, 0), (20000, 0)])
def test_plan_sweep_of_one_label_is_single_objects_record(nlev, win):
    """Engine.single_object's call: no window cap, no arena divisor, and (keep_unfit) an arena and a spill table also for a
    label whose levels fit neither the window nor LDS"""
    cnt, rmax = 50000, np.float32(700)
    lv = {"nlev": np.array([nlev]), "win": np.array([win]), "ok": np.array([True])}
    s = plan_sweep([cnt], np.array([rmax]), lv, lds_levels=8192, keep_unfit=True)
    shift, chunks = (int(v) for v in plan_arena(cnt, nlev, True, win))
    spill = int(plan_spill(cnt))
    in_lds = win > 0 or nlev <= 8192
    got = tuple(int(getattr(s, k)[0]) for k in ("nlev", "ev_offset", "ev_chunks", "ev_shift", "ev_spill", "lev_window"))
    assert got == (nlev, 0, chunks, shift, spill, win) and s.sweep_rmax[0] == rmax and s.sweep_rmax.dtype == np.float32
    assert s.ev_total == int(arena_units(chunks, shift, spill)) and s.sweep_on
    assert s.max_nlev == (win if win > 0 else (nlev if in_lds else 0))
    masked = plan_sweep([cnt], np.array([rmax]), lv, lds_levels=8192)
    assert (int(masked.ev_spill[0]), masked.ev_total) == ((spill, s.ev_total) if in_lds else (0, 0))


def test_plan_through_plan_tasks_matches_plan_sweep():
    lab = labels()
    rmax = sweep_radii(lab.dbf_max[ORDER], PARAMS)
    np.testing.assert_array_equal(rmax, np.float32(4) * lab.dbf_max[ORDER] + np.float32(500))
    lv = int_lv(rmax)
    p = plan_tasks(lab, PARAMS, lv, nlabels=9, order=ORDER, rmax_t=rmax, arena_divisor=64, window_cap=64, window_cap_always=True)
    s = plan_sweep(COUNTS[ORDER], rmax, lv, arena_divisor=64, window_cap=64, window_cap_always=True)
    for key in ("nlev", "sweep_rmax", "ev_offset", "ev_chunks", "ev_shift", "ev_spill", "lev_window"):
        np.testing.assert_array_equal(p.tasks[key], getattr(s, key))
    assert (p.ev_total, p.max_nlev, p.sweep_on) == (s.ev_total, s.max_nlev, True) and s.max_nlev == 64


def test_offsets_beyond_32_bits_are_refused():
    two = LabelSet([1, 2], [2 ** 31, 2 ** 31], [1.0, 1.0], [0, 0], [0, 0], [0, 0], [0, 0])
    with pytest.raises(ValueError, match="scratch offsets exceed 32 bits"):
        plan_tasks(two, PARAMS, None, nlabels=2)
    # 2 048 labels of 2^25 voxels, levels in LDS without a window: 2^20 - 2 chunks of 64 slots each, > 2^21 units per label
    n = 2048
    cnt = np.full(n, 2 ** 25, dtype=np.int64)
    lv = {"nlev": np.full(n, 100), "win": np.zeros(n, dtype=np.int64), "ok": np.ones(n, dtype=bool)}
    assert int(arena_units(*plan_arena(cnt, lv["nlev"], True, lv["win"])[::-1], plan_spill(cnt)).sum()) >= 2 ** 32
    with pytest.raises(ValueError, match="event arena offsets exceed 32 bits"):
        plan_sweep(cnt, np.full(n, 100, dtype=np.float32), lv)
    assert plan_sweep(cnt[:n // 2], np.full(n // 2, 100, dtype=np.float32), {k: v[:n // 2] for k, v in lv.items()}).ev_total < 2 ** 32


def test_label_stats_bbox_is_find_objects():
    """LabelStats.bbox on the numpy restatement of kh_label_stats: a blob, a single voxel and a label that touches the far faces"""
    import os
    import sys
    import scipy.ndimage
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import prep_ref
    from kimimaro_amd.plan import LabelStats
    lab = np.zeros((9, 7, 5), dtype=np.uint32, order="F")
    lab[1:4, 2:6, 0:3] = 1
    lab[2, 3, 1] = 0                    # (a hole changes no box)
    lab[5, 1, 3] = 2                    # one voxel
    lab[6:9, 4:7, 2:5] = 3              # up to the last voxel of every axis
    dbf = np.random.default_rng(3).random(lab.shape).astype(np.float32)
    stats = LabelStats(*prep_ref.label_stats(lab, dbf, 3))
    assert stats._fields == ("counts", "dbf_max", "first_index", "xmin", "xmax", "yz")
    assert stats.yz.shape == (4, 4) and stats.counts.tolist() == [0, 35, 1, 27]
    boxes = scipy.ndimage.find_objects(lab)
    assert len(boxes) == 3
    for label in (1, 2, 3):
        lo, hi = stats.bbox(label)
        assert all(type(v) is int for v in lo + hi)
        assert tuple(slice(a, b) for a, b in zip(lo, hi)) == boxes[label - 1]
    assert stats.bbox(2) == ((5, 1, 3), (6, 2, 4)) and stats.bbox(3)[1] == lab.shape
