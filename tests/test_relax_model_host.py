"""The model of the geodesic relax sweeps (tests/relax_ref.py) without a GPU.

(1) The model is right: on every thread and every random volume both orders of the simulator satisfy the per-sweep contract at
every sweep and end bit for bit at the heap Dijkstra of feature_ref.  (2) The contract has teeth: each wrong machine -- a wake rule
without corners or without edges, a clear that is left out, a sweep number kept in 32 bits -- and each tampered sweep is refused, at
a named clause of a named sweep.  (3) feature._to_fixpoint, the batch driver, against a scripted launch on the CPU."""
import numpy as np
import pytest

import relax_ref as M

ORDERS = ["jacobi", "bricks"]


def both_phases(vol, seeds, order, first_sweep=0, **wrong):
    d0, f0 = M.seeded(vol, seeds)
    d, _, counts_d = vol.run(d0, 1, order, first_sweep=first_sweep, **wrong)
    f, _, counts_f = vol.run(f0, 2, order, dist=d, first_sweep=first_sweep, **wrong)
    return d, f, counts_d, counts_f


def assert_reference(vol, seeds, d, f):
    want_d, want_f = M.reference(vol, seeds)
    np.testing.assert_array_equal(d.view(np.uint32), want_d.view(np.uint32))
    np.testing.assert_array_equal(f, want_f)


# ---- the model is right ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("step", M.STEPS, ids=str)
def test_threads(step):
    vol, seeds, path = M.thread_case(step)
    for order in ORDERS:
        d, f, counts_d, counts_f = both_phases(vol, seeds, order)
        assert_reference(vol, seeds, d, f)
        assert np.all(np.isfinite([d[q] for q in path])) and all(f[q] == 1 for q in path)
        assert counts_d[0][1] == 27 and counts_d[-1][0] == 0 and counts_f[-1][0] == 0
    # jacobi: the far brick's first voxel gets its value in sweep 3 (2 where the step has no x component), not in sweep 0
    d = M.seeded(vol, seeds)[0]
    planes = M.start_planes(vol.shape)
    arrived = None
    for s in range(5):
        d, planes, _ = vol.simulate_sweep(d, planes, s, 1, "jacobi")
        if arrived is None and np.isfinite(d[path[4]]):
            arrived = s
    assert arrived == (3 if step[0] else 2)


@pytest.mark.parametrize("k", [0, 1, 2])
def test_random_volumes(k):
    vol, seeds = M.random_case(k)
    assert M.brick_grid(vol.shape) == (3, 3, 2) and len(seeds) == 12
    for order in ORDERS:
        d, f, counts_d, counts_f = both_phases(vol, seeds, order)
        assert_reference(vol, seeds, d, f)
        if order == "jacobi":
            assert len(counts_d) > 24 and len(counts_f) > 24, "the driver has to go through several batches"


@pytest.mark.parametrize("shape", M.LINE_SHAPES, ids=str)
def test_extent_one_axes(shape):
    assert M.brick_grid(shape) in ((2, 1, 1), (1, 3, 1))
    for k in range(3):
        vol, seeds = M.random_case(k, shape)
        for order in ORDERS:
            d, f, _, _ = both_phases(vol, seeds, order)
            assert_reference(vol, seeds, d, f)


@pytest.mark.parametrize("base", [1, 2, 2 ** 32, 2 ** 40 + 2])
def test_other_first_sweeps(base):
    """the awake plane at base % 3: the right machine passes at every base"""
    vol, seeds, _ = M.thread_case((1, 1, 1))
    d, f, _, _ = both_phases(vol, seeds, "bricks", first_sweep=base)
    assert_reference(vol, seeds, d, f)


def test_dilation_counts():
    """one flag at a corner, an edge, a face, the centre of a 3 x 3 x 3 grid wakes 8, 12, 18, 27 bricks"""
    for bxyz, n in (((0, 0, 0), 8), ((1, 0, 0), 12), ((1, 1, 0), 18), ((1, 1, 1), 27)):
        plane = np.zeros(27, dtype=np.uint8)
        plane[M.brick_index(M.THREAD_SHAPE, bxyz)] = 1
        assert M.dilate(plane, M.THREAD_SHAPE).sum() == n
        assert M.dilate(plane, M.THREAD_SHAPE, reach=1).sum() == 1 + sum(1 for c in bxyz if c == 1) * 2 + sum(1 for c in bxyz if c != 1)


# ---- the contract has teeth: wrong machines ----------------------------------------------------------------------------------------
def refused(vol, seeds, phase=1, order="jacobi", first_sweep=0, planes=None, dist=None, **wrong):
    d0, f0 = M.seeded(vol, seeds)
    with pytest.raises(M.Refused) as e:
        vol.run(d0 if phase == 1 else f0, phase, order, dist=dist, first_sweep=first_sweep, planes=planes, **wrong)
    return e.value


@pytest.mark.parametrize("reach,steps", [(1, M.EDGES + M.CORNERS), (2, M.CORNERS)], ids=["faces", "faces+edges"])
def test_narrow_wake_rule_is_refused(reach, steps):
    """a wake rule of faces alone fails all 20 edge and corner crossings, one of faces and edges all 8 corner crossings: refused by
    the visited count of sweep 1, the first sweep that the rule decides; left to run, the far brick never gets its values"""
    assert len(steps) == (20 if reach == 1 else 8)
    for step in steps:
        vol, seeds, path = M.thread_case(step)
        for order in ORDERS:
            e = refused(vol, seeds, order=order, reach=reach)
            assert (e.clause, e.sweep) == ("visited", 1), (step, order, str(e))
            d, _, _ = vol.run(M.seeded(vol, seeds)[0], 1, order, check=False, reach=reach)
            want = M.reference(vol, seeds)[0]
            assert np.all(np.isinf([d[q] for q in path[4:]])) and np.all(np.isfinite([want[q] for q in path[4:]])), (step, order)
            np.testing.assert_array_equal(d[tuple(np.array(path[:4]).T)], want[tuple(np.array(path[:4]).T)])


@pytest.mark.parametrize("phase", [1, 2])
def test_missing_clear_is_refused(phase):
    """plane 0 starts all ones and is read again by sweep 3: sweep 1 has to clear it, and the checker says so at sweep 1"""
    vol, seeds, _ = M.thread_case((1, 1, 1))
    dist = M.reference(vol, seeds)[0]
    for order in ORDERS:
        e = refused(vol, seeds, phase=phase, order=order, dist=dist, clear=False)
        assert e.clause == "clear plane" and e.sweep == 1 and e.sweep <= 3


def test_sweep_number_in_32_bits_is_refused():
    """first_sweep = 2^32: the read plane is 1, a machine that truncates reads plane 0, finds it empty and visits nothing"""
    vol, seeds, _ = M.thread_case((1, 1, 1))
    assert M.plane_roles(2 ** 32) == (1, 2, 0) and M.plane_roles(2 ** 32, s_bits=32) == (0, 1, 2)
    e = refused(vol, seeds, first_sweep=2 ** 32, planes=M.start_planes(vol.shape, 1), s_bits=32)
    assert (e.clause, e.sweep) == ("visited", 0)


# ---- the contract has teeth: one right sweep, tampered with ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sweep5():
    """sweep 5 of phase 1 and of phase 2 of random volume 2, in place"""
    vol, seeds = M.random_case(2)
    out = {}
    d0, f0 = M.seeded(vol, seeds)
    dist = M.reference(vol, seeds)[0]
    for phase, state in ((1, d0), (2, f0)):
        planes = M.start_planes(vol.shape)
        for s in range(5):
            state, planes, _ = vol.simulate_sweep(state, planes, s, phase, "bricks", dist=dist)
        after, planes_after, c = vol.simulate_sweep(state, planes, 5, phase, "bricks", dist=dist)
        assert 0 < c[0] and c[1] <= vol.nbricks
        out[phase] = (vol, dist, state, after, planes, planes_after, c)
    return out


def tamper(sweep5, phase, clause, **edit):
    vol, dist, before, after, pb, pa, c = sweep5[phase]
    args = dict(before=before.copy(), after=after.copy(), pb=pb.copy(), pa=pa.copy(), c=c.copy())
    for name, fn in edit.items():
        fn(args[name])
    with pytest.raises(M.Refused) as e:
        vol.check_sweep(args["before"], args["after"], args["pb"], args["pa"], args["c"], 5, phase, dist=dist)
    assert e.value.clause == clause, str(e.value)


@pytest.mark.parametrize("phase", [1, 2])
def test_tampered_sweeps_are_refused(sweep5, phase):
    vol, dist, before, after, pb, pa, c = sweep5[phase]
    rep = vol.check_sweep(before, after, pb, pa, c, 5, phase, dist=dist)
    assert rep.forced > 0 and rep.forced_changed > 0 and rep.changed == c[0]
    read, write, clr = M.plane_roles(5)
    awake = M.dilate(pb[read], vol.shape)[vol.brick_of]
    differs = before.view(np.uint32) != after.view(np.uint32)
    b = int(np.argmax(np.bincount(vol.brick_of[differs], minlength=vol.nbricks)))        # the brick with the most changed voxels
    mine = vol.brick_of == b
    assert np.count_nonzero(differs & mine) >= 2
    v = tuple(np.argwhere(differs & mine)[0])
    still = tuple(np.argwhere(mine & ~differs & (vol.mask != 0) & (dist > 0) & np.isfinite(dist))[0])

    def put(at, value):
        return lambda a: a.__setitem__(at, value)

    tamper(sweep5, phase, "upper bound", after=put(v, before[v]))                              # a voxel that did not take its due
    tamper(sweep5, phase, "lower bound", after=put(still, 0))                                  # a value from nowhere
    tamper(sweep5, phase, "visited", c=put(1, c[1] - 1))
    tamper(sweep5, phase, "changed", c=put(0, c[0] + 1))
    tamper(sweep5, phase, "clear plane", pa=put((clr, 0), 1))
    tamper(sweep5, phase, "read plane", pa=put((read, 0), pa[read, 0] ^ 1))
    tamper(sweep5, phase, "write plane", pa=put((write, vol.brick_of[v]), 0))
    quiet = int(np.flatnonzero(pa[write] == 0)[0]) if np.any(pa[write] == 0) else None
    if quiet is not None:
        tamper(sweep5, phase, "write plane", pa=put((write, quiet), 1))
    tamper(sweep5, phase, "empty mask written", after=put(tuple(np.argwhere(mine & (vol.mask == 0))[0]), 3))
    tamper(sweep5, phase, "sleeping brick written", pb=put((read, slice(None)), 0), c=put(1, 0))
    if phase == 2:
        tamper(sweep5, phase, "seed or unreached voxel written", after=put(tuple(np.argwhere(awake & (dist == 0))[0]), 0))

def test_sleeping_brick_written_is_refused():
    vol, seeds, path = M.thread_case((1, 1, 1))
    d = M.reference(vol, seeds)[0]
    planes = np.zeros((3, 27), dtype=np.uint8)
    planes[0, 0] = 1                                               # the corner brick wakes 8 bricks; the thread's bricks are not among them
    new, new_planes, c = vol.simulate_sweep(d, planes, 0, 1, "jacobi")
    assert tuple(c) == (0, 8)
    vol.check_sweep(d, new, planes, new_planes, c, 0, 1)
    new[path[-1]] = 0
    with pytest.raises(M.Refused) as e:
        vol.check_sweep(d, new, planes, new_planes, c, 0, 1)
    assert e.value.clause == "sleeping brick written"


# ---- feature._to_fixpoint against a scripted launch ----------------------------------------------------------------------------------
class FakeEngine:
    def __init__(self):
        import torch
        self.torch, self.device = torch, "cpu"


class Script:
    """a launch that fills d_changed from `changed_of(sweep)` and records what it was given"""

    def __init__(self, changed_of, shape):
        self.changed_of, self.calls, self.dirty, self.nbricks = changed_of, [], None, M.brick_count(shape)

    def __call__(self, d_dirty, d_changed, n, first):
        if self.dirty is None:
            self.dirty = d_dirty
            assert d_dirty.dtype == FakeEngine().torch.uint8 and d_dirty.numel() == 3 * self.nbricks
            got = d_dirty.numpy().reshape(3, self.nbricks)
            assert np.all(got[0] == 1) and not got[1:].any()
        assert d_dirty is self.dirty, "one set of planes for all batches"
        assert d_changed.numel() == 2 * n and d_changed.dtype == FakeEngine().torch.int32
        self.calls.append((n, first))
        for j in range(n):
            d_changed[2 * j] = self.changed_of(first + j)
            d_changed[2 * j + 1] = 1000 + first + j
        return 0


def test_driver_batches_and_first_still_sweep():
    from kimimaro_amd import feature
    shape = (130, 9, 6)
    for still_at in (0, 5, 7, 8, 23, 24, 130, 183, 184):
        script = Script(lambda s: 0 if s >= still_at else 3, shape)      # every sweep from still_at on stands still: the first counts
        sweeps, visited = feature._to_fixpoint(FakeEngine(), script, shape, "scripted")
        assert sweeps == still_at + 1 and visited == [1000 + s for s in range(still_at + 1)]
        want = [(8, 0), (16, 8), (32, 24), (64, 56), (64, 120), (64, 184)]
        assert script.calls == [c for c in want if c[1] <= still_at]


def test_driver_reads_unsigned_counters():
    from kimimaro_amd import feature

    def launch(d_dirty, d_changed, n, first):
        d_changed[0::2] = -1                                       # 0xFFFFFFFF bricks changed: not "still"
        d_changed[1::2] = -2
        if first == 8:
            d_changed[2 * 3] = 0
        return 0
    sweeps, visited = feature._to_fixpoint(FakeEngine(), launch, (5, 5, 5), "scripted")
    assert sweeps == 12 and visited == [0xFFFFFFFE] * 12


@pytest.mark.parametrize("shape,calls", [((1, 1, 1), [(3, 0)]), ((5, 2, 2), [(8, 0), (14, 8)]), ((10, 5, 2), [(8, 0), (16, 8), (32, 24), (46, 56)])],
                         ids=str)
def test_driver_limit(shape, calls):
    """nothing ever stands still: KimiHipError after exactly nvox + 2 sweeps, the last batch cut to what is left"""
    from kimimaro_amd import _abi, feature
    script = Script(lambda s: 1, shape)
    nvox = int(np.prod(shape))
    with pytest.raises(_abi.KimiHipError, match="scripted: no fixpoint after %d sweeps over %d voxels" % (nvox + 2, nvox)):
        feature._to_fixpoint(FakeEngine(), script, shape, "scripted")
    assert script.calls == calls and sum(n for n, _ in script.calls) == nvox + 2


def test_driver_still_in_the_cut_batch():
    from kimimaro_amd import feature
    script = Script(lambda s: 0 if s == 21 else 1, (5, 2, 2))      # limit 22: sweep 21 is the last one allowed
    sweeps, visited = feature._to_fixpoint(FakeEngine(), script, (5, 2, 2), "scripted")
    assert sweeps == 22 and len(visited) == 22 and script.calls == [(8, 0), (14, 8)]
