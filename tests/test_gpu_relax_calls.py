"""kh_geodesic_relax / kh_feature_relax call by call against the model of their machine (tests/relax_ref.py).

The entry points are called directly, one sweep per call unless a test says otherwise; masks, fields and planes come from numpy
and everything is read back after each call.  Every call goes through the model's check_sweep -- awake bricks, untouched voxels,
the three planes and both counters bit for bit, the two bounds on every voxel of an awake brick -- and every run ends bit for bit
at the heap Dijkstra of feature_ref.  That the checker refuses machines with a narrower wake rule, without the clear or with a
32-bit sweep number is shown without a GPU (tests/test_relax_model_host.py).

`changed` is handed over filled with 0x7F bytes, two sentinel words behind the 2 * sweeps the call owns: the call zeroes its
words itself and leaves the sentinels.  A run may need fewer sweeps than the model's Jacobi order (a read may see a value stored
in the same sweep), never more: that bound ends every loop here."""
import functools

import numpy as np
import pytest

import oversegment_chunked_ref as H
import relax_ref as M

pytestmark = pytest.mark.gpu

KH_EINVAL = 1
SENTINEL = 0x7F7F7F7F


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


class Device:
    """the kernels on one model volume"""

    def __init__(self, vol):
        import torch
        from kimimaro_amd import ops
        self.torch, self.eng, self.vol = torch, ops.engine(), vol
        self.w = [float(np.float32(a)) for a in vol.anisotropy]
        self.d_nbr = self.up(vol.mask)

    def up(self, a):
        """a host array [x, y, z] of 32-bit words -> device, linear-index order"""
        flat = np.ascontiguousarray(M.flat(a))
        return self.torch.from_numpy(flat.view(np.int32) if flat.dtype == np.uint32 else flat).to(self.eng.device)

    def down(self, t, dtype):
        return np.ascontiguousarray(t.cpu().numpy().view(dtype).reshape(self.vol.shape, order="F"))

    def call(self, phase, state, planes, s, sweeps=1, dist=None, shape=None):
        """one call -> (rc, state after, planes after, the call's words of `changed` as uint32)"""
        eng, P, t = self.eng, self.eng.ptr, self.torch
        sx, sy, sz = self.vol.shape if shape is None else shape
        d_state = self.up(state)
        d_planes = t.from_numpy(np.ascontiguousarray(planes, dtype=np.uint8).reshape(-1)).to(eng.device)
        n = 2 * max(sweeps, 1)
        d_changed = t.full((n + 2,), SENTINEL, dtype=t.int32, device=eng.device)
        if phase == 1:
            rc = eng.lib.kh_geodesic_relax(P(self.d_nbr), sx, sy, sz, self.w[0], self.w[1], self.w[2], P(d_state), P(d_planes),
                                           P(d_changed), sweeps, s, eng.stream())
        else:
            d_dist = self.up(dist)
            rc = eng.lib.kh_feature_relax(P(self.d_nbr), sx, sy, sz, self.w[0], self.w[1], self.w[2], P(d_dist), P(d_state),
                                          P(d_planes), P(d_changed), sweeps, s, eng.stream())
        eng.sync()
        if phase == 2:
            np.testing.assert_array_equal(bits(self.down(d_dist, np.float32)), bits(dist), err_msg="phase 2 wrote the distances")
        words = d_changed.cpu().numpy().view(np.uint32)
        assert np.all(words[n:] == SENTINEL), "the words behind 2 * sweeps belong to the caller"
        after = self.down(d_state, np.float32 if phase == 1 else np.uint32)
        return rc, after, d_planes.cpu().numpy().reshape(3, -1), words[:n]

    def sweep(self, phase, state, planes, s, dist=None):
        """one sweep, checked against the contract -> (state after, planes after, (changed, visited), the checker's report)"""
        rc, after, planes_after, c = self.call(phase, state, planes, s, dist=dist)
        assert rc == 0
        report = self.vol.check_sweep(state, after, planes, planes_after, c, s, phase, dist=dist)
        return after, planes_after, (int(c[0]), int(c[1])), report

    def to_fixpoint(self, phase, state, limit, dist=None, base=0, planes=None):
        """sweeps base, base + 1, ... of one call each, every one checked, until one changes nothing; `limit`: the model's count"""
        planes = M.start_planes(self.vol.shape, base % 3) if planes is None else planes
        counts = []
        for j in range(limit):
            state, planes, c, _ = self.sweep(phase, state, planes, base + j, dist=dist)
            counts.append(c)
            if c[0] == 0:
                return state, planes, counts
        pytest.fail("phase %d: no still sweep within the %d sweeps that the Jacobi order needs: %r" % (phase, limit, counts))


class Case:
    """a model volume with its seeds, its reference fields and the sweeps the model's Jacobi order needs per phase"""

    def __init__(self, name, vol, seeds):
        self.name, self.vol, self.seeds = name, vol, seeds
        self.d0, self.f0 = M.seeded(vol, seeds)
        self.want_d, self.want_f = M.reference(vol, seeds)
        self.model_d = len(vol.run(self.d0, 1, "jacobi", check=False)[2])
        self.model_f = len(vol.run(self.f0, 2, "jacobi", dist=self.want_d, check=False)[2])

    def run_both(self, dev, base=0):
        d, _, counts_d = dev.to_fixpoint(1, self.d0, self.model_d, base=base)
        np.testing.assert_array_equal(bits(d), bits(self.want_d))
        f, _, counts_f = dev.to_fixpoint(2, self.f0, self.model_f, dist=d, base=base)
        np.testing.assert_array_equal(f, self.want_f)
        print("relax-sweeps %s: distance %d (model %d), feature %d (model %d)" %
              (self.name, len(counts_d), self.model_d, len(counts_f), self.model_f))
        return counts_d, counts_f


@functools.lru_cache(maxsize=None)
def thread_case(step):
    vol, seeds, path = M.thread_case(step)
    case = Case("thread%r" % (step,), vol, seeds)
    case.path = path
    return case


@functools.lru_cache(maxsize=None)
def random_case(k, shape=M.RANDOM_SHAPE):
    vol, seeds = M.random_case(k, shape)
    return Case("random%d%r" % (k, shape), vol, seeds)


# ---- threads through all 26 brick contacts ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("step", M.STEPS, ids=str)
def test_thread(step):
    """the label passes from brick (1, 1, 1) to its neighbour through one face, edge or corner, in a sweep in which only the wake
    rule can have the far brick awake"""
    case = thread_case(step)
    dev = Device(case.vol)
    # phase 1 by hand, to see when the far brick takes its first value
    state, planes, arrived = case.d0, M.start_planes(case.vol.shape), None
    for s in range(case.model_d):
        state, planes, c, _ = dev.sweep(1, state, planes, s)
        if arrived is None and np.isfinite(state[case.path[4]]):
            arrived = s
        if c[0] == 0:
            break
    assert c[0] == 0 and arrived is not None and arrived >= 1, "past sweep 0 a brick is awake by the wake rule alone"
    np.testing.assert_array_equal(bits(state), bits(case.want_d))
    counts_d, counts_f = case.run_both(dev)
    assert counts_d[-1][0] == 0 and counts_f[-1][0] == 0 and counts_d[0][1] == 27 and counts_f[0][1] == 27
    assert all(case.want_f[q] == 1 for q in case.path)


# ---- one flag ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def flag_case():
    lab, seeds = M.random_volume(3, M.THREAD_SHAPE, nseeds=120)
    vol = M.Volume(lab, (1.5, 1, 3))
    d, f = M.reference(vol, seeds)
    return vol, d, f


def settled_voxel(vol, d, brick):
    """the first voxel of the brick that a seed reaches from elsewhere and that has a same-label neighbour"""
    at = np.argwhere((vol.brick_of == M.brick_index(vol.shape, brick)) & (vol.mask != 0) & (d > 0) & np.isfinite(d))
    assert len(at), "the volume has such a voxel in brick %r" % (brick,)
    return tuple(int(c) for c in at[0])


@pytest.mark.parametrize("phase", [1, 2])
@pytest.mark.parametrize("brick,visited,asleep", [((0, 0, 0), 8, (2, 2, 2)), ((1, 0, 0), 12, (1, 2, 2)), ((1, 1, 0), 18, (1, 1, 2)),
                                                  ((1, 1, 1), 27, None)], ids=["corner", "edge", "face", "centre"])
def test_one_flag(brick, visited, asleep, phase):
    vol, d, f = flag_case()
    dev = Device(vol)
    fix = d if phase == 1 else f
    raised = M.INF if phase == 1 else np.uint32(M.NONE)
    s = 7
    read, write, clr = M.plane_roles(s)
    b = M.brick_index(vol.shape, brick)
    planes = np.zeros((3, vol.nbricks), dtype=np.uint8)
    planes[read, b] = 1
    planes[clr] = 1                                                # whatever the plane held: it comes back zero
    after, planes_after, c, _ = dev.sweep(phase, fix, planes, s, dist=d)
    assert c == (0, visited)
    np.testing.assert_array_equal(bits(after), bits(fix))
    assert not planes_after[write].any() and not planes_after[clr].any() and np.array_equal(planes_after[read], planes[read])

    start = fix.copy()
    a = settled_voxel(vol, d, brick)
    start[a] = raised
    z = settled_voxel(vol, d, asleep) if asleep is not None else None
    if z is not None:
        start[z] = raised
    after, planes_after, c, report = dev.sweep(phase, start, planes, s, dist=d)
    want = fix.copy()
    if z is not None:
        want[z] = raised                                           # nobody looks at a sleeping brick
    np.testing.assert_array_equal(bits(after), bits(want))         # the awake one is back at the fixpoint's value exactly
    assert c == (1, visited) and report.forced_changed >= 1
    assert np.array_equal(np.flatnonzero(planes_after[write]), [b]) and planes_after[write, b] == 1 and not planes_after[clr].any()


# ---- random partial-brick volumes, extent-one axes ------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [0, 1, 2])
def test_random_volume(k):
    case = random_case(k)
    counts_d, counts_f = case.run_both(Device(case.vol))
    assert counts_d[0][1] == case.vol.nbricks == 18


@pytest.mark.parametrize("shape", M.LINE_SHAPES, ids=str)
def test_extent_one_axes(shape):
    for k in range(3):
        case = random_case(k, shape)
        case.run_both(Device(case.vol))


# ---- plane rotation -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("base", [0, 1, 2, 2 ** 32, 2 ** 40 + 2])
def test_plane_rotation(base):
    """the awake plane at base % 3: every call reads, writes and clears the planes that the model names for first_sweep = base + j;
    the plane the first call clears is planted with ones so that its clear shows too"""
    case = thread_case((1, 1, 1))
    dev = Device(case.vol)
    planes = M.start_planes(case.vol.shape, base % 3)
    planes[(base + 2) % 3] = 1
    d, planes_d, counts_d = dev.to_fixpoint(1, case.d0, case.model_d, base=base, planes=planes)
    np.testing.assert_array_equal(bits(d), bits(case.want_d))
    f, _, counts_f = dev.to_fixpoint(2, case.f0, case.model_f, dist=d, base=base, planes=planes)
    np.testing.assert_array_equal(f, case.want_f)
    assert len(counts_d) >= 4 and len(counts_f) >= 4               # every plane was read, written and cleared at least once
    # the planes after the still sweep base + n - 1: what it read is still there, what it wrote and cleared is empty
    read, write, clr = M.plane_roles(base + len(counts_d) - 1)
    assert planes_d[read].any() and not planes_d[write].any() and not planes_d[clr].any()


# ---- a batch in one call ----------------------------------------------------------------------------------------------------------------
def check_batch_relations(counts, nbricks):
    """counts: (changed, visited) per sweep from sweep 0 on, across the batches"""
    assert counts[0][1] == nbricks
    still = False
    for j, (changed, visited) in enumerate(counts):
        assert changed <= visited <= nbricks, (j, counts)
        if j >= 1:
            assert counts[j - 1][0] <= visited <= min(nbricks, 27 * counts[j - 1][0]), (j, counts)
        if still:
            assert (changed, visited) == (0, 0), (j, counts)
        still = still or changed == 0


@pytest.mark.parametrize("phase", [1, 2])
def test_batches_in_one_call(phase):
    """sweeps = 8, then 16 with first_sweep = 8, then the driver's 32 and 64 until a sweep stands still"""
    case = random_case(1)
    dev = Device(case.vol)
    state = case.d0 if phase == 1 else case.f0
    planes, counts, first = M.start_planes(case.vol.shape), [], 0
    for n in (8, 16, 32, 64, 64):
        before, planes_before = state, planes
        rc, state, planes, words = dev.call(phase, state, planes, first, sweeps=n, dist=case.want_d)
        assert rc == 0
        counts += [(int(c), int(v)) for c, v in words.reshape(n, 2)]
        assert np.all(bits(state) <= bits(before)) and np.array_equal(state[case.vol.mask == 0], before[case.vol.mask == 0])
        first += n
        if any(c == 0 for c, _ in counts):
            break
    assert any(c == 0 for c, _ in counts) and len(counts) >= 24
    check_batch_relations(counts, case.vol.nbricks)
    np.testing.assert_array_equal(bits(state), bits(case.want_d if phase == 1 else case.want_f))
    sweeps = [c for c, _ in counts].index(0) + 1
    assert sweeps <= (case.model_d if phase == 1 else case.model_f)
    if len(counts) > sweeps:
        assert not planes.any()                                    # a sweep after the still one leaves nothing in any plane
    print("relax-sweeps batches phase %d: %d (model %d)" % (phase, sweeps, case.model_d if phase == 1 else case.model_f))


# ---- a warm start, as relax_box sees it ---------------------------------------------------------------------------------------------------
def warm_start(case):
    """distances that are partly settled (half the voxels at the fixpoint, half at +inf), some pinned below the fixpoint as a
    halo's values are, junk where the mask is empty; then the same for the features on the distances' fixpoint"""
    vol = case.vol
    rng = np.random.default_rng(11)
    junk = vol.mask == 0
    d = np.where(rng.random(vol.shape) < 0.5, case.want_d, M.INF).astype(np.float32)
    reached = np.argwhere(np.isfinite(case.want_d) & (case.want_d > 0) & ~junk)
    for p in reached[rng.choice(len(reached), size=20, replace=False)]:
        d[tuple(p)] = np.float32(0.5) * case.want_d[tuple(p)]
    d[junk] = rng.choice(np.array([-3.0, 0.0, 1e30, 7.25, np.inf], dtype=np.float32), size=int(junk.sum()))
    d_fix = H.relax_box(vol.labels, d, None, vol.anisotropy, 1)
    f = np.where(rng.random(vol.shape) < 0.5, case.want_f, np.uint32(M.NONE)).astype(np.uint32)
    for p in reached[rng.choice(len(reached), size=20, replace=False)]:
        f[tuple(p)] = 0                                            # below every seed's number
    f[junk] = rng.integers(0, 2 ** 32, size=int(junk.sum()), dtype=np.uint32)
    f_fix = H.relax_box(vol.labels, d_fix, f, vol.anisotropy, 2)
    return d, d_fix, f, f_fix


def test_warm_start():
    from kimimaro_amd import feature
    case = random_case(2)
    vol = case.vol
    dev = Device(vol)
    junk = vol.mask == 0
    d, d_fix, f, f_fix = warm_start(case)
    assert np.any(bits(d_fix) != bits(case.want_d)) and np.array_equal(bits(d_fix[junk]), bits(d[junk]))
    model_d = len(vol.run(d, 1, "jacobi", check=False)[2])
    model_f = len(vol.run(f, 2, "jacobi", dist=d_fix, check=False)[2])
    got_d, _, counts_d = dev.to_fixpoint(1, d, model_d)
    np.testing.assert_array_equal(bits(got_d), bits(d_fix))        # the junk included: untouched
    got_f, _, counts_f = dev.to_fixpoint(2, f, model_f, dist=d_fix)
    np.testing.assert_array_equal(got_f, f_fix)
    assert len(counts_d) >= 2 and len(counts_f) >= 2

    # the driver on the same starts: the same fixpoints, in no more sweeps than the Jacobi order needs
    d_dist, d_feat = dev.up(d), dev.up(f)
    sweeps_d = feature.relax_box(dev.eng, dev.d_nbr, vol.shape, vol.anisotropy, d_dist)
    np.testing.assert_array_equal(bits(dev.down(d_dist, np.float32)), bits(d_fix))
    sweeps_f = feature.relax_box(dev.eng, dev.d_nbr, vol.shape, vol.anisotropy, d_dist, d_feat)
    np.testing.assert_array_equal(dev.down(d_feat, np.uint32), f_fix)
    np.testing.assert_array_equal(bits(dev.down(d_dist, np.float32)), bits(d_fix))
    assert 2 <= sweeps_d <= model_d and 2 <= sweeps_f <= model_f
    print("relax-sweeps warm start: distance %d by calls, %d by relax_box (model %d); feature %d, %d (model %d)" %
          (len(counts_d), sweeps_d, model_d, len(counts_f), sweeps_f, model_f))


# ---- feature-phase rules ------------------------------------------------------------------------------------------------------------------
def test_feature_rules():
    """two seeds at equal float distance give the smaller number, whichever side it comes from; a seed keeps its number next to a
    smaller one; voxels no seed reaches keep NONE, or whatever was planted there"""
    lab = np.zeros((70, 5, 5), dtype=np.uint8)
    lab[1:31, 1, 1] = 4
    lab[5:16, 3, 3] = 6                                            # no seed
    seeds = [((2, 1, 1), 7), ((12, 1, 1), 3), ((20, 1, 1), 9), ((21, 1, 1), 2), ((28, 1, 1), 5)]
    case = Case("rules", M.Volume(lab, (1.5, 1, 3)), seeds)
    dev = Device(case.vol)
    d, _, _ = dev.to_fixpoint(1, case.d0, case.model_d)
    np.testing.assert_array_equal(bits(d), bits(case.want_d))
    assert d[7, 1, 1] == np.float32(7.5) and d[16, 1, 1] == np.float32(6) and np.all(np.isinf(d[5:16, 3, 3]))
    f0 = case.f0.copy()
    f0[9, 3, 3] = 77
    f, _, _ = dev.to_fixpoint(2, f0, case.model_f, dist=d)
    want = case.want_f.copy()
    want[9, 3, 3] = 77
    np.testing.assert_array_equal(f, want)
    assert f[7, 1, 1] == 3 and f[6, 1, 1] == 7                     # 5 steps from 7 and from 3: the smaller number, from the high side
    assert f[16, 1, 1] == 3 and f[17, 1, 1] == 9                   # 4 steps from 3 and from 9: the smaller number, from the low side
    assert f[20, 1, 1] == 9 and f[21, 1, 1] == 2 and f[19, 1, 1] == 9
    assert np.all(f[5:9, 3, 3] == M.NONE) and np.all(f[10:16, 3, 3] == M.NONE)


# ---- the driver ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["thread", "random"])
def test_driver(which, monkeypatch):
    """feature.geodesic_voronoi(stats=): the counters of every batch, read behind the driver's back, obey the batch relations; the
    lists in the statistics are their visited counts up to and including the first sweep that changed nothing"""
    from kimimaro_amd import feature
    real, log = feature._to_fixpoint, {}

    def listening(eng, launch, shape, what):
        def recorded(dirty, changed, n, first):
            rc = launch(dirty, changed, n, first)
            eng.sync()
            log.setdefault(what, []).append((n, first, changed.cpu().numpy().view(np.uint32).reshape(n, 2).copy()))
            return rc
        return real(eng, recorded, shape, what)
    monkeypatch.setattr(feature, "_to_fixpoint", listening)
    case = thread_case((1, 1, 1)) if which == "thread" else random_case(0)
    vol = case.vol
    dev = Device(vol)
    d_lab = dev.torch.from_numpy(np.ascontiguousarray(M.flat(vol.labels.astype(np.uint8)))).to(dev.eng.device)
    sx, sy = vol.shape[:2]
    voxel = np.array([x + sx * (y + sy * z) for (x, y, z), _ in case.seeds], dtype=np.uint32)
    number = np.array([n for _, n in case.seeds], dtype=np.uint32)
    label = np.array([vol.labels[at] for at, _ in case.seeds], dtype=np.uint32)
    stats = {}
    d_dist, d_feat = feature.geodesic_voronoi(dev.eng, d_lab, 1, vol.shape, vol.anisotropy, voxel, number, label, stats=stats)
    np.testing.assert_array_equal(bits(dev.down(d_dist, np.float32)), bits(case.want_d))
    np.testing.assert_array_equal(dev.down(d_feat, np.uint32), case.want_f)
    assert stats["bricks"] == vol.nbricks
    for what, sweeps, visited, model in (("kh_geodesic_relax", stats["distance_sweeps"], stats["distance_bricks"], case.model_d),
                                         ("kh_feature_relax", stats["feature_sweeps"], stats["feature_bricks"], case.model_f)):
        batches = log[what]
        assert [(n, first) for n, first, _ in batches] == [(8, 0), (16, 8), (32, 24), (64, 56), (64, 120)][:len(batches)]
        counts = [(int(c), int(v)) for _, _, words in batches for c, v in words]
        check_batch_relations(counts, vol.nbricks)
        assert sweeps == [c for c, _ in counts].index(0) + 1 and 2 <= sweeps <= model
        assert visited == [v for _, v in counts[:sweeps]] and sweeps > sum(n for n, _, _ in batches[:-1])
    print("relax-sweeps driver %s: distance %d (model %d), feature %d (model %d)" %
          (case.name, stats["distance_sweeps"], case.model_d, stats["feature_sweeps"], case.model_f))


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("phase", [1, 2])
@pytest.mark.parametrize("sweeps,first,shape,message", [
    (0, 0, None, "geodesic relax: sweeps >= 1 and first_sweep >= 0"),
    (1, -1, None, "geodesic relax: sweeps >= 1 and first_sweep >= 0"),
    (1, 0, (0, 9, 6), "geodesic relax: the volume must hold between 1 and 2^32 - 1 voxels"),
    (1, 0, (130, 9, 0), "geodesic relax: the volume must hold between 1 and 2^32 - 1 voxels"),
], ids=["sweeps=0", "first_sweep=-1", "sx=0", "sz=0"])
def test_refusals(sweeps, first, shape, message, phase):
    from kimimaro_amd import _abi
    case = random_case(0)
    dev = Device(case.vol)
    state = case.d0 if phase == 1 else case.f0
    planes = M.start_planes(case.vol.shape)
    planes[2] = 1
    rc, after, planes_after, words = dev.call(phase, state, planes, first, sweeps=sweeps, dist=case.want_d, shape=shape)
    assert rc == KH_EINVAL and _abi.last_error() == message
    np.testing.assert_array_equal(bits(after), bits(state))
    np.testing.assert_array_equal(planes_after, planes)
    assert np.all(words == SENTINEL)
