"""The machine of kh_geodesic_relax / kh_feature_relax (csrc/feature.hip) on the host: numpy only, nothing of the
product is imported.  tests/test_relax_model_host.py runs it alone, tests/test_gpu_relax_calls.py holds every call of the kernels
against it.

The kernels relax in place and workgroups run in no defined order: a read of another brick may return any value the word held
between the start of the launch and its end.  One sweep has no single right answer, but it has an exact contract, and
`Volume.check_sweep` is that contract:

* deterministic, bit for bit: which bricks are awake (the read plane dilated by the 27 offsets) and their count in counters[1];
  voxels of sleeping bricks, voxels with an empty mask and -- in phase 2 -- voxels with d == 0 or d == +inf do not change; the
  write plane gets a 1 exactly at the awake bricks that hold a changed voxel, counters[0] counts them; the clear plane is all 0;
  the read plane is untouched;
* bounds on every voxel of an awake brick.  Values only decrease during a launch, so whatever a thread reads of a neighbour u
  lies between before[u] and after[u], and fl(. + w) and min are monotone:
      phase 1   min(before[v], min_u fl(after[u] + w))  <=  after[v]  <=  min(before[v], min_u fl(before[u] + w))
      phase 2   the same with min f(u) over the achieving neighbours (fl(d(u) + w) == d(v)) of the final d
  The upper bound is a Jacobi sweep's progress, the lower one says that nothing comes from nowhere.  Where both coincide the
  value is forced.

`Volume.simulate_sweep` is the machine itself, in two orders that both satisfy the contract: "jacobi" (every read returns the
value from before the sweep) and "bricks" (in place, one awake brick after the other: a later brick reads what an earlier one
stored).  Its knobs reach / clear / s_bits build WRONG machines, for the tests that show that the checker refuses them.

Arrays are [x, y, z]; the linear voxel index is x + sx * (y + sy * z), the brick index bx + nbx * (by + nby * bz).  Distances are
float32, features uint32 (NONE: no seed reaches), planes uint8 [3, nbricks], counters two uint32 words (bricks changed, bricks
visited).  The same-label relation is prep_ref.neighbor_mask's, the weights are feature_ref.step_length's; every sum is one
float32 addition."""
import numpy as np

import feature_ref as R
import prep_ref as P

BRICK = (64, 4, 4)                  # KH_BRICK_X / _Y / _Z
NONE = 0xFFFFFFFF
INF = np.float32(np.inf)

THREAD_SHAPE = (192, 12, 12)        # 27 whole bricks
RANDOM_SHAPE = (130, 9, 6)          # 3 x 3 x 2 bricks, partial on every axis
LINE_SHAPES = [(70, 1, 1), (1, 9, 1)]       # extent-one axes: 2 x 1 x 1 and 1 x 3 x 1 bricks
ANISOTROPIES = [(1, 1, 1), (16, 16, 40), (1.5, 1, 3)]           # random volume k runs under ANISOTROPIES[k]
STEPS = list(P.DIRECTIONS)          # mask bit k: the neighbour at STEPS[k]; also the 26 contacts of a brick with its neighbours


class Refused(AssertionError):
    """check_sweep's verdict: `clause` names the part of the contract that does not hold"""

    def __init__(self, clause, detail=""):
        super().__init__("%s: %s" % (clause, detail))
        self.clause = clause


class Report:
    """what check_sweep saw: awake bricks, changed bricks, the voxels of awake bricks the kernel may write (`open_voxels`), those
    among them whose two bounds coincide (`forced`) and the forced ones that changed (`forced_changed`)"""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def brick_grid(shape):
    return tuple((n + b - 1) // b for n, b in zip(shape, BRICK))


def brick_count(shape):
    return int(np.prod(brick_grid(shape)))


def brick_index(shape, bxyz):
    g = brick_grid(shape)
    return bxyz[0] + g[0] * (bxyz[1] + g[1] * bxyz[2])


def flat(a):
    """[x, y, z] -> the words in linear-index order"""
    return np.asfortranarray(a).reshape(-1, order="F")


def dilate(plane, shape, reach=3):
    """the bricks a read plane wakes: every brick with a set byte at one of the offsets (-1..1)^3 that has at most `reach` non-zero
    components (3: the kernel's 27; 2 and 1: wrong machines), clipped to the brick grid -> bool [nbricks]"""
    g = brick_grid(shape)
    p = np.asarray(plane).reshape(g, order="F") != 0
    pad = np.zeros(tuple(n + 2 for n in g), dtype=bool)
    pad[1:-1, 1:-1, 1:-1] = p
    out = np.zeros(g, dtype=bool)
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if (dx != 0) + (dy != 0) + (dz != 0) <= reach:
                    out |= pad[1 + dx:1 + dx + g[0], 1 + dy:1 + dy + g[1], 1 + dz:1 + dz + g[2]]
    return out.reshape(-1, order="F")


def plane_roles(s, s_bits=64):
    """(read, write, clear) plane of sweep s; s_bits = 32 is the wrong machine that keeps s in 32 bits"""
    s = int(s) & ((1 << s_bits) - 1)
    return s % 3, (s + 1) % 3, (s + 2) % 3


def start_planes(shape, plane=0):
    """every brick awake in `plane`, the other two planes zero"""
    p = np.zeros((3, brick_count(shape)), dtype=np.uint8)
    p[plane] = 1
    return p


class Volume:
    """labels [x, y, z] and an anisotropy: the masks, the 26 (step, weight, same-label) triples and the brick of every voxel"""

    def __init__(self, labels, anisotropy):
        labels = np.asarray(labels)
        assert labels.ndim == 3
        self.labels = labels
        self.shape = labels.shape
        self.anisotropy = tuple(float(np.float32(a)) for a in anisotropy)
        self.mask = P.neighbor_mask(labels).reshape(self.shape, order="F")
        self.nbricks = brick_count(self.shape)
        self.steps = [(d, np.float32(R.step_length(d, anisotropy)), ((self.mask >> np.uint32(k)) & 1).astype(bool))
                      for k, d in enumerate(STEPS)]
        g = brick_grid(self.shape)
        ix = [np.arange(n) // b for n, b in zip(self.shape, BRICK)]
        self.brick_of = ix[0][:, None, None] + g[0] * (ix[1][None, :, None] + g[1] * ix[2][None, None, :])

    # ---- one pull step over a box of voxels --------------------------------------------------------------------------------------
    def _box(self, b):
        """the voxel slices of brick b (None: the whole volume)"""
        if b is None:
            return tuple(slice(0, n) for n in self.shape)
        g = brick_grid(self.shape)
        bxyz = (b % g[0], (b // g[0]) % g[1], b // (g[0] * g[1]))
        return tuple(slice(q * e, min((q + 1) * e, n)) for q, e, n in zip(bxyz, BRICK, self.shape))

    @staticmethod
    def _shift(pad, box, d):
        return pad[tuple(slice(1 + s.start + k, 1 + s.stop + k) for s, k in zip(box, d))]

    def _pad(self, a, fill):
        pad = np.full(tuple(n + 2 for n in self.shape), fill, dtype=a.dtype)
        pad[1:-1, 1:-1, 1:-1] = a
        return pad

    def pull_dist(self, own, src, box):
        """min(own[v], min_u fl(src[u] + w)) over the same-label neighbours, for the voxels of `box`"""
        pad = self._pad(src, INF)
        best = own[box].copy()
        for d, w, same in self.steps:
            cand = self._shift(pad, box, d) + w                    # one float32 addition
            np.copyto(best, cand, where=same[box] & (cand < best))
        return best

    def achieving(self, dist):
        """per step: the voxels v that are open (0 < d(v) < +inf) and whose neighbour u at that step has fl(d(u) + w) == d(v)"""
        pad = self._pad(dist, INF)
        whole = self._box(None)
        open_ = (dist > 0) & (dist != INF)
        return open_, [same & open_ & ((self._shift(pad, whole, d) + w) == dist) for d, w, same in self.steps]

    def pull_feat(self, own, src, box, edges):
        """min(own[v], min f_src(u)) over the achieving neighbours, for the voxels of `box`"""
        pad = self._pad(src, np.uint32(NONE))
        best = own[box].copy()
        for (d, _, _), edge in zip(self.steps, edges):
            cand = self._shift(pad, box, d)
            np.copyto(best, cand, where=edge[box] & (cand < best))
        return best

    # ---- the machine ---------------------------------------------------------------------------------------------------------------
    def simulate_sweep(self, state, planes, s, phase, order, reach=3, clear=True, s_bits=64, dist=None):
        """one sweep s of phase 1 (state: the distances) or phase 2 (state: the features, dist: the final distances) ->
        (state after, planes after, counters); nothing is changed in place"""
        assert order in ("jacobi", "bricks") and phase in (1, 2)
        state, planes = state.copy(), np.array(planes, dtype=np.uint8)
        read, write, clr = plane_roles(s, s_bits)
        awake = dilate(planes[read], self.shape, reach)
        if clear:
            planes[clr] = 0                                        # every workgroup clears its byte, asleep or not
        edges = self.achieving(dist)[1] if phase == 2 else None
        before = state.copy()
        changed = 0
        for b in np.flatnonzero(awake):
            box = self._box(int(b))
            src = before if order == "jacobi" else state
            new = self.pull_dist(state, src, box) if phase == 1 else self.pull_feat(state, src, box, edges)
            if not np.array_equal(new, before[box]):
                planes[write, b] = 1
                changed += 1
            state[box] = new
        return state, planes, np.array([changed, int(awake.sum())], dtype=np.uint32)

    def run(self, state, phase, order, dist=None, first_sweep=0, planes=None, check=True, limit=None, **wrong):
        """sweeps from `first_sweep` on until one changes nothing -> (state, planes, [(changed, visited) per sweep]).  check: every
        sweep goes through check_sweep, and a Refused leaves with .sweep set to the number of the sweep (counted from 0)"""
        planes = start_planes(self.shape, first_sweep % 3) if planes is None else planes
        limit = state.size + 2 if limit is None else limit
        counts = []
        for j in range(limit):
            new, new_planes, c = self.simulate_sweep(state, planes, first_sweep + j, phase, order, dist=dist, **wrong)
            if check:
                try:
                    self.check_sweep(state, new, planes, new_planes, c, first_sweep + j, phase, dist=dist)
                except Refused as e:
                    e.sweep = j
                    raise
            state, planes = new, new_planes
            counts.append((int(c[0]), int(c[1])))
            if c[0] == 0:
                return state, planes, counts
        raise AssertionError("no fixpoint after %d sweeps" % limit)

    # ---- the contract ----------------------------------------------------------------------------------------------------------------
    def check_sweep(self, before, after, planes_before, planes_after, counters, s, phase, dist=None):
        """raises Refused(clause) or returns a Report.  before / after: the distances (phase 1) or the features (phase 2, with
        dist = the distances the call was given); planes [3, nbricks]; counters: (bricks changed, bricks visited)"""
        assert phase in (1, 2)
        before, after = np.asarray(before), np.asarray(after)
        pb = np.asarray(planes_before, dtype=np.uint8).reshape(3, self.nbricks)
        pa = np.asarray(planes_after, dtype=np.uint8).reshape(3, self.nbricks)
        counters = np.asarray(counters).astype(np.int64)
        read, write, clr = plane_roles(s)
        bits = (lambda a: a.view(np.uint32)) if phase == 1 else (lambda a: a)
        differs = bits(np.ascontiguousarray(before)) != bits(np.ascontiguousarray(after))

        def refuse_if(bad, clause, detail=""):
            if bad:
                raise Refused(clause, "sweep %d phase %d %s" % (s, phase, detail))

        awake = dilate(pb[read], self.shape)
        refuse_if(int(counters[1]) != int(awake.sum()), "visited", "counters[1] = %d, awake bricks = %d" % (counters[1], awake.sum()))
        awake_vox = awake[self.brick_of]
        refuse_if(np.any(differs & ~awake_vox), "sleeping brick written", "%d voxels" % np.count_nonzero(differs & ~awake_vox))
        refuse_if(np.any(differs & (self.mask == 0)), "empty mask written")
        if phase == 2:
            open_, edges = self.achieving(dist)
            refuse_if(np.any(differs & ~open_), "seed or unreached voxel written")
        else:
            open_ = np.ones(self.shape, dtype=bool)
        changed_bricks = np.zeros(self.nbricks, dtype=bool)
        changed_bricks[np.unique(self.brick_of[differs])] = True
        refuse_if(np.any(pa[write][changed_bricks] != 1), "write plane", "a changed brick without its byte")
        refuse_if(np.any(pa[write][~changed_bricks] != pb[write][~changed_bricks]), "write plane", "a byte of a still brick changed")
        refuse_if(int(counters[0]) != int(changed_bricks.sum()), "changed", "counters[0] = %d, changed bricks = %d" %
                  (counters[0], changed_bricks.sum()))
        refuse_if(np.any(pa[clr] != 0), "clear plane", "%d bytes left" % np.count_nonzero(pa[clr]))
        refuse_if(np.any(pa[read] != pb[read]), "read plane")

        whole = self._box(None)
        if phase == 1:
            upper = self.pull_dist(before, before, whole)
            lower = self.pull_dist(before, after, whole)
        else:
            upper = self.pull_feat(before, before, whole, edges)
            lower = self.pull_feat(before, after, whole, edges)
        live = awake_vox & (self.mask != 0) & open_
        with np.errstate(invalid="ignore"):
            refuse_if(np.any(live & ~(after <= upper)), "upper bound", "less than a Jacobi sweep's progress at %d voxels" %
                      np.count_nonzero(live & ~(after <= upper)))
            refuse_if(np.any(live & ~(after >= lower)), "lower bound", "a value from nowhere at %d voxels" %
                      np.count_nonzero(live & ~(after >= lower)))
        forced = live & (upper == lower)
        return Report(awake=int(awake.sum()), changed=int(changed_bricks.sum()), open_voxels=int(live.sum()),
                      forced=int(forced.sum()), forced_changed=int((forced & differs).sum()))


# ---- the starts ---------------------------------------------------------------------------------------------------------------------
def seeded(vol, seeds):
    """kh_geodesic_seed's state: +inf / NONE everywhere, 0 and the smallest number at every seed ((x, y, z), number) on a label"""
    d = np.full(vol.shape, INF, dtype=np.float32)
    f = np.full(vol.shape, NONE, dtype=np.uint32)
    for at, number in seeds:
        if vol.labels[at] != 0:
            d[at] = 0
            f[at] = min(int(f[at]), number)
    return d, f


def reference(vol, seeds):
    """feature_ref.geodesic_voronoi (heap Dijkstra, then the features in ascending d) in this module's words: (dist f32, feature
    u32 with NONE where no seed reaches)"""
    d, f = R.geodesic_voronoi(vol.labels, [(at, number, int(vol.labels[at])) for at, number in seeds], vol.anisotropy)
    f = f.astype(np.uint32)
    f[d == INF] = NONE
    return np.ascontiguousarray(d), np.ascontiguousarray(f)


# ---- the volumes ----------------------------------------------------------------------------------------------------------------------
EDGES = [d for d in STEPS if sum(c != 0 for c in d) == 2]
CORNERS = [d for d in STEPS if sum(c != 0 for c in d) == 3]


def thread(shape, step):
    """a one-voxel-wide label of eight voxels in a 3 x 3 x 3 brick grid: four voxels along x inside brick (1, 1, 1), the fourth in
    the brick's outermost layer towards `step`; one step in direction `step` into the neighbouring brick -- through the face, edge
    or corner the two bricks share --; three more voxels along x there.  -> (labels uint8, the voxels in order; the seed sits on the
    first).  The four voxels of the run-in lie in one row, which one wave loads before it stores: the front moves one voxel per
    sweep and reaches the crossing in sweep 3 (a step without an x component: in sweep 2, over the diagonal from the third voxel).
    After sweep 0 a brick is awake by the wake rule alone, so only that rule lets the far brick take the value."""
    assert brick_grid(shape) == (3, 3, 3) and all(n == 3 * b for n, b in zip(shape, BRICK))
    lo = [b for b in BRICK]                                         # brick (1, 1, 1): [lo, lo + BRICK)
    hi = [2 * b - 1 for b in BRICK]
    along = step[0] if step[0] else 1                               # the direction of the runs along x
    edge = [h if c > 0 else l if c < 0 else l + 1 for c, l, h in zip(step, lo, hi)]
    if step[0] == 0:
        edge[0] = lo[0] + 32
    path = [(edge[0] - along * k, edge[1], edge[2]) for k in (3, 2, 1, 0)]
    cross = tuple(e + c for e, c in zip(edge, step))
    path += [(cross[0] + along * k, cross[1], cross[2]) for k in (0, 1, 2, 3)]
    lab = np.zeros(shape, dtype=np.uint8)
    for q in path:
        lab[q] = 5
    assert len(set(path)) == 8 and all(tuple(a // b for a, b in zip(q, BRICK)) == (1, 1, 1) for q in path[:4])
    assert all(tuple(a // b for a, b in zip(q, BRICK)) == tuple(1 + c for c in step) for q in path[4:])
    return lab, path


def random_volume(seed, shape=RANDOM_SHAPE, nseeds=12):
    """coarse blocks of 15 x 3 x 3 voxels with labels 0..3, 15 % of the voxels zeroed, `nseeds` seeds numbered 1.. on random label
    voxels -> (labels uint8, [((x, y, z), number)])"""
    rng = np.random.default_rng(seed)
    block = (15, 3, 3)
    coarse = rng.integers(0, 4, size=tuple((n + b - 1) // b for n, b in zip(shape, block)), dtype=np.uint8)
    lab = coarse
    for axis, b in enumerate(block):
        lab = np.repeat(lab, b, axis=axis)
    lab = np.ascontiguousarray(lab[:shape[0], :shape[1], :shape[2]])
    lab[rng.random(shape) < 0.15] = 0
    pts = np.argwhere(lab != 0)
    pick = pts[rng.choice(len(pts), size=min(nseeds, len(pts)), replace=False)]
    return lab, [(tuple(int(c) for c in p), k + 1) for k, p in enumerate(pick)]


def random_case(k, shape=RANDOM_SHAPE):
    """random volume k under its anisotropy -> (Volume, seeds); the extent-one shapes get two seeds, so that something is left to
    relax"""
    lab, seeds = random_volume(k, shape, 12 if shape == RANDOM_SHAPE else 2)
    return Volume(lab, ANISOTROPIES[k]), seeds


def thread_case(step, anisotropy=(1.5, 1, 3)):
    lab, path = thread(THREAD_SHAPE, step)
    return Volume(lab, anisotropy), [(path[0], 1)], path
