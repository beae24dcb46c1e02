"""The labels tests/test_ghost_model_host.py runs through the model of the path loop's ghosts (tests/ghost_ref.py) and
tests/test_gpu_ghost_calls.py traces on the device: test infrastructure.  Every case stays below 4 000 object voxels.

A case is a namespace: name, mask, dbf, kw (the keyword arguments of trace(): anisotropy, TEASAR parameters, fix_branching, root,
manual targets, max_paths, soma thresholds), graph (a voxel graph or None), abandon (the paths whose ball the case's knob makes the
sweep abandon) and knob (the engine attributes that do so).  `model(case, mode)` and `oracle_paths(case)` run once per process;
nobody changes what they return.

Seeded tubes (found by a search with the model over seeds 3000-3459, like the "seeds found by search" of sweep_cases.TUBE_SPECS):
random_walk_tube((34, 30, 26), seed, steps=40, step=3.0, radius=(1.3, 4.0)), largest component, DBF = oracle.edt(black_border=False),
scale 1.5, const 2 * min(anisotropy), pdrf_scale 100 000, pdrf_exponent 4.

Combs (hand-built; the tie of sweep_cases.sequences()'s gadget on every branch that is to make ghosts).  A 3 x 3 tube along x, its
centre line the first path (DBF 1.5 there: every ball takes its cross-section, 0.5 elsewhere); branches, one voxel wide, leave it in
+y, each a later path (DBF 1.1: a branch voxel takes its two neighbours on the branch).  A TWIG leaves a branch in +x at height t.
The branch voxels below and above the twig's foot, A and B, reach the twig's first voxel w at the same key (sqrt 2); the foot itself
has DBF 0.9 and reaches nothing; A's ball (4.2) goes on along the twig for three voxels more, B's (1.5) ends at w.  Whether those
three die depends on which node of w the heap pops first: the sweep leaves them undecided, they become ghosts.  A twig of four voxels
is ghosts to its end (its voxels can be the next target, or the only voxels left); a twig of six ends in two certainly-alive
voxels, and the path from its tip runs through the ghosts and kills them for certain.  scale 1, const 0: a voxel's ball radius is
its DBF; roots and manual targets dictate the order of the paths.
"""
from types import SimpleNamespace

import numpy as np

import ghost_ref
from shapes import random_walk_tube

TEASAR = dict(pdrf_scale=100000, pdrf_exponent=4)
NON_INTEGRAL = (0.5, 1.25, 3.0)


def _case(name, mask, dbf, kw, graph=None, abandon=(), knob=None):
    assert int(np.count_nonzero(mask)) < 4000, name
    return SimpleNamespace(name=name, mask=np.asfortranarray(mask, dtype=np.uint8), dbf=np.asfortranarray(dbf, dtype=np.float32),
                           kw=kw, graph=None if graph is None else np.asfortranarray(graph, dtype=np.uint32), abandon=tuple(abandon),
                           knob=dict(knob or {}))


# ---- seeded tubes ---------------------------------------------------------------------------------------------------------------
# (seed, anisotropy, fix_branching, one-way voxel graph) -- and what the model finds there in mode "ghosts"
TUBE_SPECS = (
    (3000, (1, 1, 1), True, False),        # the first call makes ghosts, the second kills them for certain: no roll-back
    (3000, (1, 1, 1), False, False),       # the same, every path a predecessor walk (no saved rail weights)
    (3064, (1, 1, 1), True, False),        # two ghost calls, then nothing certainly valid is left: back to the first path
    (3033, (16, 16, 40), True, False),     # two ghost calls 22 paths apart, then a ghost is the farthest voxel
    (3033, (16, 16, 40), False, False),
    (3180, (16, 16, 40), True, False),     # two ghost calls in a row, all ghosts killed for certain
    (3075, NON_INTEGRAL, True, False),     # table of ranks only; the call of path 21 makes the ghost, the roll-back returns there
    (3031, (1, 2, 3), True, False),        # two roll-backs, to path 0 and to path 8
    (3440, (1, 1, 1), True, True),         # KH_TRACE_VOXEL_GRAPH: one-way edges; path 1 makes the ghosts, the finder meets one at once
                                           # (its exact flood is small: the label's heap slice holds it, no second attempt)
)


def tube(seed, an, fix_branching, graph):
    import oracle
    from voxel_graphs import random_graph
    m = random_walk_tube((34, 30, 26), seed, steps=40, step=3.0, radius=(1.3, 4.0))
    cc, _ = oracle.connected_components(m)
    m = np.asfortranarray((cc == np.argmax(np.bincount(cc.ravel())[1:]) + 1).astype(np.uint8))
    dbf = oracle.edt(m, an, black_border=False)
    g = random_graph(m.shape, np.random.default_rng(seed), 0.08, False) if graph else None
    kw = dict(anisotropy=an, scale=1.5, const=2.0 * min(an), fix_branching=fix_branching, **TEASAR)
    return _case("tube_%d_%g_%g_%g_%s%s" % ((seed,) + tuple(an) + ("rail" if fix_branching else "walk", "_graph" if graph else "")),
                 m, dbf, kw, graph=g)


# ---- combs ----------------------------------------------------------------------------------------------------------------------
ROOT = (0, 3, 3)
R_A, R_B = 4.2, 1.5


def comb(length, branches):
    """branches: (x, voxels, twig) with twig = 0 (none) or the twig's length; the twig leaves the branch at its fourth voxel.
    Returns mask, dbf, the branches' tips, the twigs' tips (None for a branch without one) and the far end of the tube."""
    ymax = 5 + max(b[1] for b in branches) + 1
    m = np.zeros((length, ymax, 7), np.uint8, order="F")
    d = np.zeros(m.shape, np.float32, order="F")
    m[:, 2:5, 2:5] = 1
    d[m != 0] = 0.5
    d[:, 3, 3] = 1.5
    tips, twigs = [], []
    for x, n, twig in branches:
        m[x, 5:5 + n, 3] = 1
        d[x, 5:5 + n, 3] = 1.1
        tips.append((x, 5 + n - 1, 3))
        twigs.append((x + twig, 8, 3) if twig else None)
        if twig:
            d[x, 7, 3], d[x, 8, 3], d[x, 9, 3] = R_A, 0.9, R_B
            m[x + 1:x + 1 + twig, 8, 3] = 1
            d[x + 1:x + 1 + twig, 8, 3] = 0.9
    return m, d, tips, twigs, (length - 1, 3, 3)


def _comb_case(name, length, branches, targets, graph=None, abandon=(), knob=None, edit=None, **kw):
    m, d, tips, twigs, far = comb(length, branches)
    if edit is not None:
        edit(m, d)
    before = [far if t == "far" else tips[t] for t in targets][::-1]          # (a LIFO stack: the last one is the first path)
    kw = dict(dict(anisotropy=(1, 1, 1), scale=1.0, const=0.0, manual_targets_before=before, **TEASAR), **kw)
    if "soma_detection_threshold" not in kw:
        kw["root"] = ROOT
    return _case(name, m, d, kw, graph=graph, abandon=abandon, knob=knob)


GHOSTS, PLAIN = lambda x, twig=4: (x, 8, twig), lambda x, n=6: (x, n, 0)
WIDE_KNOB = dict(window_cap=64, window_cap_always=True)


def _wide(m, d):
    """the wide branch (x = 20): its voxels take nothing but themselves (0.9), except the fourth, whose ball of radius 80 floods a
    line of 66 voxels next to the branch (x = 21, not on the path): the level of the line's voxel i is 1 + i * i, and the step from
    one voxel to the next outruns a window of 64 level words from i = 32 on (in the table of ranks a little later)"""
    d[20, 5:75, 3] = 0.9
    d[20, 8, 3] = 80.0
    m[21, 9:75, 3] = 1
    d[21, 9:75, 3] = 0.5


def combs():
    return [
        # two branches make ghosts (paths 1 and 2); the finder's next targets are the certainly-alive tips of their twigs, and the two
        # paths from there kill every ghost for certain: ghost calls, no roll-back
        _comb_case("comb_all_killed", 44, [GHOSTS(8, 6), GHOSTS(18, 6), PLAIN(28), PLAIN(34)], ["far", 0, 1, 2, 3]),
        # ghost calls at paths 1 and 2, plain paths 3 and 4, then the finder meets a ghost (a plain branch near the root is still
        # alive, so valid != 0): one roll-back over two ghost calls to path 1 -- not the label's first --, three later paths get their
        # rail weights back; the redone loop makes path 2's ghosts again and rolls back once more, to path 2
        _comb_case("comb_two_then_one", 44, [PLAIN(4), GHOSTS(12), GHOSTS(22), PLAIN(32), PLAIN(38)], ["far", 1, 2, 3, 4]),
        # after path 1 only the ghosts are left: valid == 0 with ghosts; once they are settled the two after-targets are taken
        # (valid == 0 for good: paths without an invalidation)
        _comb_case("comb_valid0_after", 24, [GHOSTS(8)], ["far", 0], manual_targets_after=[(5, 2, 2), (20, 4, 4)]),
        # max_paths = 4: the tube, two ghost calls, one path from a twig's tip; the other twig's ghosts are alive when the loop ends
        _comb_case("comb_max_paths", 44, [GHOSTS(8, 6), GHOSTS(18, 6), PLAIN(28)], ["far", 0, 1], max_paths=4),
        # soma mode (thresholds below the DBF of the tube's first voxel, 5.0): the one-off call around the root runs without ghosts
        # allowed, the paths lose their vertices within the soma's radius, the ghosts come with paths 1 and 2
        _comb_case("comb_soma", 44, [GHOSTS(12), GHOSTS(22), PLAIN(32)], ["far", 0, 1, 2], edit=lambda m, d: d.__setitem__((0, 3, 3), 5.0),
                   soma_detection_threshold=4.5, soma_acceptance_threshold=4.8, soma_invalidation_scale=1.0, soma_invalidation_const=0.0),
        # the sweep abandons a later call while a ghost is alive: path 1 makes ghosts, path 2 is a branch of 70 voxels whose fourth
        # voxel has a ball of radius 80 that floods a line beside the branch (_wide) -- with the level window capped at 64 words
        # (the planner's knob) an event of that ball leaves the window: SW_BAIL_LEVEL, the label rolls back to path 1; without
        # ghosts alive (after the redo, in the other modes) the same call goes to the heap at once
        _comb_case("comb_forced_bail", 30, [GHOSTS(8), PLAIN(20, 70)], ["far", 0, 1], abandon=(2,), knob=WIDE_KNOB, edit=_wide),
    ]


# ---- what the host test requires of the inputs ------------------------------------------------------------------------------------------
# every reason of a roll-back, by the case (and mode) that reaches it
REASON_CASES = {"ghost target": ("comb_two_then_one", "ghosts"), "valid == 0": ("comb_valid0_after", "ghosts"),
                "sweep abandoned": ("comb_forced_bail", "ghosts"), "paranoid": ("comb_two_then_one", "paranoid"),
                "no journal": ("comb_two_then_one", "no_journal")}
UNREACHED = ()            # (at most one reason, never "ghost target", "valid == 0" or "paranoid")
NO_ROLLBACK = "comb_all_killed"
TWO_THEN_ONE = "comb_two_then_one"
NOT_FIRST_PATH = "comb_two_then_one"
ENDS_WITH_GHOSTS = "comb_max_paths"
SOMA = "comb_soma"

# the labels of the pool test, side by side in one volume (side_by_side): three that make ghosts and two that never touch the pool
POOL_LABELS = ("comb_two_then_one", "comb_plain_a", "comb_all_killed", "comb_valid0_after", "comb_plain_b")


def plain_combs():
    """labels without a twig: every call certified, no ghost, no heap (not among cases(): they reach nothing of the machine)"""
    return [_comb_case("comb_plain_a", 30, [PLAIN(8), PLAIN(20, 9)], ["far", 0]),
            _comb_case("comb_plain_b", 36, [PLAIN(6, 5), PLAIN(16), PLAIN(28, 8)], ["far", 2])]


_cases = []


def cases():
    if not _cases:
        _cases.extend([tube(*spec) for spec in TUBE_SPECS] + combs())
        assert len(set(c.name for c in _cases)) == len(_cases)
    return _cases


def by_name(name):
    return next(c for c in cases() + plain_combs() if c.name == name)


_models, _oracle = {}, {}


def model(case, mode, soundness=False):
    key = (case.name, mode)
    if key not in _models or (soundness and not _models[key][1]):
        r = ghost_ref.trace_model(case.mask, case.dbf, voxel_graph=case.graph, mode=mode, abandon=case.abandon, soundness=soundness,
                                  **case.kw)
        _models[key] = (r, soundness)
    return _models[key][0]


def oracle_paths(case):
    if case.name not in _oracle:
        from oracle import pipeline as P
        _oracle[case.name] = P.trace(case.mask, case.dbf, voxel_graph=case.graph, return_paths=True, **case.kw)
    return _oracle[case.name]


def side_by_side(names):
    """The named cases as labels 1, 2, ... of ONE volume, stacked along z with an empty plane between them (same x and y of every
    voxel, so roots and targets keep their coordinates up to the z offset).  Returns (labels u32, dbf f32, [per label: a case on
    the whole volume -- mask = the label, its DBF, its kw with the points moved -- for the model and the oracle])."""
    parts = [by_name(n) for n in names]
    an = parts[0].kw["anisotropy"]
    assert all(p.kw["anisotropy"] == an and p.graph is None and not p.abandon for p in parts)
    sx, sy = max(p.mask.shape[0] for p in parts), max(p.mask.shape[1] for p in parts)
    sz = sum(p.mask.shape[2] + 1 for p in parts)
    lab = np.zeros((sx, sy, sz), np.uint32, order="F")
    dbf = np.zeros((sx, sy, sz), np.float32, order="F")
    out, z0 = [], 0
    for i, p in enumerate(parts):
        px, py, pz = p.mask.shape
        lab[:px, :py, z0:z0 + pz] = p.mask.astype(np.uint32) * (i + 1)
        dbf[:px, :py, z0:z0 + pz] = np.where(p.mask != 0, p.dbf, 0)
        move = lambda pt: (int(pt[0]), int(pt[1]), int(pt[2]) + z0)
        kw = dict(p.kw)
        for key in ("manual_targets_before", "manual_targets_after"):
            if kw.get(key):
                kw[key] = [move(t) for t in kw[key]]
        if kw.get("root") is not None:
            kw["root"] = move(kw["root"])
        out.append((p, kw))
        z0 += pz + 1
    whole = [_case("%s@%d" % (p.name, i + 1), lab == i + 1, np.where(lab == i + 1, dbf, 0), kw) for i, (p, kw) in enumerate(out)]
    return lab, dbf, whole
