"""GPU parity: the per-label TEASAR trace on the MI355X vs the oracle pipeline (paths bit exact)."""
import numpy as np
import pytest

from shapes import random_walk_tube, voronoi_labels
from voxel_graphs import random_graph as _random_graph

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from kimimaro_amd.engine import Engine
    return Engine()


def biggest_component(mask):
    import oracle
    cc, n = oracle.connected_components(mask)
    big = np.argmax(np.bincount(cc.ravel())[1:]) + 1
    return np.asfortranarray((cc == big).astype(np.uint8))


TUBES = [
    (0, (1, 1, 1), dict(scale=1.5, const=2, pdrf_scale=100000, pdrf_exponent=4)),
    (1, (16, 16, 40), dict(scale=4, const=8, pdrf_scale=100000, pdrf_exponent=4)),
    (2, (4, 4, 40), dict(scale=0.5, const=24, pdrf_scale=5000, pdrf_exponent=16)),
    (3, (1, 1, 1), dict(scale=1.5, const=0.5, pdrf_scale=100000, pdrf_exponent=4)),
    (4, (16, 16, 40), dict(scale=1.5, const=300, pdrf_scale=100000, pdrf_exponent=4)),
    (5, (2, 3, 5), dict(scale=2, const=4, pdrf_scale=100000, pdrf_exponent=8)),
]


@pytest.mark.parametrize("seed,an,params", TUBES)
def test_trace_paths_match_oracle(eng, seed, an, params):
    import oracle
    from oracle import pipeline as P
    from kimimaro_amd.trace import trace
    m = biggest_component(random_walk_tube((48, 44, 40), 2000 + seed, steps=60, step=3.0, radius=(1.2, 5.0)))
    dbf = oracle.edt(m, an)
    want = P.trace(m, dbf, anisotropy=an, return_paths=True, **params)
    got = trace(m, dbf, anisotropy=an, return_paths=True, _engine=eng, **params)
    assert len(got) == len(want)
    for a, b in zip(got, want):
        np.testing.assert_array_equal(a, np.asarray(b, dtype=np.int64))


def test_trace_skeleton_fields(eng):
    import oracle
    from oracle import pipeline as P
    from kimimaro_amd.trace import trace
    an = (16, 16, 40)
    m = biggest_component(random_walk_tube((40, 40, 40), 77, steps=50))
    dbf = oracle.edt(m, an)
    params = dict(scale=1.5, const=30, pdrf_scale=100000, pdrf_exponent=4)
    a = trace(m, dbf, anisotropy=an, _engine=eng, **params)
    b = P.trace(m, dbf, anisotropy=an, **params)
    np.testing.assert_array_equal(a.vertices, b.vertices)
    np.testing.assert_array_equal(a.edges, b.edges)
    np.testing.assert_array_equal(a.radii, b.radii)
    np.testing.assert_array_equal(a.transform, b.transform)


@pytest.mark.parametrize("an,nlab,shape", [((1, 1, 1), 8, (64, 64, 64)), ((16, 16, 40), 20, (96, 96, 40))])
def test_skeletonize_matches_oracle(eng, an, nlab, shape):
    import kimimaro_amd
    from oracle import pipeline as P
    lab = voronoi_labels(shape, nlab, seed=11, pts_per_label=5, step=10.0, anisotropy=an)
    params = dict(kimimaro_amd.DEFAULT_TEASAR_PARAMS)
    params["const"] = 4 * an[0]
    got = kimimaro_amd.skeletonize(lab, params, anisotropy=an, dust_threshold=100, fix_borders=False,
                                   progress=False, _engine=eng)
    want = P.skeletonize(lab, params, anisotropy=an, dust_threshold=100, fix_borders=False)
    assert sorted(got.keys()) == sorted(want.keys())
    assert len(got) > 0
    for k in got:
        np.testing.assert_array_equal(got[k].vertices, want[k].vertices)
        np.testing.assert_array_equal(got[k].edges, want[k].edges)
        np.testing.assert_allclose(got[k].radii, want[k].radii, rtol=1e-4)
        assert got[k].space == "physical" and got[k].id == k


@pytest.mark.parametrize("seed,an", [(10, (1, 1, 1)), (11, (16, 16, 40))])
def test_trace_no_fix_branching_matches_oracle(eng, seed, an):
    """fix_branching=False: parental field + path_from_parents (trace.py:155,244)."""
    import oracle
    from oracle import pipeline as P
    from kimimaro_amd.trace import trace
    m = biggest_component(random_walk_tube((44, 40, 36), 3000 + seed, steps=50, step=3.0, radius=(1.2, 4.5)))
    dbf = oracle.edt(m, an)
    params = dict(scale=1.5, const=2 * an[0], pdrf_scale=100000, pdrf_exponent=4)
    want = P.trace(m, dbf, anisotropy=an, fix_branching=False, return_paths=True, **params)
    got = trace(m, dbf, anisotropy=an, fix_branching=False, return_paths=True, _engine=eng, **params)
    assert len(got) == len(want) and len(got) > 0
    for a, b in zip(got, want):
        np.testing.assert_array_equal(a, np.asarray(b, dtype=np.int64))


@pytest.mark.parametrize("seed,an,params", TUBES)
def test_parental_field_array_matches_oracle(eng, seed, an, params):
    """dijkstra3d.parental_field as an ARRAY (kh_parental_field; SURVEY 8b, kimimaro/trace.py:155): parents = index + 1, 0 = none,
    equal to the oracle's ko_parental_field word for word; the reference's own edit `parents[tuple(root)] = 0` (trace.py:220)
    works on it, and path_from_parents (kh_path_from_parents, trace.py:244) chases it like the oracle's pointer chase."""
    import oracle
    from kimimaro_amd import ops
    ops._engine = eng
    m = biggest_component(random_walk_tube((48, 44, 40), 2000 + seed, steps=60, step=3.0, radius=(1.2, 5.0)))
    dbf = oracle.edt(m, an)
    src = oracle.first_label(m)
    daf, far = oracle.euclidean_distance_field(m, src, an)
    daf = oracle.inf2zero(daf.copy(order="F"))
    pdrf = oracle.compute_pdrf(np.max(dbf), params["pdrf_scale"], params["pdrf_exponent"], oracle.zero2inf(dbf.copy(order="F")),
                               daf, daf[far])
    want = oracle.parental_field(pdrf, far)
    got = ops.parental_field(pdrf, far)
    assert isinstance(got, np.ndarray) and got.dtype == np.uint32 and got.shape == pdrf.shape
    np.testing.assert_array_equal(got, want)
    assert got[tuple(far)] == 0 and int((got != 0).sum()) == int(m.sum()) - 1
    got[tuple(far)] = 0                                  # kimimaro/trace.py:220
    idx = np.flatnonzero(m.ravel(order="F"))
    rng = np.random.default_rng(seed)
    for loc in rng.choice(idx, size=6, replace=False).tolist() + [int(oracle.loc_of(src, m.shape))]:
        tgt = tuple(int(v) for v in oracle.locs_to_pts([loc], m.shape)[0])
        a = ops.path_from_parents(got, tgt)
        np.testing.assert_array_equal(a, oracle.path_from_parents(want, tgt))
        assert tuple(a[0]) == tuple(far) and tuple(a[-1]) == tgt
    # an edit by the caller is honoured: cutting the chain at a vertex makes that vertex the path's first point
    tgt = tuple(int(v) for v in oracle.locs_to_pts([int(idx[-1])], m.shape)[0])
    full = ops.path_from_parents(got, tgt)
    if len(full) > 3:
        cut = tuple(int(v) for v in full[len(full) // 2])
        got[cut] = 0
        np.testing.assert_array_equal(ops.path_from_parents(got, tgt), full[len(full) // 2:])


def test_manual_targets_and_root(eng):
    """border-style forced root + extra targets before/after (intake.py:486-492, trace.py:225-228)."""
    import oracle
    from oracle import pipeline as P
    from kimimaro_amd.trace import trace
    an = (16, 16, 40)
    m = biggest_component(random_walk_tube((40, 40, 32), 4242, steps=45))
    dbf = oracle.edt(m, an)
    idx = np.flatnonzero(m.ravel(order="F"))
    pts = [tuple(int(v) for v in p) for p in oracle.locs_to_pts(idx[[3, idx.size // 2, idx.size - 5, idx.size // 3]], m.shape)]
    params = dict(scale=1.5, const=40, pdrf_scale=100000, pdrf_exponent=4)
    kw = dict(anisotropy=an, root=pts[0], manual_targets_before=[pts[1], pts[2]], manual_targets_after=[pts[3]],
              return_paths=True)
    want = P.trace(m, dbf, **kw, **params)
    got = trace(m, dbf, _engine=eng, **kw, **params)
    assert len(got) == len(want)
    for a, b in zip(got, want):
        np.testing.assert_array_equal(a, np.asarray(b, dtype=np.int64))


def test_max_paths(eng):
    import oracle
    from oracle import pipeline as P
    from kimimaro_amd.trace import trace
    m = biggest_component(random_walk_tube((40, 40, 32), 99, steps=45))
    dbf = oracle.edt(m, (1, 1, 1))
    params = dict(scale=1.0, const=1.0, pdrf_scale=100000, pdrf_exponent=4)
    want = P.trace(m, dbf, max_paths=3, return_paths=True, **params)
    got = trace(m, dbf, max_paths=3, return_paths=True, _engine=eng, **params)
    assert len(got) == len(want) == 3
    for a, b in zip(got, want):
        np.testing.assert_array_equal(a, np.asarray(b, dtype=np.int64))


@pytest.mark.parametrize("hole", [False, True])
@pytest.mark.parametrize("an", [(1, 1, 1), (2, 2, 3)])
def test_soma_mode_matches_oracle(eng, hole, an):
    """soma branch (trace.py:108-134,160-168,246-251): void fill + re-EDT, soma root, free-space DAF,
    one-off invalidation, path trimming.  (dijkstra3d's free_space_radius is restated, parity unpinned.)"""
    import oracle
    from oracle import pipeline as P
    from kimimaro_amd.trace import trace
    from shapes import soma_shape
    m = soma_shape(hole=hole)
    dbf = oracle.edt(m, an)
    kw = dict(scale=1.5, const=2 * an[0], anisotropy=an, soma_detection_threshold=6 * an[0],
              soma_acceptance_threshold=10 * an[0], pdrf_scale=100000, pdrf_exponent=4,
              soma_invalidation_scale=1.0, soma_invalidation_const=1.0 * an[0], return_paths=True)
    want = P.trace(m, dbf, **kw)
    got = trace(m, dbf, _engine=eng, **kw)
    assert len(got) == len(want) and len(got) >= 4
    for a, b in zip(got, want):
        np.testing.assert_array_equal(a, np.asarray(b, dtype=np.int64))


def test_skeletonize_with_a_soma_label(eng):
    """a soma label (with an internal void) next to ordinary labels: it leaves the batch and is traced on its crop."""
    import kimimaro_amd
    from oracle import pipeline as P
    from shapes import soma_shape
    vol = np.zeros((96, 64, 64), np.uint32, order="F")
    vol[:64][soma_shape(hole=True) > 0] = 5
    vol[70:90, 10:50, 20:30] = 9
    params = dict(kimimaro_amd.DEFAULT_TEASAR_PARAMS)
    params.update(const=2, soma_detection_threshold=6, soma_acceptance_threshold=10,
                  soma_invalidation_scale=1.0, soma_invalidation_const=1.0)
    got = kimimaro_amd.skeletonize(vol, params, dust_threshold=100, fix_borders=False, _engine=eng)
    want = P.skeletonize(vol, params, dust_threshold=100, fix_borders=False)
    assert sorted(got) == sorted(want) == [5, 9]
    for k in got:
        np.testing.assert_array_equal(got[k].vertices, want[k].vertices)
        np.testing.assert_array_equal(got[k].edges, want[k].edges)


def test_skeletonize_with_two_soma_labels_side_by_side(eng):
    """two soma labels in one volume are traced side by side (Engine.soma_lanes: a host thread, an Engine and a stream each);
    the skeletons are the oracle's, and the same as with one after the other"""
    import kimimaro_amd
    from oracle import pipeline as P
    from shapes import soma_shape
    vol = np.zeros((160, 64, 64), np.uint32, order="F")
    vol[:64][soma_shape(hole=True) > 0] = 5
    vol[96:][soma_shape(hole=False)[::-1] > 0] = 7
    vol[70:90, 10:50, 20:30] = 9
    params = dict(kimimaro_amd.DEFAULT_TEASAR_PARAMS)
    params.update(const=2, soma_detection_threshold=6, soma_acceptance_threshold=10,
                  soma_invalidation_scale=1.0, soma_invalidation_const=1.0)
    assert eng.soma_lanes > 1
    got = kimimaro_amd.skeletonize(vol, params, dust_threshold=100, fix_borders=False, _engine=eng)
    assert eng._soma_pool is not None and eng._soma_pool.width == 2
    want = P.skeletonize(vol, params, dust_threshold=100, fix_borders=False)
    assert sorted(got) == sorted(want) == [5, 7, 9]
    eng.soma_lanes, keep = 1, eng.soma_lanes
    try:
        serial = kimimaro_amd.skeletonize(vol, params, dust_threshold=100, fix_borders=False, _engine=eng)
    finally:
        eng.soma_lanes = keep
    for k in got:
        np.testing.assert_array_equal(got[k].vertices, want[k].vertices)
        np.testing.assert_array_equal(got[k].edges, want[k].edges)
        np.testing.assert_array_equal(got[k].vertices, serial[k].vertices)
        np.testing.assert_array_equal(got[k].edges, serial[k].edges)


@pytest.mark.parametrize("fix_branching", [True, False])
def test_float_absorption_plateau(eng, fix_branching):
    """A 6000-voxel stick accumulates ~4.5e8 of PDRF (ulp 32) before it reaches the ball, whose centre has
    PDRF < 16: fl(d + w) == d there.  The predecessor walk must cross the plateau the same way in the
    oracle and on the GPU (BFS over equal-distance achieving neighbours)."""
    import ctypes as C
    import oracle
    from oracle import pipeline as P
    from kimimaro_amd.trace import trace
    from shapes import lollipop
    m, centre = lollipop(length=6000)
    dbf = oracle.edt(m, (1, 1, 1))
    root = centre if fix_branching else (1, m.shape[1] // 2, m.shape[2] // 2)  # big costs first, tiny ones last
    kw = dict(scale=1.5, const=2, anisotropy=(1, 1, 1), pdrf_scale=100000, pdrf_exponent=4, root=root,
              fix_branching=fix_branching, soma_detection_threshold=1e9, return_paths=True)
    L = oracle.lib()
    L.ko_get_plateau_count.restype = C.c_int64
    L.ko_get_plateau_count(1)
    want = P.trace(m, dbf, **kw)
    assert L.ko_get_plateau_count(1) >= 1, "the fixture no longer produces a plateau"
    got = trace(m, dbf, _engine=eng, **kw)
    assert len(got) == len(want) >= 1
    for a, b in zip(got, want):
        np.testing.assert_array_equal(a, np.asarray(b, dtype=np.int64))


@pytest.mark.parametrize("seed", range(12))
def test_skeletonize_fuzz_small_volumes(eng, seed):
    """random small multi-label volumes, dust_threshold 0 (single voxels, 2-voxel labels, flat volumes,
    labels touching every face) with fix_borders on and off: the whole product path vs the oracle pipeline."""
    import kimimaro_amd
    from oracle import pipeline as P
    rng = np.random.default_rng(1000 + seed)
    shape = [(24, 20, 16), (40, 9, 7), (31, 31, 1), (12, 12, 12), (50, 3, 3), (17, 23, 5)][seed % 6]
    an = [(1, 1, 1), (16, 16, 40), (4, 3, 2)][seed % 3]
    nlab = int(rng.integers(2, 9))
    lab = voronoi_labels(shape, nlab, seed=seed, pts_per_label=2, step=4.0, anisotropy=an)
    lab[rng.random(shape) < 0.25] = 0          # holes and isolated voxels
    params = dict(kimimaro_amd.DEFAULT_TEASAR_PARAMS)
    params["const"] = float(rng.choice([0.5, 2.0, 6.0])) * an[0]
    params["scale"] = float(rng.choice([0.5, 1.5, 4.0]))
    fb = bool(seed % 2)
    got = kimimaro_amd.skeletonize(lab, params, anisotropy=an, dust_threshold=0, fix_borders=fb, progress=False, _engine=eng)
    want = P.skeletonize(lab, params, anisotropy=an, dust_threshold=0, fix_borders=fb)
    assert sorted(got.keys()) == sorted(want.keys())
    for k in got:
        np.testing.assert_array_equal(got[k].vertices, want[k].vertices)
        np.testing.assert_array_equal(got[k].edges, want[k].edges)
        np.testing.assert_allclose(got[k].radii, want[k].radii, rtol=1e-4)


@pytest.mark.parametrize("sweep,slots", [(False, 3), (False, 128), (True, 3), (True, 128)])
def test_skeletonize_sweep_and_heap_paths(sweep, slots):
    """The invalidation has two implementations: the order-free level sweep (csrc/sweep.h) and the exact emulation
    of the reference's heap (csrc/heap.h, the sweep's fall-back).  Both must give the oracle's skeletons; the volume is one
    whose heaps outgrow the LDS part.  `slots` forces the two-stream split of the labels (3 of 7, and all)."""
    import kimimaro_amd
    from kimimaro_amd.engine import Engine
    from oracle import pipeline as P
    eng2 = Engine()
    eng2.split_min_voxels = 1
    eng2.split_slots = slots
    eng2.sweep = sweep
    an = (16, 16, 40)
    lab = voronoi_labels((96, 96, 40), 7, seed=5, pts_per_label=3, step=12.0, anisotropy=an)
    params = dict(kimimaro_amd.DEFAULT_TEASAR_PARAMS)
    got = kimimaro_amd.skeletonize(lab, params, anisotropy=an, dust_threshold=100, fix_borders=True,
                                   progress=False, _engine=eng2)
    want = P.skeletonize(lab, params, anisotropy=an, dust_threshold=100, fix_borders=True)
    tk = eng2.last_tasks
    if sweep:
        assert int(tk["stat_sweep_calls"].sum()) > 0
        assert int(tk["stat_sweep_calls"].sum() - tk["stat_sweep_bails"].sum()) > 0   # the sweep certified calls
    else:
        assert int(tk["stat_sweep_calls"].sum()) == 0
        assert int(tk["stat_heap_pushes"].max()) > 20000   # deep heaps: both the LDS and the HBM part are used
    assert sorted(got.keys()) == sorted(want.keys()) and len(got) >= 4
    for k in got:
        np.testing.assert_array_equal(got[k].vertices, want[k].vertices)
        np.testing.assert_array_equal(got[k].edges, want[k].edges)
        np.testing.assert_allclose(got[k].radii, want[k].radii, rtol=1e-4)


@pytest.mark.parametrize("variant", ["threads64", "threads128", "table_keys", "no_window", "tiny_arena", "narrow_window", "tiny_pool", "no_pool", "unfused", "early_labels"])
def test_sweep_storage_variants_and_their_bails(variant):
    """Round-4 storage of the sweep (pending-deadline filter, level window, recycled chunks) and its knobs: one wave / two
    waves per label, levels from the table of ranks (the fallback of round 6's integer levels), the window off, an arena a 64th of its size (calls run out of chunks: SW_BAIL_ARENA) and a
    window of 64 levels (events land beyond it: SW_BAIL_LEVEL).  A bail is a matter of speed: the skeletons are the oracle's."""
    import kimimaro_amd
    from kimimaro_amd.engine import Engine
    from oracle import pipeline as P
    eng2 = Engine()
    if variant == "threads64":
        eng2.trace_threads = 64
    elif variant == "threads128":
        eng2.trace_threads = 128
    elif variant == "table_keys":
        eng2.int_keys = False             # the table of ranks instead of the integer levels an integral anisotropy allows
    elif variant == "no_window":
        eng2.sweep_window = False
    elif variant == "tiny_arena":
        eng2.arena_divisor = 64
    elif variant == "narrow_window":
        eng2.window_cap = 64
        eng2.window_cap_always = True     # (the production rule caps only when few labels pay for it)
    elif variant == "tiny_pool":
        eng2.scratch_pool_fraction = 0.001   # heap and journal on demand from a pool that serves nobody: ghost calls are rolled back at
    elif variant == "no_pool":               # once, labels that need the heap emulation are traced again with scratch of their own
        eng2.scratch_pool = False
    elif variant == "unfused":
        eng2.fuse_edf = False                # find_root / DAF / PDRF as batch launches in front of the path kernel (what the lanes run)
    elif variant == "early_labels":
        eng2.early_labels = 3                # the three largest labels fused and first on a second stream, the rest behind batch searches
    an = (16, 16, 40)
    lab = voronoi_labels((96, 96, 40), 7, seed=5, pts_per_label=3, step=12.0, anisotropy=an)
    params = dict(kimimaro_amd.DEFAULT_TEASAR_PARAMS)
    got = kimimaro_amd.skeletonize(lab, params, anisotropy=an, dust_threshold=100, fix_borders=True,
                                   progress=False, _engine=eng2)
    want = P.skeletonize(lab, params, anisotropy=an, dust_threshold=100, fix_borders=True)
    tk = eng2.last_tasks
    calls, bails = int(tk["stat_sweep_calls"].sum()), int(tk["stat_sweep_bails"].sum())
    why = int(np.bitwise_or.reduce(tk["stat_sweep_why"].astype(np.int64)))
    assert calls > 0
    if variant == "tiny_arena":
        assert why & 4 and bails > 0          # SW_BAIL_ARENA happened and the heap emulation took those calls
    elif variant == "narrow_window":
        assert why & 8 and bails > 0          # SW_BAIL_LEVEL (an event beyond the window)
    elif variant == "tiny_pool":
        # every label whose call went to the heap emulation was refused by the pool and traced again with scratch of its own
        assert eng2.last_retries >= int(np.count_nonzero(tk["stat_heap_pushes"]))
    else:
        assert calls - bails > 0
    assert sorted(got.keys()) == sorted(want.keys()) and len(got) >= 4
    for k in got:
        np.testing.assert_array_equal(got[k].vertices, want[k].vertices)
        np.testing.assert_array_equal(got[k].edges, want[k].edges)
        np.testing.assert_allclose(got[k].radii, want[k].radii, rtol=1e-4)


def test_scratch_overflow_is_retried():
    """a label whose heap / path scratch overflows is traced again on its own with more room (the reference has no
    such limits); the others keep their results.  Scratch shrunk 64-fold, heap path only."""
    import kimimaro_amd
    from kimimaro_amd.engine import Engine
    from oracle import pipeline as P
    eng2 = Engine()
    eng2.sweep = False
    eng2.scratch_divisor = 64
    an = (16, 16, 40)
    lab = voronoi_labels((64, 64, 32), 6, seed=9, pts_per_label=3, step=10.0, anisotropy=an)
    params = dict(kimimaro_amd.DEFAULT_TEASAR_PARAMS)
    params["const"] = 50
    got = kimimaro_amd.skeletonize(lab, params, anisotropy=an, dust_threshold=100, fix_borders=False, fix_branching=False,
                                   progress=False, _engine=eng2)
    want = P.skeletonize(lab, params, anisotropy=an, dust_threshold=100, fix_borders=False, fix_branching=False)
    assert sorted(got.keys()) == sorted(want.keys()) and len(got) >= 3
    for k in got:
        np.testing.assert_array_equal(got[k].vertices, want[k].vertices)
        np.testing.assert_array_equal(got[k].edges, want[k].edges)


def test_skeletonize_fill_holes(eng):
    """fill_holes=True (kimimaro/intake.py:168-169, 747-795): a label enclosed by another one is swallowed, a
    background void is filled, a cavity open to the face of the volume is not."""
    import kimimaro_amd
    from oracle import pipeline as P
    shape = (48, 44, 40)
    g = np.stack(np.meshgrid(*[np.arange(s) for s in shape], indexing="ij"), axis=-1).astype(np.float64)
    lab = np.zeros(shape, dtype=np.uint32)
    lab[np.linalg.norm(g - (16, 20, 20), axis=-1) < 13] = 7      # a ball ...
    lab[np.linalg.norm(g - (16, 20, 20), axis=-1) < 5] = 9       # ... with another label inside
    lab[np.linalg.norm(g - (18, 28, 22), axis=-1) < 2.5] = 0     # ... and a background void
    lab[np.linalg.norm(g - (36, 20, 20), axis=-1) < 9] = 11      # a second ball
    lab[34:39, 18:23, 0:21] = 0                                  # with a tunnel open to the z = 0 face
    lab = np.asfortranarray(lab)
    params = dict(kimimaro_amd.DEFAULT_TEASAR_PARAMS)
    params["const"] = 4
    kw = dict(anisotropy=(1, 1, 1), dust_threshold=50, fix_borders=False, fill_holes=True)
    got = kimimaro_amd.skeletonize(lab, params, progress=False, _engine=eng, **kw)
    want = P.skeletonize(lab, params, **kw)
    plain = P.skeletonize(lab, params, anisotropy=(1, 1, 1), dust_threshold=50, fix_borders=False)
    assert sorted(want.keys()) == [7, 11] and 9 in plain            # label 9 was swallowed
    assert sorted(got.keys()) == sorted(want.keys())
    for k in got:
        np.testing.assert_array_equal(got[k].vertices, want[k].vertices)
        np.testing.assert_array_equal(got[k].edges, want[k].edges)
        np.testing.assert_allclose(got[k].radii, want[k].radii, rtol=1e-4)


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.uint64, np.int64])
def test_skeletonize_label_dtypes_and_object_ids(eng, dtype):
    """the public mirror takes the label dtypes kimimaro takes (kimimaro/intake.py:315-342, utility.py:58-83) and
    object_ids (intake.py:519-535); the skeletons are keyed by the original ids."""
    import kimimaro_amd
    from oracle import pipeline as P
    an = (4, 4, 10)
    base = voronoi_labels((48, 40, 24), 9, seed=21, pts_per_label=3, step=8.0, anisotropy=an)   # ids 1000..1008
    lab = np.asfortranarray((base - 1000 + 3).astype(dtype))                                     # ids 3..11
    params = dict(kimimaro_amd.DEFAULT_TEASAR_PARAMS)
    params["const"] = 10
    kw = dict(anisotropy=an, dust_threshold=50, fix_borders=True, object_ids=[3, 5, 6, 11])
    got = kimimaro_amd.skeletonize(lab, params, progress=False, _engine=eng, **kw)
    want = P.skeletonize(lab, params, **kw)
    assert sorted(got.keys()) == sorted(want.keys()) and set(got.keys()) <= {3, 5, 6, 11} and len(got) >= 3
    for k in got:
        np.testing.assert_array_equal(got[k].vertices, want[k].vertices)
        np.testing.assert_array_equal(got[k].edges, want[k].edges)
        np.testing.assert_allclose(got[k].radii, want[k].radii, rtol=1e-4)


def test_skeletonize_2d_bool_with_extra_targets(eng):
    """2-D boolean input (format_labels adds the third axis) and extra_targets_before / after (intake.py:497-504)."""
    import kimimaro_amd
    from oracle import pipeline as P
    m = random_walk_tube((90, 70, 1), 5, steps=40, step=4.0, radius=(2.0, 4.0))[:, :, 0].astype(bool)
    pts = np.argwhere(m)
    before = [tuple(int(v) for v in pts[len(pts) // 3]) + (0,)]
    after = [tuple(int(v) for v in pts[2 * len(pts) // 3]) + (0,)]
    params = dict(kimimaro_amd.DEFAULT_TEASAR_PARAMS)
    params["const"] = 3
    kw = dict(anisotropy=(1, 1, 1), dust_threshold=10, fix_borders=False, extra_targets_before=before,
              extra_targets_after=after)
    got = kimimaro_amd.skeletonize(m, params, progress=False, _engine=eng, **kw)
    want = P.skeletonize(m, params, **kw)
    assert sorted(got.keys()) == sorted(want.keys()) == [1]
    np.testing.assert_array_equal(got[1].vertices, want[1].vertices)
    np.testing.assert_array_equal(got[1].edges, want[1].edges)


def test_trace_matches_reference_trace_goldens(eng):
    """kimimaro_amd.trace.trace (the HIP path for one object) against the path lists of the reference's OWN trace()
    (tests/golden/trace_paths.npz, kimimaro/trace.py:36-267 executed in the build container): control flow of
    compute_paths incl. target stacks, max_paths, both branching modes and the soma branch."""
    import kimimaro_amd.trace as T
    import oracle
    from golden_trace import cases
    seen = 0
    for i, mask, an, kw, extra, want in cases():
        dbf = oracle.edt(mask, an, black_border=bool(np.all(mask)))
        got = T.trace(mask.astype(bool), dbf, anisotropy=an, return_paths=True, _engine=eng, **kw,
                      **{k: (list(v) if isinstance(v, list) else v) for k, v in extra.items()})
        assert len(got) == len(want), i
        for a, b in zip(got, want):
            np.testing.assert_array_equal(np.asarray(a), b, err_msg="case %d" % i)
        seen += 1
    assert seen >= 20


@pytest.mark.parametrize("sweep", [True, False])
def test_invalidate_ball_reference_goldens(sweep):
    """kh_invalidate_ball (ops.roll_invalidation_ball_inside_component) on the 60 vectors made with the COMPILED
    REFERENCE (tests/golden/invalidation_ball.npz, incl. the 99-voxel shadow case of SURVEY B-8): counts and masks bit
    exact, through the order-free sweep (with its heap fall-back) and through the heap emulation alone."""
    import os
    from kimimaro_amd import ops
    from kimimaro_amd.engine import Engine
    eng2 = Engine()
    eng2.sweep = sweep
    ops._engine = eng2
    try:
        z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "invalidation_ball.npz"))
        unpack = lambda b, shape: np.unpackbits(b)[: int(np.prod(shape))].reshape(shape, order="F").astype(np.uint8)
        for i in range(int(z["n"])):
            shape = tuple(int(v) for v in z["shape_%d" % i])
            m = np.asfortranarray(unpack(z["mask_%d" % i], shape))
            path = z["path_%d" % i]
            dbf = np.zeros(shape, np.float32, order="F")
            dbf[path[:, 0], path[:, 1], path[:, 2]] = z["dbfpath_%d" % i]
            scale, const = z["sc_%d" % i]
            cnt, out = ops.roll_invalidation_ball_inside_component(m, dbf, scale, const, z["an_%d" % i], path)
            assert out is m
            assert cnt == int(z["count_%d" % i]), i
            np.testing.assert_array_equal(out, unpack(z["after_%d" % i], shape), err_msg="case %d" % i)
    finally:
        ops._engine = None


@pytest.mark.parametrize("sweep", [True, False])
def test_invalidate_ball_voxel_graph_reference_goldens(sweep):
    """roll_invalidation_ball_inside_component(..., voxel_connectivity_graph=) (skeletontricks.pyx:380,405-416 ->
    dijkstra_invalidation.hpp:126-191) on the 40 vectors of the COMPILED REFERENCE with random connectivity graphs
    (tests/golden/invalidation_ball_graph.npz): kh_apply_voxel_graph + kh_invalidate_ball, counts and masks bit exact through
    the sweep (with its fall-back) and through the heap emulation alone, incl. the corner entries at the x faces."""
    import os
    from kimimaro_amd import ops
    from kimimaro_amd.engine import Engine
    eng2 = Engine()
    eng2.sweep = sweep
    ops._engine = eng2
    try:
        z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "invalidation_ball_graph.npz"))
        unpack = lambda b, shape: np.unpackbits(b)[: int(np.prod(shape))].reshape(shape, order="F").astype(np.uint8)
        for i in range(int(z["n"])):
            shape = tuple(int(v) for v in z["shape_%d" % i])
            m = np.asfortranarray(unpack(z["mask_%d" % i], shape))
            path = z["path_%d" % i]
            dbf = np.zeros(shape, np.float32, order="F")
            dbf[path[:, 0], path[:, 1], path[:, 2]] = z["dbfpath_%d" % i]
            scale, const = z["sc_%d" % i]
            vcg = np.asfortranarray(z["graph_%d" % i].reshape(shape, order="F"))
            cnt, out = ops.roll_invalidation_ball_inside_component(m, dbf, scale, const, z["an_%d" % i], path,
                                                                   voxel_connectivity_graph=vcg)
            assert out is m
            assert cnt == int(z["count_%d" % i]), i
            np.testing.assert_array_equal(out, unpack(z["after_%d" % i], shape), err_msg="case %d" % i)
    finally:
        ops._engine = None


def _unpack(b, shape):
    return np.unpackbits(b)[: int(np.prod(shape))].reshape(shape, order="F").astype(np.uint8)


def test_pdrf_reference_goldens(eng):
    """kh_pdrf_field (ops.compute_pdrf) on the vectors of the reference's OWN compute_pdrf (tests/golden/pdrf.npz,
    kimimaro/trace.py:315-356 loaded in the build container): bit exact incl. the +-inf background and the in-place
    normalisation of DAF; north_star's 1e-4 tolerance on PDRF floats is met with zero error.  Exponent 3 takes the
    np.power branch (device base + tail around the host numpy's own power)."""
    import os
    from kimimaro_amd import ops
    ops._engine = eng
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pdrf.npz"))
    shape = (9, 7, 5)
    done = npow = 0
    for i in range(int(z["n"])):
        dbf = np.asfortranarray(z["dbf_%d" % i].reshape(shape, order="F"))
        daf = np.asfortranarray(z["daf_in_%d" % i].reshape(shape, order="F")).copy(order="F")
        dbf_max, scale, expo, max_daf = z["par_%d" % i]
        if int(expo) & (int(expo) - 1):
            # the np.power branch (trace.py:346-347): numpy's powf is the host's (libm or SVML by CPU features), so the
            # vector made in the build container is matched to 1e-6 relative, and the same recipe evaluated by THIS host's
            # numpy bit for bit (that is what the reference would return on this machine)
            f = np.float32
            M = f(1 / (f(dbf_max) ** 1.01))
            with np.errstate(all="ignore"):
                local = np.subtract(f(1), np.multiply(dbf, M))
                np.power(local, int(expo), out=local)
                local *= f(scale)
                d2 = daf.copy(order="F")
                if max_daf != 0:
                    d2 *= (1 / f(max_daf))
                    local += d2
            out = ops.compute_pdrf(np.float32(dbf_max), scale, int(expo), dbf, daf, np.float32(max_daf))
            np.testing.assert_array_equal(out, local, err_msg="case %d (np.power branch)" % i)
            gold = z["out_%d" % i]
            fin = np.isfinite(gold)
            np.testing.assert_array_equal(np.isfinite(out.ravel(order="F")), fin)
            np.testing.assert_allclose(out.ravel(order="F")[fin], gold[fin], rtol=1e-6)
            np.testing.assert_array_equal(daf.ravel(order="F"), z["daf_out_%d" % i])
            npow += 1
            continue
        out = ops.compute_pdrf(np.float32(dbf_max), scale, int(expo), dbf, daf, np.float32(max_daf))
        np.testing.assert_array_equal(out.ravel(order="F"), z["out_%d" % i], err_msg="case %d" % i)
        np.testing.assert_array_equal(daf.ravel(order="F"), z["daf_out_%d" % i])
        done += 1
    assert done >= 8 and npow >= 1


def test_target_finder_reference_goldens(eng):
    """kh_target_max (ops.CachedTargetFinder) replays the sequences of the compiled reference's CachedTargetFinder
    (tests/golden/target_finder.npz, tie-free DAFs)."""
    import os
    from kimimaro_amd import ops
    ops._engine = eng
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "target_finder.npz"))
    for i in range(int(z["n"])):
        shape = tuple(int(v) for v in z["shape_%d" % i])
        mask = _unpack(z["mask_%d" % i], shape)
        daf = np.asfortranarray(z["daf_%d" % i].reshape(shape, order="F"))
        finder = ops.CachedTargetFinder(mask, daf)
        m = mask.copy(order="F")
        seq, kills = z["seq_%d" % i], z["kills_%d" % i]
        for step in range(seq.shape[0]):
            assert finder.find_target(m) == tuple(int(v) for v in seq[step]), (i, step)
            m = _unpack(kills[step], shape)
        assert finder.find_target(m) is None


def test_legacy_find_target_and_first_label_reference_goldens(eng):
    """kh_find_target / kh_first_label (ops.find_target, ops.first_label) on the vectors of the compiled reference's legacy
    skeletontricks.find_target (skeletontricks.pyx:331-367) and first_label (:307-326): heavy ties (first maximum of the
    x-outermost scan), negative fields, -inf inside the mask, empty mask (tests/golden/legacy_targets.npz)."""
    import os
    from kimimaro_amd import ops
    ops._engine = eng
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "legacy_targets.npz"))
    for i in range(int(z["n"])):
        shape = tuple(int(v) for v in z["shape_%d" % i])
        mask = _unpack(z["mask_%d" % i], shape)
        field = np.asfortranarray(z["field_%d" % i].reshape(shape, order="F"))
        assert ops.find_target(mask, field) == tuple(int(v) for v in z["target_%d" % i]), i
        fl = ops.first_label(mask)
        assert (fl if fl is not None else (-1, -1, -1)) == tuple(int(v) for v in z["first_%d" % i]), i


def test_point_to_point_and_dijkstra_match_oracle(eng):
    """kimimaro.trace.point_to_point (trace.py:358-390) and its dijkstra3d.dijkstra call on the HIP mirrors vs the same
    composition of oracle functions (dijkstra3d is absent from the reference tree: ties follow the canonical predecessor
    rule in both)."""
    import oracle
    from kimimaro_amd import ops
    from kimimaro_amd.trace import point_to_point
    ops._engine = eng
    for t, an in enumerate([(1, 1, 1), (16, 16, 40), (2, 3, 5)]):
        m = biggest_component(random_walk_tube((40, 36, 30), 8800 + t, steps=45, step=3.0, radius=(1.3, 4.0)))
        idx = np.flatnonzero(m.ravel(order="F"))
        start, end = (tuple(int(v) for v in p) for p in oracle.locs_to_pts(idx[[5, idx.size - 7]], m.shape))
        got = point_to_point(m, start, end, anisotropy=an, pdrf_scale=100000, pdrf_exponent=4)
        dbf = oracle.edt(m, an, black_border=True)
        dbf_max = np.max(dbf)
        dbf = oracle.zero2inf(dbf)
        daf, tgt = oracle.euclidean_distance_field(m, start, an)
        daf = oracle.inf2zero(daf)
        pdrf = oracle.compute_pdrf(dbf_max, 100000, 4, dbf, daf, daf[tgt])
        want = oracle.path_to_source(pdrf, oracle.field_distances(pdrf, end), end, start)
        np.testing.assert_array_equal(got.vertices, np.asarray(want, dtype=np.float32))
        assert got.edges.shape[0] == len(want) - 1
        w = np.asarray(want, dtype=np.int64)
        np.testing.assert_array_equal(got.radii, dbf[w[:, 0], w[:, 1], w[:, 2]])
        np.testing.assert_array_equal(ops.dijkstra(pdrf, end, start), want)


def test_target_finder_large_mask(eng):
    """kh_target_max on an object far larger than its 1024-thread block (40^3 = 64 000 voxels): every thread then keeps
    the maximum of its stride, not the first valid voxel of it (round-2 advisor finding: `best` carried the found flag,
    a bare key never beat it).  Sequence = the oracle's CachedTargetFinder order (ko_target_order, pinned to the
    reference), with kills in between; a DAF with ties checks the larger-index rule."""
    import oracle
    from oracle import pipeline as P
    from kimimaro_amd import ops
    ops._engine = eng
    shape = (40, 40, 40)
    rng = np.random.default_rng(5150)
    mask = np.ones(shape, dtype=np.uint8, order="F")
    for ties in (False, True):
        daf = rng.random(shape, dtype=np.float32) * 1000.0
        if ties:
            daf = np.floor(daf / 50.0).astype(np.float32)     # 20 distinct values: thousands of ties
        daf = np.asfortranarray(daf)
        finder = ops.CachedTargetFinder(mask, daf)
        ref = P._TargetFinder(oracle.target_order(mask, daf), shape)
        m = mask.copy(order="F")
        for step in range(12):
            got, want = finder.find_target(m), ref.find_target(m)
            assert got == want, (ties, step)
            # kill the target and a random tenth of what is left
            m[want] = 0
            m[np.asfortranarray(rng.random(shape) < 0.1)] = 0
        m[...] = 0
        assert finder.find_target(m) is None


def test_function_level_mirrors_match_oracle(eng):
    """the stand-alone entry points behind the names trace.py imports: euclidean_distance_field (field bit exact incl.
    the max location), railroad, parental_field + path_from_parents, zero2inf / inf2zero, fill -- against the oracle on
    eight random-walk tubes (three anisotropies)."""
    import oracle
    from kimimaro_amd import ops
    ops._engine = eng
    for t in range(8):
        an = [(1, 1, 1), (16, 16, 40), (40, 32, 20)][t % 3]
        m = random_walk_tube((34, 30, 26), 4400 + t, steps=40, step=3.0, radius=(1.3, 4.0))
        cc, _ = oracle.connected_components(m)
        m = np.asfortranarray((cc == np.argmax(np.bincount(cc.ravel())[1:]) + 1).astype(np.uint8))
        src = oracle.first_label(m)
        want, wloc = oracle.euclidean_distance_field(m, src, an)
        got, gloc = ops.euclidean_distance_field(m, src, anisotropy=an, return_max_location=True)
        np.testing.assert_array_equal(got, want)
        assert gloc == wloc
        dbf = oracle.zero2inf(oracle.edt(m, an))
        daf = oracle.inf2zero(want.copy(order="F"))
        pdrf = oracle.compute_pdrf(np.max(oracle.edt(m, an)), 100000, 4, dbf, daf, daf[wloc])
        field = pdrf.copy(order="F")
        field[src] = 0.0                                         # a rail at the source
        np.testing.assert_array_equal(ops.railroad(field, wloc), oracle.railroad(field, wloc))
        par = ops.parental_field(pdrf, src)
        np.testing.assert_array_equal(ops.path_from_parents(par, wloc),
                                      oracle.path_to_source(pdrf, oracle.field_distances(pdrf, src), src, wloc))
        z = oracle.edt(m, an)
        np.testing.assert_array_equal(ops.zero2inf(z.copy(order="F")), oracle.zero2inf(z.copy(order="F")))
        np.testing.assert_array_equal(ops.inf2zero(want.copy(order="F")), oracle.inf2zero(want.copy(order="F")))
    import scipy.ndimage
    from shapes import soma_shape
    h = np.asfortranarray(soma_shape(hole=True).astype(np.uint8))
    filled, n = ops.fill(h.copy(order="F"), in_place=True, return_fill_count=True)
    want = scipy.ndimage.binary_fill_holes(h)
    assert n == int(want.sum()) - int(h.sum()) and n > 0
    np.testing.assert_array_equal(filled.astype(bool), want)


@pytest.mark.parametrize("seed,an,symmetric,fix_branching", [(41, (1, 1, 1), True, True), (42, (16, 16, 40), False, True),
                                                             (43, (2, 2, 3), False, False), (44, (1, 1, 1), False, True),
                                                             (45, (16, 16, 40), True, False), (46, (4, 4, 40), False, True)])
def test_trace_with_voxel_graph_matches_oracle(eng, seed, an, symmetric, fix_branching):
    """kimimaro.trace.trace(..., voxel_graph=) (kimimaro/trace.py:139-145,155,167,240-242,257): the graph gates every search
    (root, DAF, railroad / parental field, the predecessor walks -- one-way edges when it is asymmetric) and the invalidation.
    dijkstra3d's source is absent, so this pins HIP == oracle restatement (unpinned by reference code)."""
    import oracle as K
    from oracle import pipeline as P
    from kimimaro_amd.trace import trace
    rng = np.random.default_rng(seed)
    m = biggest_component(random_walk_tube((44, 40, 36), seed, steps=34, step=2.6, radius=(2.0, 4.5)))
    dbf = K.edt(m, an, black_border=False)
    g = _random_graph(m.shape, rng, 0.08, symmetric)
    kw = dict(scale=3.0, const=2.0 * an[0], anisotropy=an, pdrf_scale=5000, pdrf_exponent=4, fix_branching=fix_branching)
    want = P.trace(m, dbf, return_paths=True, voxel_graph=g, **kw)
    got = trace(m, dbf, return_paths=True, voxel_graph=g, _engine=eng, **kw)
    assert len(got) == len(want) and len(want) > 0
    for a, b in zip(got, want):
        np.testing.assert_array_equal(np.asarray(a), np.asarray(b))
    plain = P.trace(m, dbf, return_paths=True, **kw)
    # (the graph matters on at least some of the cases: different paths than without it)
    test_trace_with_voxel_graph_matches_oracle.changed = getattr(test_trace_with_voxel_graph_matches_oracle, "changed", 0) + int(
        len(plain) != len(want) or any(not np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(plain, want)))


def test_search_mirrors_with_voxel_graph_match_oracle(eng):
    """dijkstra3d.euclidean_distance_field / railroad / dijkstra with voxel_graph= through the function-level mirrors"""
    import oracle as K
    from kimimaro_amd import ops
    ops._engine = eng
    try:
        rng = np.random.default_rng(7)
        m = biggest_component(random_walk_tube((36, 36, 30), 77, steps=30, step=2.5, radius=(2.0, 4.0)))
        an = (16, 16, 40)
        g = _random_graph(m.shape, rng, 0.15, False)
        src = tuple(int(v) for v in np.argwhere(m)[0])
        with K.voxel_graph(g):
            want, wloc = K.euclidean_distance_field(m, src, an)
        got, gloc = ops.euclidean_distance_field(m, src, an, voxel_graph=g, return_max_location=True)
        np.testing.assert_array_equal(got, want)
        assert tuple(gloc) == tuple(wloc)
        plain, _ = K.euclidean_distance_field(m, src, an)
        assert not np.array_equal(plain, want)            # the graph really lengthens some routes
        field = np.where(m != 0, rng.uniform(1.0, 9.0, m.shape), np.inf).astype(np.float32, order="F")
        rail = tuple(int(v) for v in np.argwhere(m)[-1])
        field[rail] = 0.0
        with K.voxel_graph(g):
            wpath = K.railroad(field, src)
        np.testing.assert_array_equal(ops.railroad(field, src, voxel_graph=g), wpath)
    finally:
        ops._engine = None


def test_fix_avocados_matches_oracle(eng):
    """skeletonize(fix_avocados=True) (kimimaro/intake.py:187-193, 600-704) on the MI355X -- transforms, bounding boxes and the 2-D /
    3-D fills are HIP kernels, the sets and their iteration order the reference's -- against the oracle restatement: pits merged
    into their fruits (free-standing, cut by a wall, nested), everything else untouched, skeletons equal."""
    import kimimaro_amd
    from oracle import pipeline as P
    from shapes import avocado_volume
    lab = avocado_volume()
    params = dict(kimimaro_amd.DEFAULT_TEASAR_PARAMS)
    params.update(scale=1.5, const=20, soma_detection_threshold=10.0, soma_acceptance_threshold=1e9)
    an = (4, 4, 4)
    got = kimimaro_amd.skeletonize(lab, params, anisotropy=an, dust_threshold=50, fix_borders=False, fix_avocados=True,
                                   progress=False, _engine=eng)
    want = P.skeletonize(lab, params, anisotropy=an, dust_threshold=50, fix_borders=False, fix_avocados=True)
    assert sorted(got) == sorted(want) == [11, 21, 31, 41, 51]
    for k in got:
        np.testing.assert_array_equal(got[k].vertices, want[k].vertices)
        np.testing.assert_array_equal(got[k].edges, want[k].edges)
        np.testing.assert_allclose(got[k].radii, want[k].radii, rtol=1e-4)
    # the 2-D fill the six faces of a crop go through (kh_fill_voids_nd): the outline of the IMAGE is its border
    import scipy.ndimage
    rng = np.random.default_rng(5)
    t = eng.torch
    for _ in range(6):
        img = np.asfortranarray(rng.random((int(rng.integers(1, 30)), int(rng.integers(1, 30)))) < 0.45)
        d = t.from_numpy(np.ascontiguousarray(img.astype(np.uint8).reshape(-1, order="F"))).to(eng.device)
        out, n = eng.fill_voids(d, (img.shape[0], img.shape[1], 1), ndim=2)
        wantf = scipy.ndimage.binary_fill_holes(img)
        np.testing.assert_array_equal(out.cpu().numpy().reshape(img.shape, order="F").astype(bool), wantf)
        assert n == int(wantf.sum()) - int(img.sum())
