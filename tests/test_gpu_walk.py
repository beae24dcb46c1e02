"""The predecessor walk of csrc/backtrack.h (backtrack<RAILS>) on its own: kh_path_search mode 2 takes the distances as an
argument, so the reference's fixpoint (tests/search_ref.py) is uploaded and the walk runs with no device search before it.  Inputs
and references come from tests/walk_cases.py; tests/test_walk_ref_host.py has proven, without a GPU, that every case is in the
regime it is built for (plateaus in three dimensions, a ring, two in one walk, queues of hundreds of entries, one-way edges, a
plateau that holds the source) and that tests/walk_ref.py, which restates the rule and not the kernel, agrees with the oracle.

Compared exactly: paths, the distance words (the walk writes none), the membership bytes (the visited marks of the plateau search
are bit 4 of them and must be gone) and the status word.  The capacity tests read a status the walk reports; nothing faults."""
import numpy as np
import pytest

import search_ref as R
import walk_cases as WC
import walk_ref as W

pytestmark = pytest.mark.gpu

INF_BITS = 0x7F800000
ST_PATH_OVERFLOW, ST_PLATEAU = 4, 16          # KH_ST_PATH_OVERFLOW, KH_ST_PLATEAU
SENTINEL = 0x5A5A5A5A
BEHIND = 64                                   # words behind the path buffer's capacity that must stay untouched


@pytest.fixture(scope="module")
def eng():
    from kimimaro_amd import ops
    from kimimaro_amd.engine import Engine
    e = Engine()
    ops._engine = e
    try:
        yield e
    finally:
        ops._engine = None


def search_with_distances(w):
    """ops._Search on the walk's field (and graph) with the reference's distances in d_dist[:n]; the four padding words stay +inf"""
    from kimimaro_amd import ops
    s = ops._Search(w.field, voxel_graph=w.graph)
    n = w.field.size
    s.d_dist[:n] = s.eng.torch.from_numpy(w.dist.reshape(-1, order="F").copy()).to(s.eng.device)     # (the reference is read-only)
    words = dist_words(s)
    assert np.all(words[n:] == INF_BITS) and np.array_equal(words[:n], w.dist.reshape(-1, order="F").view(np.uint32))
    return s


def dist_words(s):
    return s.d_dist.cpu().numpy().view(np.uint32).copy()


def status(s):
    from kimimaro_amd import _abi
    return int(s.ctx["d_task"].cpu().numpy().view(_abi.LABEL_T)["status"][0])


def marks_left(s):
    return int(s.ctx["d_qstate"].count_nonzero())


def source_first(w):
    return np.asarray(w.path[::-1], dtype=np.int64)


def raw_walk(s, w, cap, q_capacity=None):
    """kh_path_search mode 2 called directly on a COPY of the object's task record (so a reported status stays out of the
    object's own), into a path buffer of cap + BEHIND words filled with SENTINEL: (status, *path_length, the buffer's words)"""
    from kimimaro_amd import _abi
    eng, ctx = s.eng, s.ctx
    t, P = eng.torch, eng.ptr
    rec = ctx["d_task"].cpu().numpy().view(_abi.LABEL_T).copy()
    assert int(rec["status"][0]) == 0
    if q_capacity is not None:
        assert q_capacity <= int(rec["q_capacity"][0])          # the lists only shrink: nothing leaves the object's queues
        rec["q_capacity"] = q_capacity
    d_task = t.from_numpy(rec.view(np.uint8).reshape(-1).copy()).to(eng.device)
    d_path = t.full((cap + BEHIND,), SENTINEL, dtype=t.int32, device=eng.device)
    d_n = t.full((1,), -1, dtype=t.int32, device=eng.device)
    sx, sy, sz = s.shape
    _abi.check(eng.lib.kh_path_search(P(d_task), 2, P(ctx["d_lists"]), P(ctx["d_nbr"]), sx, sy, sz, 1.0, 1.0, 1.0, P(s.d_field),
                                      P(s.d_dist), P(ctx["d_qstate"]), P(ctx["d_queues"]), R.lin(w.source, s.shape),
                                      R.lin(w.start, s.shape), P(d_path), cap, P(d_n), int(s.graph), eng.stream()))
    st = int(d_task.cpu().numpy().view(_abi.LABEL_T)["status"][0])
    return st, int(d_n.item()), d_path.cpu().numpy().view(np.uint32)


# ---- a. the walk alone ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c["name"] for c in WC.WALK_CASES])
def test_walk_alone(eng, name):
    for w in WC.solved(name):
        s = search_with_distances(w)
        before = dist_words(s)
        src, tgt = R.lin(w.source, s.shape), R.lin(w.start, s.shape)
        for call in range(2):                                    # the second call meets what the first left behind
            got = s.run(2, src, tgt)
            print(name, w.source, "->", w.start, "call", call, "path", len(got), w.stats)
            np.testing.assert_array_equal(got, source_first(w))
            W.check_path(w.field, w.dist, [tuple(p) for p in got[::-1]], w.graph, stop=w.stop)
            np.testing.assert_array_equal(dist_words(s), before)
            assert marks_left(s) == 0, "visited marks left in the membership bytes"
            assert status(s) == 0


# ---- b. the railroad: backtrack<true>, the rail end inside the plateau ----------------------------------------------------------
@pytest.mark.parametrize("name", [c["name"] for c in WC.RAIL_CASES])
def test_railroad_from_a_plateau(eng, name):
    import oracle
    from kimimaro_amd import ops
    (w,) = WC.solved(name)
    want = np.asarray(w.path, dtype=np.int64)                    # rail end first
    got = ops.railroad(w.field, w.source, voxel_graph=w.graph)
    np.testing.assert_array_equal(got, want)
    with oracle.voxel_graph(w.graph):
        np.testing.assert_array_equal(got, oracle.railroad(w.field, w.source))
    W.check_path(w.field, w.dist, [tuple(p) for p in got], w.graph, rails=True, stop=w.stop)
    s = ops._Search(w.field, voxel_graph=w.graph)
    for _ in range(2):
        np.testing.assert_array_equal(s.run(0, R.lin(w.source, s.shape)), want)
        assert np.all(dist_words(s) == INF_BITS)
        assert marks_left(s) == 0
        assert status(s) == 0


# ---- c. path capacity ----------------------------------------------------------------------------------------------------------
def test_path_capacity_one_short_and_exact(eng):
    """the step-by-step bail (n >= cap): one word short reports the overflow and no path, the exact size gives the path"""
    w = WC.solved("field_flat")[0]
    assert w.stats["plateaus"] == 0 and len(w.path) >= 3
    s = search_with_distances(w)
    n = len(w.path)
    st, length, buf = raw_walk(s, w, n - 1)
    assert st == ST_PATH_OVERFLOW
    assert length == 0
    assert np.all(buf[n - 1:] == SENTINEL)
    assert marks_left(s) == 0
    st, length, buf = raw_walk(s, w, n)
    assert st == 0
    assert length == n
    np.testing.assert_array_equal(buf[:n], [R.lin(p, s.shape) for p in w.path[::-1]])
    assert np.all(buf[n:] == SENTINEL)
    assert marks_left(s) == 0


def test_path_capacity_inside_the_plateau_branch(eng):
    """the walk starts in the plateau, so the first thing appended is the route of the breadth-first search, which cannot fit:
    the bail of the plateau branch (n + len > cap), after the marks were cleaned"""
    w = WC.solved("absorb")[0]
    assert w.start == (11, 11, 7) and w.stats["maxroute"] > 4 and w.dist[w.path[1]] == w.dist[w.start]
    s = search_with_distances(w)
    before = dist_words(s)
    st, length, buf = raw_walk(s, w, 4)
    assert st == ST_PATH_OVERFLOW
    assert length == 0
    assert np.all(buf[4:] == SENTINEL)
    assert marks_left(s) == 0
    np.testing.assert_array_equal(dist_words(s), before)
    np.testing.assert_array_equal(s.run(2, R.lin(w.source, s.shape), R.lin(w.start, s.shape)), source_first(w))


# ---- d. the capacity of the plateau search's lists -------------------------------------------------------------------------------
def test_plateau_queue_capacity(eng):
    """a record whose lists hold 64 entries each (the first 256 words of the object's queues): the plateau's queue of hundreds
    cannot fit, the walk reports the plateau and no path, and takes its marks back; the object's own record then gives the path"""
    w = WC.solved("absorb")[0]
    assert w.stats["maxq"] > 64
    s = search_with_distances(w)
    before = dist_words(s)
    st, length, buf = raw_walk(s, w, 4 * w.field.size, q_capacity=64)
    assert st == ST_PLATEAU
    assert length == 0
    assert np.all(buf[4 * w.field.size:] == SENTINEL)
    assert marks_left(s) == 0
    np.testing.assert_array_equal(dist_words(s), before)
    assert status(s) == 0
    np.testing.assert_array_equal(s.run(2, R.lin(w.source, s.shape), R.lin(w.start, s.shape)), source_first(w))
    assert marks_left(s) == 0 and status(s) == 0


# ---- e. end to end: the device's own search, then the walk ----------------------------------------------------------------------
@pytest.mark.parametrize("name", ["absorb", "ring", "two", "absorb_graph_symmetric", "absorb_graph_one_way"])
def test_dijkstra_across_plateaus(eng, name):
    """positive weights, the regime the wide_* fields already drive sssp<2> in"""
    check_dijkstra(name)


@pytest.mark.parametrize("name", ["zslab", "zero_source"])
def test_dijkstra_with_zero_weights(eng, name):
    """The device search relaxes zero-weight edges here.  That sssp<2> (csrc/sssp.h) ends does not depend on positive weights:
      - an edge is offered only when fl(d[u] + w) is strictly below the distance word read in the same pass (`nb < dr[idx]`), and
        no word is stored between that read and the flush (stores happen in the flush alone, behind a barrier), so every store
        strictly lowers a non-negative float word: a voxel is stored finitely often, whatever the weights;
      - a list entry is made only by such a store (t_next / t_far) or by a far-list split, so the near phase ends;
      - a split raises the threshold to Tn > mn, the smallest far distance (`if (!(Tn > mn)) Tn = next_up(mn)`; with mn == 0 that
        is the smallest denormal, and the kernels are built with float denormals kept), so every split takes at least the
        entries at mn out of the far list, which only stores refill.
    The fixpoint itself is unique for any non-negative weights (fl(d + w) is monotone in d), so the words are search_ref's."""
    check_dijkstra(name)


def check_dijkstra(name):
    from kimimaro_amd import ops
    for w in WC.solved(name):
        got = ops.dijkstra(w.field, w.source, w.start, voxel_graph=w.graph)
        np.testing.assert_array_equal(got, source_first(w))
        # the same two calls on an object of the test's own: the distances the walk ran on are the reference's, and it left no mark
        s = ops._Search(w.field, voxel_graph=w.graph)
        s.run(1, R.lin(w.source, s.shape))
        n = w.field.size
        np.testing.assert_array_equal(dist_words(s)[:n], w.dist.reshape(-1, order="F").view(np.uint32))
        np.testing.assert_array_equal(s.run(2, R.lin(w.source, s.shape), R.lin(w.start, s.shape)), got)
        assert marks_left(s) == 0 and status(s) == 0
